#!/usr/bin/env python3
"""Times reconstruct_batch (cauchy_256_reconstruct_batch: chosen rows of a stripe's codeword from
its k survivors, out of place) against the route it replaces, in one process on one GPU.

Per shape three cases: one lost data row (want = 1), one lost recovery row (want = 1) and
min(k, m) lost data rows (want = min(k, m)).  The old route keeps the survivors as they are only by
copying them: a clone of blocks and rows, decode_batch in place on the clone and, for the lost
recovery row, encode_batch of all m rows into a scratch.  Both routes run in every pass.

Device-resident buffers, HIP-event times on the launch stream, mean of --reps after untimed passes
for --settle-ms (as bench.py: a fresh process's first steps run slow).  Per case it prints the new
call's time, the least it could move (k blocks read, `want` written per stripe) and that rate in
TB/s, beside the old route's steps.  Before timing, the new call's output must equal the encoder's
own rows.  For scale: a device copy runs at 6.6 TB/s read + write (profiles/r5b_ubench_floor.txt).

    python tools/reconstruct_bench.py            # k29/m4/1296 x 65 536, k128/m32/8192 x 8 192, k200/m56/65536 x 64 (as k199/m56)
    python tools/reconstruct_bench.py --scale 64 # the same shapes over 1/64 of the stripes (rehearsal)
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (k, m, block_bytes, stripes): the shapes of BASELINE.md.  k200/m56 has k + m = 256, which the
# call refuses (a row is one byte and 0xFF is reserved): the tool checks the -1 and times k199/m56,
# the nearest shape the contract admits, in its place.
CASES = [(29, 4, 1296, 65536), (128, 32, 8192, 8192), (200, 56, 65536, 64)]
NEAREST = {(200, 56): (199, 56)}
COPY_TBPS = 6.6


def timed(lh, torch, m, blocks, rows, want_rows, out, status, clone, clone_rows, scratch, reps, settle_s):
    """(new ms, clone ms, decode ms, encode ms, untimed passes): both routes per pass."""
    stream = torch.cuda.current_stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]

    def one_pass(record):
        mark = (lambda i: ev[i].record(stream)) if record else (lambda i: None)
        mark(0)
        lh.reconstruct_batch(blocks, rows, m, want_rows, out=out, status=status, stream=stream)
        mark(1)
        clone.copy_(blocks)
        clone_rows.copy_(rows)
        mark(2)
        lh.decode_batch(clone, clone_rows, m, status=status, stream=stream)
        mark(3)
        if scratch is not None:
            lh.encode_batch(clone, m, recovery=scratch, stream=stream)
        mark(4)
    t_s, warm = time.perf_counter(), 0
    while True:   # untimed passes (at least four) for settle_s
        one_pass(False)
        warm += 1
        if warm % 4 == 0:
            torch.cuda.synchronize()
            if time.perf_counter() - t_s >= settle_s:
                break
    new = cp = dec = enc = 0.0
    for i in range(reps + 1):
        one_pass(True)
        torch.cuda.synchronize()
        if i:   # the first pass warms up
            new += ev[0].elapsed_time(ev[1]) / reps
            cp += ev[1].elapsed_time(ev[2]) / reps
            dec += ev[2].elapsed_time(ev[3]) / reps
            if scratch is not None:   # (no encode step: the gap between the two events is not its time)
                enc += ev[3].elapsed_time(ev[4]) / reps
    return new, cp, dec, enc, warm


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--settle-ms", type=float, default=250.0)
    ap.add_argument("--scale", type=int, default=1, help="divide every case's stripes by this (rehearsal)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("reconstruct_bench: no GPU (times are taken on the device; there is no CPU stand-in)")
    import longhair_amd as lh
    assert lh.cauchy_256_init() == 0, lh.lib().cauchy_256_last_error()
    print(f"# reconstruct_bench: {torch.cuda.get_device_name(0)}; HIP events, mean of {args.reps} after untimed passes for "
          f"{args.settle_ms:.0f} ms; reconstruct_batch and clone + decode_batch (+ encode_batch) alternate in every pass")
    print(f"# bytes moved: the least a repair moves, k blocks read + `want` written per stripe; the old route copies k "
          f"blocks (read + write) before it decodes; device copy {COPY_TBPS} TB/s (profiles/r5b_ubench_floor.txt)")
    slower = []
    for k, m, nbytes, stripes in CASES:
        stripes = max(1, stripes // args.scale)
        if k + m > 255:
            one = torch.zeros((1, k, nbytes), dtype=torch.uint8, device="cuda")
            try:
                lh.reconstruct_batch(one, torch.arange(k, dtype=torch.uint8, device="cuda")[None].contiguous(), m,
                                     torch.full((1, 1), k, dtype=torch.uint8, device="cuda"))
                sys.exit(f"reconstruct_bench: k{k}/m{m} was accepted")
            except lh.LonghairError as e:
                assert e.code == -1, e
            nk, nm = NEAREST[(k, m)]
            print(f"# k{k}/m{m}/{nbytes}: k + m = {k + m} > 255, the call returns -1 (row 255 would be the reserved 0xFF); "
                  f"timed in its place: k{nk}/m{nm}/{nbytes}")
            k, m = nk, nm
        lh.prepare(k, m, nbytes, stripes)
        gen = torch.Generator(device="cuda").manual_seed(k * 1000 + m)
        X = torch.randint(0, 256, (stripes, k, nbytes), dtype=torch.uint8, device="cuda", generator=gen)
        rec = lh.encode_batch(X, m)
        sidx = torch.arange(stripes, device="cuda")
        clone, scratch = torch.empty_like(X), torch.empty_like(rec)
        clone_rows = torch.empty((stripes, k), dtype=torch.uint8, device="cuda")
        status = torch.empty((stripes,), dtype=torch.int8, device="cuda")
        for name, e, recovery in (("data row", 1, False), ("recovery row", 0, True), (f"{min(k, m)} data rows", min(k, m), False)):
            rows = torch.arange(k, dtype=torch.uint8, device="cuda").repeat(stripes, 1)
            if recovery:    # every data block survives; recovery row s % m is wanted
                blocks = X
                want_rows = (k + sidx % m).to(torch.uint8)[:, None].contiguous()
                exp = rec[sidx, sidx % m][:, None]
            else:           # data rows (s + i (k // e)) % k are lost, recovery row i sits in their slot
                lost = (sidx[:, None] + torch.arange(e, device="cuda")[None, :] * (k // e)) % k
                blocks = X.clone()
                blocks.scatter_(1, lost[:, :, None].expand(stripes, e, nbytes), rec[:, :e])
                rows.scatter_(1, lost, (k + torch.arange(e, device="cuda")).to(torch.uint8).repeat(stripes, 1))
                want_rows = lost.to(torch.uint8).contiguous()
                exp = torch.gather(X, 1, lost[:, :, None].expand(stripes, e, nbytes))
            want = want_rows.shape[1]
            out = torch.empty((stripes, want, nbytes), dtype=torch.uint8, device="cuda")
            lh.reconstruct_batch(blocks, rows, m, want_rows, out=out, status=status)
            kernels = lh.last_launch()
            if not (torch.equal(out, exp) and int((status != 0).sum()) == 0):
                sys.exit(f"reconstruct_bench: k{k}/m{m}/{nbytes}, {name}: the rebuilt rows differ from the encoder's")
            del exp
            new, cp, dec, enc, warm = timed(lh, torch, m, blocks, rows, want_rows, out, status, clone, clone_rows,
                                            scratch if recovery else None, args.reps, args.settle_ms / 1e3)
            old_kernels = lh.last_launch()
            old = cp + dec + enc
            moved = (k + want) * nbytes * stripes
            print(f"k{k}/m{m}/{nbytes} x {stripes}  {name:>13}  want {want:2d}  reconstruct {new:9.4f} ms  {moved / 1e9:7.3f} GB "
                  f"({k + want} blocks/stripe)  {moved / (new * 1e-3) / 1e12:6.3f} TB/s "
                  f"({100 * moved / (new * 1e-3) / 1e12 / COPY_TBPS:4.1f} % of copy) | clone {cp:8.4f} ms + decode {dec:8.4f} ms"
                  f" + encode {enc:8.4f} ms = {old:8.4f} ms | reconstruct / old {new / old:6.3f}  kernels {kernels} vs "
                  f"{old_kernels}  ({warm} untimed passes)")
            if new >= old:
                slower.append(f"k{k}/m{m}/{nbytes} {name}")
            del blocks, rows, want_rows, out
        del X, rec, clone, scratch, clone_rows, status
        torch.cuda.empty_cache()
    print("# reconstruct slower than the old route at: " + (", ".join(slower) if slower else "no case"))


if __name__ == "__main__":
    main()
