#!/usr/bin/env python3
"""Times update_batch (cauchy_256_update_batch: patch the recovery blocks after c data blocks of
a stripe changed) against encode_batch of the same shape -- the re-encode it replaces -- in one
process on one GPU.

Device-resident buffers, HIP-event times on the launch stream, mean of --reps after untimed
passes for --settle-ms (as bench.py: a fresh process's first steps run slow), the two calls
alternating inside every pass.  Per case and form it prints the update's time, the bytes it
moves ((2 c or, delta form, c) + 2 m blocks per stripe: old, new, and the recovery read and
written) and that rate in TB/s, beside the encode's time over its k + m blocks.  Each form's
result is first checked against encode_batch of the patched data.  For scale: a device copy
runs at 6.6 TB/s read + write (profiles/r5b_ubench_floor.txt).

    python tools/update_bench.py            # k29/m4/1296 x 65 536 and k128/m32/8192 x 8 192
    python tools/update_bench.py --scale 64 # the same shapes over 1/64 of the stripes (rehearsal)
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [(29, 4, 1296, 65536), (128, 32, 8192, 8192)]   # (k, m, block_bytes, stripes)
COPY_TBPS = 6.6


def timed(lh, torch, k, m, X, rec, work, cols, old, new, reps, settle_s):
    """(encode ms, update ms): both calls per pass, events around each."""
    stream = torch.cuda.current_stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]

    def one_pass(record):
        if record:
            ev[0].record(stream)
        lh.encode_batch(X, m, recovery=rec, stream=stream)
        if record:
            ev[1].record(stream)
            ev[2].record(stream)
        lh.update_batch(k, work, cols, old, new, stream=stream)
        if record:
            ev[3].record(stream)
    t_s, warm = time.perf_counter(), 0
    while True:   # untimed passes (at least four) for settle_s
        one_pass(False)
        warm += 1
        if warm % 4 == 0:
            torch.cuda.synchronize()
            if time.perf_counter() - t_s >= settle_s:
                break
    enc = upd = 0.0
    for i in range(reps + 1):
        one_pass(True)
        torch.cuda.synchronize()
        if i:   # the first pass warms up
            enc += ev[0].elapsed_time(ev[1]) / reps
            upd += ev[2].elapsed_time(ev[3]) / reps
    return enc, upd, warm


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--settle-ms", type=float, default=250.0)
    ap.add_argument("--scale", type=int, default=1, help="divide every case's stripes by this (rehearsal)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("update_bench: no GPU (times are taken on the device; there is no CPU stand-in)")
    import longhair_amd as lh
    assert lh.cauchy_256_init() == 0, lh.lib().cauchy_256_last_error()
    print(f"# update_bench: {torch.cuda.get_device_name(0)}; HIP events, mean of {args.reps} after untimed passes for "
          f"{args.settle_ms:.0f} ms; encode_batch and update_batch alternate in every pass")
    print(f"# bytes moved: update (2c | c) + 2m blocks per stripe, encode k + m; device copy {COPY_TBPS} TB/s "
          "(profiles/r5b_ubench_floor.txt)")
    slower = []
    for k, m, nbytes, stripes in CASES:
        stripes = max(1, stripes // args.scale)
        lh.prepare(k, m, nbytes, stripes)
        gen = torch.Generator(device="cuda").manual_seed(k * 1000 + m)
        X = torch.randint(0, 256, (stripes, k, nbytes), dtype=torch.uint8, device="cuda", generator=gen)
        rec = lh.encode_batch(X, m)
        enc_kernels = lh.last_launch()
        for c in (1, 4):
            cols = torch.rand((stripes, k), device="cuda", generator=gen).argsort(dim=1)[:, :c].to(torch.uint8).contiguous()
            idx = cols.long()[:, :, None].expand(stripes, c, nbytes)
            old = torch.gather(X, 1, idx).contiguous()
            new = torch.randint(0, 256, (stripes, c, nbytes), dtype=torch.uint8, device="cuda", generator=gen)
            delta = old ^ new
            X.scatter_(1, idx, new)            # the patched data, re-encoded: what the update must give
            want = lh.encode_batch(X, m)
            X.scatter_(1, idx, old)
            for form, o, n in (("old+new", old, new), ("delta", delta, None)):
                work = rec.clone()
                status = lh.update_batch(k, work, cols, o, n)
                upd_kernels = lh.last_launch()
                torch.cuda.synchronize()
                ok = bool(torch.equal(work, want)) and int((status != 0).sum()) == 0
                enc_ms, upd_ms, warm = timed(lh, torch, k, m, X, rec, work, cols, o, n, args.reps, args.settle_ms / 1e3)
                blocks = (c if n is None else 2 * c) + 2 * m
                moved = blocks * nbytes * stripes
                enc_moved = (k + m) * nbytes * stripes
                print(f"k{k}/m{m}/{nbytes} x {stripes}  c={c} {form:7s}  update {upd_ms:8.4f} ms  {moved / 1e9:7.3f} GB "
                      f"({blocks} blocks/stripe)  {moved / (upd_ms * 1e-3) / 1e12:6.3f} TB/s "
                      f"({100 * moved / (upd_ms * 1e-3) / 1e12 / COPY_TBPS:4.1f} % of copy) | encode {enc_ms:8.4f} ms  "
                      f"{enc_moved / 1e9:7.3f} GB ({k + m} blocks/stripe)  {enc_moved / (enc_ms * 1e-3) / 1e12:6.3f} TB/s | "
                      f"update / encode {upd_ms / enc_ms:5.3f}  ok={ok}  kernels {upd_kernels} vs {enc_kernels}  "
                      f"({warm} untimed passes)")
                if not ok:
                    sys.exit("update_bench: the update differs from the re-encode of the patched data")
                if upd_ms >= enc_ms:
                    slower.append((k, m, nbytes, c, form))
            del old, new, delta, want, work
        del X, rec
        torch.cuda.empty_cache()
    print("# update slower than the re-encode at: " + (", ".join(map(str, slower)) if slower else "no case"))


if __name__ == "__main__":
    main()
