#!/usr/bin/env python3
"""Times locate_batch (cauchy_256_locate_batch: scrub, and name the corrupt block of a bad stripe)
against verify_batch of the same shape, in one process on one GPU.

Device-resident buffers, HIP-event times on the launch stream, mean of --reps after untimed
passes for --settle-ms (as bench.py: a fresh process's first steps run slow), the two calls
alternating inside every pass.  Per shape three batches: clean; one stripe in 100 with one corrupt
data byte; every stripe with one whole data block replaced.  Before timing, the statuses and rows
of the planted batch are checked against the plant.  The quantity reported is locate / verify in
the same run; expected from the code about 1 on a clean batch (the scrub, a byte read per lane
and two bytes written per stripe) and about 2 where every stripe is corrupt (each lane computes
its m syndromes once more and searches the k columns of row 1); observed 1.00-1.02 and 2.6-3.4
(DESIGN.md 6.2.5 says why).

    python tools/locate_bench.py            # k29/m4/1296 x 65 536, k128/m28/8192 x 8 192, k200/m55/65536 x 64
    python tools/locate_bench.py --scale 64 # the same shapes over 1/64 of the stripes (rehearsal)

The large shapes are bench.py's with m reduced so that k + m <= 255.  The lines also go to --out
(default profiles/locate_bench.txt)."""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

CASES = [(29, 4, 1296, 65536), (128, 28, 8192, 8192), (200, 55, 65536, 64)]   # (k, m, block_bytes, stripes)
BATCHES = ("clean", "1 stripe in 100: one data byte", "every stripe: one data block")


def timed(lh, torch, X, rec, outs, reps, settle_s):
    """(verify ms, locate ms, untimed passes): both calls per pass, events around each."""
    vstatus, status, rows = outs
    stream = torch.cuda.current_stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]

    def one_pass(record):
        if record:
            ev[0].record(stream)
        lh.verify_batch(X, rec, status=vstatus, stream=stream)
        if record:
            ev[1].record(stream)
            ev[2].record(stream)
        lh.locate_batch(X, rec, status=status, rows=rows, stream=stream)
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
    ver = loc = 0.0
    for i in range(reps + 1):
        one_pass(True)
        torch.cuda.synchronize()
        if i:   # the first pass warms up
            ver += ev[0].elapsed_time(ev[1]) / reps
            loc += ev[2].elapsed_time(ev[3]) / reps
    return ver, loc, warm


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--settle-ms", type=float, default=250.0)
    ap.add_argument("--scale", type=int, default=1, help="divide every case's stripes by this (rehearsal)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "locate_bench.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("locate_bench: no GPU (times are taken on the device; there is no CPU stand-in)")
    # The encoder only prepares the batches: no specialised module is compiled for it (two of the
    # shapes are in no cache), in the call or behind the timed passes; verify and locate have none.
    os.environ.setdefault("LONGHAIR_AMD_JIT_COMPILE", "0")
    import longhair_amd as lh
    assert lh.cauchy_256_init() == 0, lh.lib().cauchy_256_last_error()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    say(f"# locate_bench: {torch.cuda.get_device_name(0)}; HIP events, mean of {args.reps} after untimed passes for "
        f"{args.settle_ms:.0f} ms; verify_batch and locate_batch alternate in every pass")
    say("# ratio = locate_batch ms / verify_batch ms (status only) of the same batch in the same run")
    for k, m, nbytes, stripes in CASES:
        stripes = max(1, stripes // args.scale)
        gen = torch.Generator(device="cuda").manual_seed(k * 1000 + m)
        X = torch.randint(0, 256, (stripes, k, nbytes), dtype=torch.uint8, device="cuda", generator=gen)
        rec = lh.encode_batch(X, m)
        outs = (torch.empty((stripes,), dtype=torch.int8, device="cuda"), torch.empty((stripes,), dtype=torch.int8, device="cuda"),
                torch.empty((stripes,), dtype=torch.uint8, device="cuda"))
        idx = torch.arange(stripes, device="cuda")
        cols = (idx * 7 + 3) % k                                  # the corrupt data block of stripe s
        for batch in BATCHES:
            hit = torch.zeros((stripes,), dtype=torch.bool, device="cuda")
            saved = None
            if batch == BATCHES[1]:
                hit = idx % 100 == 50 % min(stripes, 100)
                at = idx[hit]
                X[at, cols[at], (at * 13) % nbytes] ^= 0x20
            elif batch == BATCHES[2]:
                hit[:] = True
                saved = X[idx, cols].clone()
                X[idx, cols] = torch.randint(0, 256, (stripes, nbytes), dtype=torch.uint8, device="cuda", generator=gen)
            status, rows = lh.locate_batch(X, rec, status=outs[1], rows=outs[2])
            kernels = lh.last_launch()
            want_status = hit.to(torch.int8)
            want_rows = torch.where(hit, cols, torch.full_like(cols, 0xFF)).to(torch.uint8)
            if not (torch.equal(status, want_status) and torch.equal(rows, want_rows)):
                sys.exit(f"locate_bench: k{k}/m{m}/{nbytes}, {batch}: statuses or rows differ from the plant")
            ver_ms, loc_ms, warm = timed(lh, torch, X, rec, outs, args.reps, args.settle_ms / 1e3)
            ok = torch.equal(outs[1], want_status) and torch.equal(outs[2], want_rows) and torch.equal(outs[0] != 0, hit)
            say(f"k{k}/m{m}/{nbytes} x {stripes}  {batch:34s} corrupt stripes {int(hit.sum()):6d}  verify {ver_ms:9.4f} ms  "
                f"locate {loc_ms:9.4f} ms  ratio {loc_ms / ver_ms:6.3f}  (2m + 2) / m = {(2 * m + 2) / m:5.3f}  ok={ok}  "
                f"kernels {kernels}  ({warm} untimed passes)")
            if not ok:
                sys.exit("locate_bench: a timed call changed its answer")
            if batch == BATCHES[1]:
                at = idx[hit]
                X[at, cols[at], (at * 13) % nbytes] ^= 0x20
            elif saved is not None:
                X[idx, cols] = saved
        del X, rec, outs
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
