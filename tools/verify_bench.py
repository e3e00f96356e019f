#!/usr/bin/env python3
"""Times verify_batch (cauchy_256_verify_batch: do the stored recovery blocks still belong to the
stored data?) against the scrub it replaces -- encode_batch into a preallocated scratch the size
of the recovery blocks, then the per-stripe compare (scratch != recovery).flatten(1).any(1) -- in
one process on one GPU.

Device-resident buffers, HIP-event times on the launch stream, mean of --reps after untimed
passes for --settle-ms (as bench.py: a fresh process's first steps run slow), the two routes
alternating inside every pass.  Per case it prints the verify's time, the bytes it moves (k + m
blocks per stripe, read once) and that rate in TB/s, beside the encode's and the compare's
times.  Before timing, verify must return all zeros on the encoder's own output and flag one
planted corruption (stripe and row).  For scale: a device copy runs at 6.6 TB/s read + write
(profiles/r5b_ubench_floor.txt).

    python tools/verify_bench.py            # k29/m4/1296 x 65 536, k128/m32/8192 x 8 192, k200/m56/65536 x 64
    python tools/verify_bench.py --scale 64 # the same shapes over 1/64 of the stripes (rehearsal)
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [(29, 4, 1296, 65536), (128, 32, 8192, 8192), (200, 56, 65536, 64)]   # (k, m, block_bytes, stripes)
COPY_TBPS = 6.6


def timed(lh, torch, m, X, rec, scratch, status, bad, reps, settle_s):
    """(encode ms, compare ms, verify ms, untimed passes): both routes per pass, events around each step."""
    stream = torch.cuda.current_stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]

    def one_pass(record):
        if record:
            ev[0].record(stream)
        lh.encode_batch(X, m, recovery=scratch, stream=stream)
        if record:
            ev[1].record(stream)
        differs = (scratch != rec).flatten(1).any(1)
        if record:
            ev[2].record(stream)
            ev[3].record(stream)
        lh.verify_batch(X, rec, status=status, bad_rows=bad, stream=stream)
        if record:
            ev[4].record(stream)
        return differs
    t_s, warm = time.perf_counter(), 0
    while True:   # untimed passes (at least four) for settle_s
        one_pass(False)
        warm += 1
        if warm % 4 == 0:
            torch.cuda.synchronize()
            if time.perf_counter() - t_s >= settle_s:
                break
    enc = cmp_ = ver = 0.0
    for i in range(reps + 1):
        one_pass(True)
        torch.cuda.synchronize()
        if i:   # the first pass warms up
            enc += ev[0].elapsed_time(ev[1]) / reps
            cmp_ += ev[1].elapsed_time(ev[2]) / reps
            ver += ev[3].elapsed_time(ev[4]) / reps
    return enc, cmp_, ver, warm


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--settle-ms", type=float, default=250.0)
    ap.add_argument("--scale", type=int, default=1, help="divide every case's stripes by this (rehearsal)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("verify_bench: no GPU (times are taken on the device; there is no CPU stand-in)")
    import longhair_amd as lh
    assert lh.cauchy_256_init() == 0, lh.lib().cauchy_256_last_error()
    print(f"# verify_bench: {torch.cuda.get_device_name(0)}; HIP events, mean of {args.reps} after untimed passes for "
          f"{args.settle_ms:.0f} ms; encode_batch + compare and verify_batch alternate in every pass")
    print(f"# bytes moved: verify k + m blocks per stripe (read once, no scratch); encode + compare k + 3m blocks and m blocks "
          f"of scratch; device copy {COPY_TBPS} TB/s (profiles/r5b_ubench_floor.txt)")
    slower = []
    for k, m, nbytes, stripes in CASES:
        stripes = max(1, stripes // args.scale)
        lh.prepare(k, m, nbytes, stripes)
        gen = torch.Generator(device="cuda").manual_seed(k * 1000 + m)
        X = torch.randint(0, 256, (stripes, k, nbytes), dtype=torch.uint8, device="cuda", generator=gen)
        rec = lh.encode_batch(X, m)
        enc_kernels = lh.last_launch()
        scratch = torch.empty_like(rec)
        status = torch.empty((stripes,), dtype=torch.int8, device="cuda")
        bad = torch.empty((stripes, m), dtype=torch.uint8, device="cuda")
        lh.verify_batch(X, rec, status=status, bad_rows=bad)
        ver_kernels = lh.last_launch()
        ok = int((status != 0).sum()) == 0 and int((bad != 0).sum()) == 0
        s, r, p = stripes // 2, m - 1, nbytes - 1      # one planted corruption
        rec[s, r, p] ^= 0x40
        lh.verify_batch(X, rec, status=status, bad_rows=bad)
        ok = ok and int(status.sum()) == 1 and int(status[s]) == 1 and int(bad.sum()) == 1 and int(bad[s, r]) == 1
        rec[s, r, p] ^= 0x40
        if not ok:
            sys.exit(f"verify_bench: k{k}/m{m}/{nbytes}: verify is wrong on the encoder's output or misses the planted corruption")
        enc_ms, cmp_ms, ver_ms, warm = timed(lh, torch, m, X, rec, scratch, status, bad, args.reps, args.settle_ms / 1e3)
        torch.cuda.synchronize()
        ok = int((status != 0).sum()) == 0
        moved = (k + m) * nbytes * stripes
        old_ms = enc_ms + cmp_ms
        print(f"k{k}/m{m}/{nbytes} x {stripes}  verify {ver_ms:9.4f} ms  {moved / 1e9:7.3f} GB ({k + m} blocks/stripe)  "
              f"{moved / (ver_ms * 1e-3) / 1e12:6.3f} TB/s ({100 * moved / (ver_ms * 1e-3) / 1e12 / COPY_TBPS:4.1f} % of copy) | "
              f"encode {enc_ms:8.4f} ms + compare {cmp_ms:8.4f} ms = {old_ms:8.4f} ms, {m * nbytes * stripes / 1e9:6.3f} GB scratch | "
              f"verify / (encode + compare) {ver_ms / old_ms:6.3f}  ok={ok}  kernels {ver_kernels} vs {enc_kernels}  "
              f"({warm} untimed passes)")
        if not ok:
            sys.exit("verify_bench: a timed verify flagged clean stripes")
        if ver_ms >= old_ms:
            slower.append((k, m, nbytes))
        del X, rec, scratch, status, bad
        torch.cuda.empty_cache()
    print("# verify slower than encode + compare at: " + (", ".join(map(str, slower)) if slower else "no case"))


if __name__ == "__main__":
    main()
