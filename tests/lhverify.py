"""Shared helpers of the recovery-scrub tests (cauchy_256_verify_batch, test infrastructure).

The expectation is always first principles: row r of stripe s is bad iff the stored recovery
bytes differ from the C oracle's encode of the *stored* data (`expected`).  `syndrome` is the
kernel's arithmetic in numpy (lhupdate.model_update over all k columns, from the stored recovery
words); tests/test_verify_model.py pins it to the oracle.  `positions` / `tile_rows` choose where
a corruption goes so that every class of the kernel's lanes and row tiles is hit, and
`corrupt_case` builds one mixed batch."""
import functools

import numpy as np

import lhupdate
import lhutil

LANE, FLAT_LANE, TILE = 8, 16, 4   # kernels.hip: bytes per lane and sub-block; flat lanes; rows per tile
STYLES = ("clean", "rec-byte", "two-rows", "data-bit", "swapped-block")


def is_flat(k, m):
    return m == 1 or k == 1


def geometry(k, m, nbytes):
    """(sub-blocks, span, lane bytes, lanes per stripe) of lh_verify_kernel for a shape."""
    if is_flat(k, m):
        return 1, nbytes, FLAT_LANE, -(-nbytes // FLAT_LANE)
    sub = nbytes // 8
    return 8, sub, LANE, -(-sub // LANE)


def stripes_per_workgroup(k, m, nbytes):
    return max(1, 256 // geometry(k, m, nbytes)[3])


def syndrome(k, m, nbytes, data, rec, rows):
    """recovery_r ^ sum_j B(G[r][j]) data_j for one stripe, uint8 [m, nbytes]."""
    return lhupdate.model_update(k, m, nbytes, rec, list(range(k)), np.asarray(data).reshape(k, nbytes), rows)


def expected(oracle, k, m, nbytes, data, rec):
    """(status int8 [S], bad_rows uint8 [S, m]) of stored data [S, k, B] and recovery [S, m, B]."""
    S = data.shape[0]
    bad = np.zeros((S, m), dtype=np.uint8)
    for s in range(S):
        rc, r = oracle.encode(k, m, data[s], nbytes)
        assert rc == 0, (k, m, nbytes, rc)
        bad[s] = (r.reshape(m, nbytes) != rec[s]).any(axis=1)
    return bad.any(axis=1).astype(np.int8), bad


@functools.lru_cache(maxsize=None)
def encoded(oracle, k, m, nbytes, stripes, seed):
    """`stripes` stripes of lhutil.fill data with the oracle's recovery blocks, read-only."""
    data = lhutil.fill(seed, stripes * k * nbytes).reshape(stripes, k, nbytes)
    rec = np.empty((stripes, m, nbytes), dtype=np.uint8)
    for s in range(stripes):
        rc, r = oracle.encode(k, m, data[s], nbytes)
        assert rc == 0
        rec[s] = r.reshape(m, nbytes)
    for a in (data, rec):
        a.setflags(write=False)
    return data, rec


def lane_class(k, m, nbytes, p):
    """The classes of byte p of a block, by the lane of lh_verify_kernel that reads it:
    'first' / 'last' byte of a sub-block; 'piecewise' (a span under one lane), 'whole' (a lane
    at its own place), 'overlap' (the neighbour's bytes in the last lane's window, read twice),
    'tail' (the bytes only the shifted last lane covers)."""
    _, span, lane, nch = geometry(k, m, nbytes)
    o = p % span
    out = set()
    if o == 0:
        out.add("first")
    if o == span - 1:
        out.add("last")
    if span < lane:
        out.add("piecewise")
    elif span % lane == 0 or o < (nch - 1) * lane:
        out.add("whole")
        if span % lane and o >= span - lane:
            out.add("overlap")
    else:
        out.add("tail")
    return out


def positions(k, m, nbytes, seed, extra=3):
    """Byte positions of a block worth corrupting, ascending and unique: the first and the last
    byte of every sub-block, the first byte of the last lane's overlapped window and the first
    byte it alone covers (where the span is no multiple of the lane), and `extra` random ones."""
    ns, span, lane, nch = geometry(k, m, nbytes)
    offs = {0, span - 1}
    if span > lane and span % lane:
        offs.update((span - lane, (nch - 1) * lane))
    out = {y * span + o for y in range(ns) for o in offs}
    rng = np.random.Generator(np.random.PCG64(seed))
    out.update(int(p) for p in rng.integers(0, nbytes, size=extra))
    return sorted(out)


def tile_rows(m):
    """The first and the last row of every row tile, the partial last tile included."""
    return sorted({r for i0 in range(0, m, TILE) for r in (i0, min(i0 + TILE, m) - 1)})


def corrupt_case(oracle, k, m, nbytes, stripes, seed):
    """A mixed batch: STYLES cycle over the stripes (clean; one recovery byte; two recovery rows;
    one data bit; a recovery block replaced by the next stripe's), the bytes from `positions` and
    the rows from `tile_rows`, both walked in order so that every one is used when the batch is
    long enough.  Returns read-only (data, rec, status, bad_rows, plan) with the expectation from
    `expected` and plan[s] = (style, rows meant to be bad)."""
    data0, rec0 = encoded(oracle, k, m, nbytes, stripes, seed)
    data, rec = data0.copy(), rec0.copy()
    pos, rows = positions(k, m, nbytes, seed), tile_rows(m)
    plan = []
    n = 0   # corruptions placed so far: walks pos and rows
    for s in range(stripes):
        style = STYLES[s % len(STYLES)]
        p, r = pos[n % len(pos)], rows[n % len(rows)]
        bit = np.uint8(1 << (n % 8))
        meant = []
        if style == "rec-byte":
            rec[s, r, p] ^= bit
            meant = [r]
        elif style == "two-rows":
            r2 = rows[(n + 1) % len(rows)] if len(rows) > 1 else r
            rec[s, r, p] ^= bit
            rec[s, r2, pos[(n + 1) % len(pos)]] ^= np.uint8(0x80)
            meant = sorted({r, r2})
        elif style == "data-bit":
            data[s, n % k, p] ^= bit
            meant = list(range(m))
        elif style == "swapped-block":
            rec[s, r] = rec0[(s + 1) % stripes, r]
            meant = [r]
        if style != "clean":
            n += 1
        plan.append((style, meant))
    status, bad = expected(oracle, k, m, nbytes, data, rec)
    for s, (style, meant) in enumerate(plan):   # the generator plants what it says it plants
        assert np.nonzero(bad[s])[0].tolist() == meant, (k, m, nbytes, s, style, meant)
    for a in (data, rec, status, bad):
        a.setflags(write=False)
    return data, rec, status, bad, plan


def byte_sweep_recovery(oracle, k, m, nbytes, seed):
    """nbytes * m stripes: stripe p * m + r has one bit of byte p of recovery row r flipped."""
    S = nbytes * m
    data, rec0 = encoded(oracle, k, m, nbytes, S, seed)
    rec = rec0.copy()
    for p in range(nbytes):
        for r in range(m):
            rec[p * m + r, r, p] ^= np.uint8(1 << ((p + r) % 8))
    return data, rec


def byte_sweep_data(oracle, k, m, nbytes, seed):
    """nbytes stripes: stripe p has one bit of byte p of data block p % k flipped."""
    data0, rec = encoded(oracle, k, m, nbytes, nbytes, seed)
    data = data0.copy()
    for p in range(nbytes):
        data[p, p % k, p] ^= np.uint8(1 << (p % 8))
    return data, rec
