"""Shared helpers of the locate tests (cauchy_256_locate_batch, test infrastructure).

The expectation is the contract of include/cauchy_256_locate.h, never the kernel: `model_locate`
takes the syndromes (lhverify.syndrome) and applies the definition literally -- is the syndrome
that of an error in block x only, for every x -- and tests/test_locate_model.py pins it to the C
oracle, where the same question is asked with no syndrome arithmetic at all (`definition_locate`:
rebuild block x from the others, does the stripe encode to its stored recovery?).  The planting
helpers corrupt one bit, one byte or a whole block, at the positions of lhverify.positions and the
recovery rows of lhverify.tile_rows, and two blocks at different offsets of the sub-block span;
every plant's meant answer is checked against the model before a test uses it."""
import functools

import numpy as np

import lhupdate
import lhverify

NONE = 0xFF   # "no row"
CLEAN, ONE, MANY = 0, 1, 2
STYLES = ("clean", "data-bit", "data-block", "rec-byte", "rec0-byte", "two-recs", "two-data", "data+rec")


def mul(k, m, nbytes, e, block):
    """B(e) block, uint8 [nbytes] (the plain copy when the shape is flat: every coefficient is 1)."""
    block = np.asarray(block, dtype=np.uint8)
    if lhverify.is_flat(k, m):
        return block.copy()
    sub = nbytes // 8
    v = lhupdate.ladder(block.reshape(8, sub))
    out = np.zeros((8, sub), dtype=np.uint8)
    for q in range(8):
        if (e >> q) & 1:
            for y in range(8):
                out[y] ^= v[q + y]
    return out.reshape(nbytes)


def locate_syndromes(k, m, nbytes, syn, rows):
    """The definition on the syndromes uint8 [m, nbytes] of one stripe: (status, row)."""
    syn = np.asarray(syn, dtype=np.uint8).reshape(m, nbytes)
    if not syn.any():
        return CLEAN, NONE
    hits = []
    flat = lhverify.is_flat(k, m)
    for x in range(k):   # an error in data block x only: s_r == B(G[r][x]) s_0 for every r
        if all(np.array_equal(mul(k, m, nbytes, 1 if flat else lhupdate.coefficient(rows, r, x), syn[0]), syn[r])
               for r in range(m)):
            hits.append(x)
    bad = syn.any(axis=1)
    for r in range(m):   # an error in recovery block r only: no other row is non-zero
        if bad[r] and int(bad.sum()) == 1:
            hits.append(k + r)
    assert len(hits) <= 1 or m == 1, ("two single blocks explain one stripe", k, m, hits)
    return (ONE, hits[0]) if len(hits) == 1 else (MANY, NONE)


def model_locate(k, m, nbytes, data, rec, rows):
    """(status, row) of one stored stripe, data uint8 [k, nbytes] and rec uint8 [m, nbytes]."""
    return locate_syndromes(k, m, nbytes, lhverify.syndrome(k, m, nbytes, data, rec, rows), rows)


def definition_locate(oracle, k, m, nbytes, data, rec):
    """The contract through the C oracle alone: for every block x, rebuild it from the others
    (a data block by oracle.decode from the other data blocks and recovery row 0, the one row a
    replacement has to satisfy first; a recovery block by oracle.encode) and ask whether the stripe
    then encodes to its stored recovery blocks."""
    data = np.asarray(data, dtype=np.uint8).reshape(k, nbytes)
    rec = np.asarray(rec, dtype=np.uint8).reshape(m, nbytes)

    def encode(d):
        rc, r = oracle.encode(k, m, d, nbytes)
        assert rc == 0
        return r.reshape(m, nbytes)
    if np.array_equal(encode(data), rec):
        return CLEAN, NONE
    hits = []
    for x in range(k):
        bufs = [data[j].copy() for j in range(k)]
        bufs[x] = rec[0].copy()
        rws = list(range(k))
        rws[x] = k
        rc, _ = oracle.decode(k, m, bufs, rws, nbytes)
        assert rc == 0
        fixed = data.copy()
        fixed[x] = bufs[x]
        if np.array_equal(encode(fixed), rec):
            hits.append(x)
    same = (encode(data) == rec).all(axis=1)
    for r in range(m):
        if not same[r] and int((~same).sum()) == 1:
            hits.append(k + r)
    return (ONE, hits[0]) if len(hits) == 1 else (MANY, NONE)


def expected(oracle, k, m, nbytes, data, rec):
    """(status int8 [S], rows uint8 [S]) of stored data [S, k, B] and recovery [S, m, B]."""
    S = data.shape[0]
    rows = None if lhverify.is_flat(k, m) else oracle.cauchy_rows(k, m)
    status, out = np.zeros(S, dtype=np.int8), np.full(S, NONE, dtype=np.uint8)
    for s in range(S):
        status[s], out[s] = model_locate(k, m, nbytes, data[s], rec[s], rows)
    return status, out


# ------------------------------------------------------------------ planting
def block_of(data, rec, s, x):
    """Block x of stripe s of the stored word: data block x, or recovery block x - k."""
    k = data.shape[1]
    return data[s, x] if x < k else rec[s, x - k]


def plant_bit(data, rec, s, x, p, n=0):
    block_of(data, rec, s, x)[p] ^= np.uint8(1 << (n % 8))


def plant_byte(data, rec, s, x, p, n=0):
    block_of(data, rec, s, x)[p] ^= np.uint8(1 + (n * 37) % 255)   # never 0


def plant_block(data, rec, s, x, data0, rec0):
    """Block x replaced by the next stripe's (which differs: the data is random)."""
    S = data0.shape[0]
    new = block_of(data0, rec0, (s + 1) % S, x)
    assert not np.array_equal(new, block_of(data0, rec0, s, x))
    block_of(data, rec, s, x)[:] = new


def other_offset(k, m, nbytes, p, n=0):
    """A byte position whose offset within the sub-block span differs from p's (span >= 2)."""
    ns, span, _, _ = lhverify.geometry(k, m, nbytes)
    assert span >= 2
    o = (p % span + 1 + n % (span - 1)) % span
    assert o != p % span
    return ((p // span + n) % ns) * span + o


def meant(k, m, style, blocks):
    """The answer a plant of `style` in `blocks` (rows of the stored word) is meant to have."""
    if style == "clean":
        return CLEAN, NONE
    if m == 1 or len(blocks) > 1:
        return MANY, NONE
    return ONE, blocks[0]


def mixed_case(oracle, k, m, nbytes, stripes, seed, check=None):
    """STYLES cycle over the stripes: clean; one data bit; a data block replaced by the next
    stripe's; one recovery byte; one byte of recovery 0; two recovery rows, two data blocks, one
    data and one recovery block -- each pair at different offsets of the span, so the answer is 2
    for every m >= 2.  Positions from lhverify.positions, recovery rows from lhverify.tile_rows,
    both walked in order.  Returns read-only (data, rec, status, rows, plan), plan[s] = (style,
    corrupt blocks).  The meant answers follow from the plants by the header's argument; they are
    compared with model_locate's for the first `check` stripes (default: all -- the model costs
    about k m small numpy operations a stripe, so long batches and large codes check a prefix
    that holds every style)."""
    data0, rec0 = lhverify.encoded(oracle, k, m, nbytes, stripes, seed)
    data, rec = data0.copy(), rec0.copy()
    pos, trows = lhverify.positions(k, m, nbytes, seed), lhverify.tile_rows(m)
    status, out, plan = np.zeros(stripes, dtype=np.int8), np.full(stripes, NONE, dtype=np.uint8), []
    n = 0
    for s in range(stripes):
        style = STYLES[s % len(STYLES)]
        p, r, x = pos[n % len(pos)], trows[n % len(trows)], n % k
        p2 = other_offset(k, m, nbytes, p, n) if style in ("two-recs", "two-data", "data+rec") else None
        blocks = []
        if style == "data-bit":
            plant_bit(data, rec, s, x, p, n)
            blocks = [x]
        elif style == "data-block":
            plant_block(data, rec, s, x, data0, rec0)
            blocks = [x]
        elif style == "rec-byte":
            plant_byte(data, rec, s, k + r, p, n)
            blocks = [k + r]
        elif style == "rec0-byte":
            plant_byte(data, rec, s, k, p, n)
            blocks = [k]
        elif style == "two-recs":
            r2 = (r + 1 + n % max(m - 1, 1)) % m
            plant_byte(data, rec, s, k + r, p, n)
            blocks = [k + r]
            if r2 != r:
                plant_bit(data, rec, s, k + r2, p2, n)
                blocks.append(k + r2)
        elif style == "two-data":
            y = (x + 1 + n % max(k - 1, 1)) % k
            plant_bit(data, rec, s, x, p, n)
            blocks = [x]
            if y != x:
                plant_byte(data, rec, s, y, p2, n)
                blocks.append(y)
        elif style == "data+rec":
            plant_byte(data, rec, s, x, p, n)
            plant_bit(data, rec, s, k + r, p2, n)
            blocks = [x, k + r]
        if style != "clean":
            n += 1
        status[s], out[s] = meant(k, m, style, blocks)
        plan.append((style, blocks))
    c = stripes if check is None else min(check, stripes)
    got = expected(oracle, k, m, nbytes, data[:c], rec[:c])
    assert got[0].tolist() == status[:c].tolist() and got[1].tolist() == out[:c].tolist(), (k, m, nbytes, "plant against model")
    for a in (data, rec, status, out):
        a.setflags(write=False)
    return data, rec, status, out, plan


@functools.lru_cache(maxsize=None)
def bit_sweep(oracle, k, m, nbytes, seed):
    """One stripe per (position of lhverify.positions, block of the stored word), one bit of that
    byte of that block flipped: data blocks and recovery blocks, recovery 0 among them.  Returns
    read-only (data, rec, status, rows); the answer is the block (2 when m == 1)."""
    pos = lhverify.positions(k, m, nbytes, seed)
    S = len(pos) * (k + m)
    data0, rec0 = lhverify.encoded(oracle, k, m, nbytes, S, seed)
    data, rec = data0.copy(), rec0.copy()
    status = np.full(S, MANY if m == 1 else ONE, dtype=np.int8)
    out = np.full(S, NONE, dtype=np.uint8)
    for i, p in enumerate(pos):
        for x in range(k + m):
            s = i * (k + m) + x
            plant_bit(data, rec, s, x, p, i + x)
            if m > 1:
                out[s] = x
    for a in (data, rec, status, out):
        a.setflags(write=False)
    return data, rec, status, out


def lane_bytes(k, m, nbytes, lane):
    """The byte positions of a block that lane `lane` of lh_locate_kernel reads and no other lane
    does (sub-block 0): its own window, without the bytes the shifted last lane reads again."""
    ns, span, w, nch = lhverify.geometry(k, m, nbytes)
    assert 0 <= lane < nch
    lo, hi = lane * w, min(lane * w + w, span)
    if lane < nch - 1 and span % w and span > w:
        hi = min(hi, span - w)   # the last lane's window starts at span - w
    return list(range(lo, hi))
