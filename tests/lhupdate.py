"""Shared helpers of the recovery-patch tests (cauchy_256_update_batch, test infrastructure).

`model_update` is the update in numpy, written from include/cauchy_256_update.h and the ladder
kernels.hip documents (tests/test_update_model.py pins it to the C oracle's re-encode);
`update_case` builds one batch with its expectation, which is always the oracle's encode of the
patched data."""
import numpy as np

import lhutil

NONE = 0xFF   # a cols entry without a change


def ladder(delta8):
    """delta8 uint8 [8, sub] -> lad[q][y] = (B(2^q) delta)_y as v[q + y]: v[0..7] = delta,
    v[8 + i] = v[i] ^ v[i + 1] ^ v[i + 2] ^ v[i + 7] (mul2's row 7: 2 * 2^7 = 0x87)."""
    v = [delta8[y] for y in range(8)]
    for i in range(7):
        v.append(v[i] ^ v[i + 1] ^ v[i + 2] ^ v[i + 7])
    return v


def coefficient(rows, r, x):
    """G[r][x]: row 0 is all ones, rows 1.. are lho_cauchy_rows (`rows`, uint8 [m - 1, k])."""
    return 1 if r == 0 else int(rows[r - 1][x])


def model_update(k, m, nbytes, rec, cols, deltas, rows):
    """recovery uint8 [m, nbytes] patched by deltas uint8 [c, nbytes] at data indices `cols`
    (0xFF skipped; the caller passes valid columns only); returns the new recovery blocks."""
    out = np.array(rec, dtype=np.uint8).reshape(m, nbytes).copy()
    for col, d in zip(cols, deltas):
        if int(col) == NONE:
            continue
        assert 0 <= int(col) < k
        if m == 1 or k == 1:
            out ^= d[None, :]
            continue
        sub = nbytes // 8
        v = ladder(np.asarray(d).reshape(8, sub))
        for r in range(m):
            e = coefficient(rows, r, int(col))
            o = out[r].reshape(8, sub)
            for q in range(8):
                if (e >> q) & 1:
                    for y in range(8):
                        o[y] ^= v[q + y]
    return out


def stripe_valid(cols, k):
    return all(int(c) == NONE or int(c) < k for c in cols)


def pick_cols(rng, k, changes, style):
    """One stripe's cols: 'plain' distinct columns where k allows, 'dup' a repeated column,
    'hole' one 0xFF entry among changes, 'none' all 0xFF."""
    if style == "none":
        return [NONE] * changes
    cols = rng.choice(k, size=changes, replace=k < changes).tolist()
    if style == "dup" and changes >= 2:
        cols[-1] = cols[0]
    if style == "hole":
        cols[int(rng.integers(0, changes))] = NONE
    return [int(c) for c in cols]


def update_case(oracle, data, rec, k, m, nbytes, changes, seed, invalid=()):
    """A batch over the stripes of (data [S, k, B], rec [S, m, B]): styles cycle plain / dup / hole
    / none over the stripes; the stripes in `invalid` get one column of k or 0xFE (alternating) and
    stay as they are.  Returns cols uint8 [S, c], old, new uint8 [S, c, B], the expected recovery
    [S, m, B] (the oracle's encode of the patched data) and the expected status int8 [S]."""
    S = data.shape[0]
    rng = np.random.Generator(np.random.PCG64(seed))
    cols = np.empty((S, changes), dtype=np.uint8)
    old = lhutil.fill(seed * 31 + 1, S * changes * nbytes).reshape(S, changes, nbytes)
    new = lhutil.fill(seed * 31 + 2, S * changes * nbytes).reshape(S, changes, nbytes)
    exp = np.array(rec, dtype=np.uint8).copy()
    status = np.zeros(S, dtype=np.int8)
    styles = ("plain", "dup", "hole", "none")
    bad = sorted(invalid)
    for s in range(S):
        cs = pick_cols(rng, k, changes, styles[s % 4])
        if s in bad:
            if all(c == NONE for c in cs):
                cs[0] = 0
            cand = [c for c in (k, 0xFE) if k <= c < NONE]   # (k = 255 has no invalid column)
            cs[int(rng.integers(0, changes))] = cand[bad.index(s) % len(cand)]
            status[s] = -1
        cols[s] = cs
        assert stripe_valid(cs, k) == (s not in bad)
        if s in bad or all(c == NONE for c in cs):
            continue
        patched = np.array(data[s], dtype=np.uint8).copy()
        for j, c in enumerate(cs):
            if c != NONE:
                patched[c] ^= old[s, j] ^ new[s, j]
        rc, r = oracle.encode(k, m, patched, nbytes)
        assert rc == 0, (k, m, nbytes, rc)
        exp[s] = r.reshape(m, nbytes)
    return cols, old, new, exp, status
