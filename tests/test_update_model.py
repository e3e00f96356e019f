"""The recovery patch in numpy against the C oracle (no GPU): recovery'[r] = recovery[r] ^
B(G[r][x]) (old_x ^ new_x), with the mul2 ladder and bit masks kernels.hip documents, rows
1..m-1 of G from lho_cauchy_rows and row 0 all ones, equals the oracle's encode of the patched
data byte for byte.  This pins what tests/test_gpu_update.py expects of the kernel; it needs no
symbol of the library."""
import numpy as np
import pytest

import lhupdate
import lhutil

SHAPES = [(4, 2, 8), (29, 4, 1296), (10, 13, 24), (200, 56, 40), (3, 5, 56), (5, 1, 13), (255, 1, 8), (1, 3, 16)]


@pytest.mark.parametrize("k,m,nbytes", SHAPES, ids=[f"k{k}m{m}b{b}" for k, m, b in SHAPES])
def test_model_equals_reencode(oracle, k, m, nbytes):
    seed = k * 1000 + m * 10 + nbytes
    rng = np.random.Generator(np.random.PCG64(seed))
    rows = oracle.cauchy_rows(k, m) if m > 1 and k > 1 else None
    data = lhutil.fill(seed, k * nbytes).reshape(k, nbytes)
    rc, rec = oracle.encode(k, m, data, nbytes)
    assert rc == 0
    rec = rec.reshape(m, nbytes).copy()
    for changes, style in ((1, "plain"), (3, "plain"), (3, "dup"), (3, "hole"), (2, "none")):
        cols = lhupdate.pick_cols(rng, k, changes, style)
        old = lhutil.fill(seed + 7 * changes, changes * nbytes).reshape(changes, nbytes)
        new = lhutil.fill(seed + 7 * changes + 1, changes * nbytes).reshape(changes, nbytes)
        patched = data.copy()
        for j, c in enumerate(cols):
            if c != lhupdate.NONE:
                patched[c] ^= old[j] ^ new[j]
        rc, exp = oracle.encode(k, m, patched, nbytes)
        assert rc == 0
        got = lhupdate.model_update(k, m, nbytes, rec, cols, old ^ new, rows)
        assert got.tobytes() == exp.tobytes(), (k, m, nbytes, style, cols)
        if style == "dup":
            assert cols[-1] == cols[0]
        if style == "none":
            assert got.tobytes() == rec.tobytes()


def test_ladder_is_mul2():
    """v[q + y] is row y of B(2^q) delta: one step of the ladder is kernels.hip's mul2."""
    d = lhutil.fill(5, 8 * 16).reshape(8, 16)
    v = lhupdate.ladder(d)
    cur = [d[y] for y in range(8)]
    for q in range(8):
        assert all((cur[y] == v[q + y]).all() for y in range(8)), q
        cur = cur[1:] + [cur[0] ^ cur[1] ^ cur[2] ^ cur[7]]
