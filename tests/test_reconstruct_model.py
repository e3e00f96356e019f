"""The repair in numpy against the C oracle (no GPU): the coefficient composition of
lh_reconstruct_coef_kernel (lhreconstruct.compose, with a GF(256) inverse of its own) applied with
the kernel's B(c) arithmetic (lhreconstruct.apply over lhupdate.ladder) gives, for every survivor
set, the rows of the codeword -- the data followed by the oracle's encode of it.  This pins what
tests/test_gpu_reconstruct.py expects of the kernels; it needs no symbol of the library."""
import numpy as np
import pytest

import lhreconstruct as lr


def _check(oracle, k, m, nbytes, rows, want_rows, seed):
    cw = lr.codewords(oracle, k, m, nbytes, 1, seed)
    G = lr.generator(oracle, k, m)
    blocks, exp, status = lr.case(cw, k, m, [rows], [want_rows], 0)
    assert status.tolist() == [0]
    C = lr.compose(k, m, G, rows, want_rows)
    got = lr.apply(k, m, nbytes, blocks[0], C)
    assert np.array_equal(got, exp[0]), (k, m, nbytes, rows, want_rows)
    return C


def test_gf_arithmetic():
    assert lr.gmul(2, 0x80) == 0x87 and lr.gmul(1, 77) == 77 and lr.gmul(0, 5) == 0
    for a in (1, 2, 3, 0x53, 0x87, 0xFF):
        assert lr.gmul(a, lr.ginv(a)) == 1
    A = [[1, 1, 1], [3, 7, 9], [0x53, 2, 0xCA]]
    Ai = lr.gf_inverse(A)
    for i in range(3):
        for j in range(3):
            v = 0
            for t in range(3):
                v ^= lr.gmul(A[i][t], Ai[t][j])
            assert v == int(i == j)


def test_every_survivor_set_of_k4m2(oracle):
    """All C(6, 4) = 15 survivor sets x every wanted row (all six at once, and each alone), the
    slots ascending and reversed."""
    k, m, nbytes = 4, 2, 16
    sets = lr.survivor_sets(k, m)
    assert len(sets) == 15
    for rows in sets:
        for order in (rows, rows[::-1]):
            C = _check(oracle, k, m, nbytes, order, list(range(k + m)), 42)
            for w in range(k + m):
                assert _check(oracle, k, m, nbytes, order, [w], 42) == [C[w]]
                if w in order:   # a present row is a copy
                    assert C[w] == [int(i == order.index(w)) for i in range(k)]


NET = [
    # (survivor rows, wanted rows) of k5/m7: one erasure; min(k, m) = 5 erasures; only recovery rows wanted
    ([0, 1, 5, 3, 4], [2]),
    ([0, 1, 11, 3, 4], [2, 5, 6, 10]),
    ([11, 7, 5, 9, 6], [0, 1, 2, 3, 4]),
    ([5, 6, 7, 8, 9], [10, 11, 4, 0, 10]),
    ([0, 1, 2, 3, 4], [5, 6, 7, 8, 9, 10, 11]),
    ([4, 8, 0, 10, 2], [5, 6, 7, 9, 11]),
    ([4, 8, 0, 10, 2], [lr.NONE, 11, lr.NONE]),
]


@pytest.mark.parametrize("rows,want_rows", NET, ids=[f"net{i}" for i in range(len(NET))])
def test_designed_net_of_k5m7(oracle, rows, want_rows):
    """k < m: the generator's Cauchy closed form in the planner."""
    C = _check(oracle, 5, 7, 16, rows, want_rows, 57)
    for w, c in zip(want_rows, C):
        if w == lr.NONE:
            assert not any(c)


@pytest.mark.parametrize("k,m,nbytes", [(5, 1, 13), (1, 3, 7), (29, 4, 56)])
def test_flat_and_one_wide_shape(oracle, k, m, nbytes):
    rng = np.random.Generator(np.random.PCG64(k * 100 + m))
    for e in range(0, min(k, m) + 1):
        rows = lr.pick_rows(rng, k, m, e)
        _check(oracle, k, m, nbytes, rows, list(range(k + m)), 7 + e)


def test_case_marks_invalid_stripes(oracle):
    k, m, nbytes = 4, 2, 16
    cw = lr.codewords(oracle, k, m, nbytes, 5, 3)
    rows = [[0, 1, 2, 3], [0, 1, 1, 3], [0, 6, 2, 3], [0, 1, 2, 3], [0, 1, 2, 3]]
    want = [[4, lr.NONE], [4, 5], [4, 5], [6, 0], [lr.NONE, lr.NONE]]
    blocks, exp, status = lr.case(cw, k, m, rows, want, 0xC3)
    assert status.tolist() == [0, -1, -1, -1, 0]
    assert np.array_equal(exp[0, 0], cw[0, 4]) and (exp[0, 1] == 0xC3).all()
    assert (exp[1:] == 0xC3).all()
    assert lr.stripes_per_workgroup(4, 2, 64) == 256 and lr.stripes_per_workgroup(4, 2, 1296) == 12
    assert lr.stripes_per_workgroup(5, 1, 13) == 256 and lr.lanes_per_stripe(4, 2, 72) == 2
