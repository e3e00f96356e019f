"""lhutil's deterministic erasure patterns (test infrastructure): placements,
exhaustive_patterns and designed_patterns, which tests/test_gpu_patterns.py and
tests/test_decode_patterns.py build their stripes from.  The GPU tests claim to cover every e,
every edge slot and row and both kinds of row-0 subset; these tests hold the generators to
that, so a GPU test never passes because its net lost a mesh.  No GPU needed."""
import math

import pytest

import lhutil
import test_gpu_patterns as tp

EXHAUSTIVE = sorted({(k, m) for k, m, kind, _ in tp.CODES if kind == "x"})
DESIGNED = sorted({(k, m) for k, m, kind, _ in tp.CODES if kind == "d"})


def test_shape_tables():
    assert EXHAUSTIVE == [(1, 4), (4, 4), (5, 5), (6, 4), (6, 6), (8, 1), (8, 2), (10, 6)]
    assert DESIGNED == [(4, 5), (8, 4), (9, 8), (9, 9), (10, 4), (20, 64), (20, 65), (29, 4), (30, 13), (40, 4),
                        (40, 12), (40, 20), (40, 33), (65, 4), (128, 128)]
    assert len({r[0] for r in tp.ROWS}) == len(tp.ROWS)
    # placements are dropped only from designed sets, and only (b) and (d)
    assert {keep for _, _, kind, keep in tp.CODES if kind == "x"} == {"abcde"}
    assert {keep for _, _, _, keep in tp.CODES} == {"abcde", "ace"}


def test_edges():
    assert lhutil.edges(1) == [0]
    assert lhutil.edges(4) == [0, 1, 2, 3]
    assert lhutil.edges(65) == [0, 1, 2, 31, 32, 62, 63, 64]
    assert lhutil.edges(200) == [0, 1, 2, 31, 32, 62, 63, 64, 65, 126, 127, 128, 129, 197, 198, 199]


def test_placements_layouts():
    k, E, R = 6, (1, 4), (0, 3)
    got = lhutil.placements(k, E, R, seed=7, labels=True)
    assert [g[0] for g in got] == list("abcde")
    by = {label: slots for label, slots, _ in got}
    d = lambda *xs: [("d", x) for x in xs]  # noqa: E731
    assert by["a"] == d(0) + [("r", 0)] + d(2, 3) + [("r", 3)] + d(5)
    assert by["b"] == d(0) + [("r", 3)] + d(2, 3) + [("r", 0)] + d(5)
    assert by["c"] == d(0, 2, 3, 5) + [("r", 0), ("r", 3)]
    assert by["d"] == [("r", 0), ("r", 3)] + d(0, 2, 3, 5)
    assert sorted(by["e"]) == sorted(by["c"]) and by["e"] not in (by["a"], by["b"], by["c"], by["d"])
    for _, slots, rows in got:
        assert rows == [x if kind == "d" else k + x for kind, x in slots]
    # the (slots, rows) form of erasure_case, and `keep`
    assert lhutil.placements(k, E, R, seed=7) == [(s, r) for _, s, r in got]
    assert [g[0] for g in lhutil.placements(k, E, R, 7, keep="ace", labels=True)] == list("ace")
    # duplicates go: nothing erased leaves the identity and its permutation; the last original
    # erased makes (a), (b) and (c) one layout
    assert [g[0] for g in lhutil.placements(8, (), (), 1, labels=True)] == ["a", "e"]
    assert [g[0] for g in lhutil.placements(4, (3,), (0,), 1, labels=True)][:2] == ["a", "d"]
    # another seed permutes otherwise
    assert lhutil.placements(29, E, R, 1)[-1] != lhutil.placements(29, E, R, 2)[-1]


@pytest.mark.parametrize("k,m", EXHAUSTIVE + [(2, 2), (3, 6), (8, 8)])
def test_exhaustive_patterns_count(k, m):
    pats = lhutil.exhaustive_patterns(k, m)
    assert len(pats) == len(set(pats)) == math.comb(k + m, k)      # Vandermonde's identity
    for E, R in pats:
        assert len(E) == len(R) <= min(k, m)
        assert list(E) == sorted(set(E)) and list(R) == sorted(set(R))
        assert all(0 <= x < k for x in E) and all(0 <= j < m for j in R)


@pytest.mark.parametrize("k,m,kind,keep", tp.CODES, ids=[f"{kind}-k{k}m{m}" for k, m, kind, _ in tp.CODES])
def test_every_stripe_is_valid_and_reproducible(k, m, kind, keep):
    cases = tp.cases_of(k, m, kind)
    assert cases == tp.cases_of(k, m, kind)                        # nothing unseeded
    assert cases == lhutil.pattern_cases(k, m, tp.patterns_of(k, m, kind), tp.seed_of(k, m), keep)
    assert len({tuple(c[4]) for c in cases}) == len({(c[0], c[1], c[2]) for c in cases}) == len(cases)
    for E, R, label, slots, rows in cases:
        assert label in keep
        assert lhutil.rows_valid(rows, k, m), (E, R, label)
        assert sorted(r - k for r in rows if r >= k) == list(R)
        assert sorted(set(range(k)) - {r for r in rows if r < k}) == list(E)


@pytest.mark.parametrize("k,m", DESIGNED)
def test_designed_patterns_cover_the_edges(k, m):
    pats = lhutil.designed_patterns(k, m)
    assert pats == lhutil.designed_patterns(k, m) and len(set(pats)) == len(pats)
    assert pats[0] == ((), ())
    e_max = min(k, m)
    assert {len(E) for E, _ in pats} == set(range(e_max + 1))      # every e occurs
    for E, R in pats:
        assert len(E) == len(R) and list(E) == sorted(set(E)) and list(R) == sorted(set(R))
        assert all(0 <= x < k for x in E) and all(0 <= j < m for j in R)
    singles = {(E[0], R[0]) for E, R in pats if len(E) == 1}
    xs, js = (range(k), range(m)) if k * m <= 1024 else (lhutil.edges(k), lhutil.edges(m))
    assert singles >= {(x, j) for x in xs for j in js}
    for e in range(1, e_max + 1):                                   # the four ladders
        for E in (tuple(range(e)), tuple(range(k - e, k))):
            for R in (tuple(range(e)), tuple(range(m - e, m))):
                assert (E, R) in pats
    assert {j for _, R in pats for j in R} >= set(lhutil.edges(m))  # every edge row is used
    with_last = [R for _, R in pats if 0 in R and m - 1 in R]
    without = [R for _, R in pats if 0 in R and m - 1 not in R]
    assert with_last and without                                    # row 0 with and without row m - 1
    assert {len(R) for R in with_last} >= set(range(2, e_max + 1))  # ... at every e >= 2
    # every edge slot holds a recovery block in some stripe and an original in another, in the
    # placements the tests keep
    keep = tp.KEEP[(k, m, "d")]
    holds = {"d": set(), "r": set()}
    for _, _, _, slots, _ in lhutil.pattern_cases(k, m, pats, tp.seed_of(k, m), keep):
        for i, (kind, _) in enumerate(slots):
            holds[kind].add(i)
    assert holds["r"] >= set(lhutil.edges(k)) and holds["d"] >= set(lhutil.edges(k))


def test_designed_strided_patterns():
    pats = lhutil.designed_patterns(40, 20)
    assert ((0, 8, 16, 24, 32), (0, 4, 8, 12, 16)) in pats          # E = floor(i k / e), R = floor(i m / e)
    assert ((0, 8, 16, 24, 32), (0, 4, 9, 14, 19)) in pats          # the rows spread to row m - 1
    # k > m: the strided originals keep going where the strided rows would repeat -- they never
    # do for e <= m; for k < m the originals stop being distinct only above e = k
    assert ((0, 1, 2, 3), (0, 1, 2, 3)) in lhutil.designed_patterns(4, 5)


def test_pattern_batch_and_digest():
    """pattern_batch lays out what the cases say; decode_all leaves its input alone."""
    import numpy as np
    orc = lhutil.Oracle()
    k, m, nbytes = 5, 3, 8
    cases = lhutil.pattern_cases(k, m, lhutil.exhaustive_patterns(k, m), 3)
    blocks, rows = lhutil.pattern_batch(orc, k, m, nbytes, cases, seed=11, pool=4)
    data = lhutil.pattern_data(k, nbytes, len(cases), 11, pool=4)
    assert data.shape == (4, k, nbytes) and not np.array_equal(data[0], data[1])
    for s in (0, 1, 5, len(cases) - 1):
        rec = orc.encode(k, m, data[s % 4], nbytes)[1].reshape(m, nbytes)
        for i, (kind, x) in enumerate(cases[s][3]):
            assert blocks[s, i].tobytes() == (data[s % 4, x] if kind == "d" else rec[x]).tobytes()
        assert rows[s].tolist() == cases[s][4]
    before = blocks.copy()
    rcs, rows_out, out = lhutil.decode_all(orc, k, m, blocks, rows, nbytes)
    assert np.array_equal(blocks, before) and (rcs == 0).all()
    for s in range(len(cases)):       # against the per-stripe call every other test uses
        bufs = [blocks[s, i].copy() for i in range(k)]
        rc, r = orc.decode(k, m, bufs, rows[s].tolist(), nbytes)
        assert rc == 0 and r == rows_out[s].tolist() and np.array_equal(np.stack(bufs), out[s])
    d = lhutil.pattern_digest(rcs, rows_out, out)
    assert d == lhutil.pattern_digest(rcs, rows_out, out) and len(d) == 16
    out[3, 2, 1] ^= 1
    assert d != lhutil.pattern_digest(rcs, rows_out, out)
