"""The recovery scrub in numpy against the C oracle (no GPU): the syndrome recovery_r ^ sum_j
B(G[r][j]) data_j (lhupdate.model_update over all k columns, from the stored recovery words) is
zero on the oracle's recovery, non-zero in exactly the row of a flipped recovery bit and in
every row after a flipped data bit.  This pins what tests/test_gpu_verify.py expects of the
kernel; it needs no symbol of the library.  Also the self-tests of lhverify's generators."""
import numpy as np
import pytest

import lhutil
import lhverify

SHAPES = [(4, 2, 8), (29, 4, 1296), (29, 4, 56), (10, 13, 24), (200, 56, 64), (5, 1, 13), (1, 3, 16), (255, 1, 8)]
IDS = [f"k{k}m{m}b{b}" for k, m, b in SHAPES]


def _bad_rows(syn):
    return np.nonzero(syn.any(axis=1))[0].tolist()


@pytest.mark.parametrize("k,m,nbytes", SHAPES, ids=IDS)
def test_syndrome_model(oracle, k, m, nbytes):
    seed = k * 1000 + m * 10 + nbytes
    rng = np.random.Generator(np.random.PCG64(seed))
    rows = oracle.cauchy_rows(k, m) if m > 1 and k > 1 else None
    data = lhutil.fill(seed, k * nbytes).reshape(k, nbytes)
    rc, rec = oracle.encode(k, m, data, nbytes)
    assert rc == 0
    rec = rec.reshape(m, nbytes).copy()
    assert not lhverify.syndrome(k, m, nbytes, data, rec, rows).any()
    # rows and positions walked together; the numpy model costs ~k m small operations a syndrome,
    # so a large code takes an even sample of the pairs
    tr, pos = lhverify.tile_rows(m), lhverify.positions(k, m, nbytes, seed)
    budget = max(4, 4000 // (k * m))
    n = min(budget, max(len(tr), len(pos)))
    pairs = [(tr[(i * len(tr) // n) % len(tr)] if len(tr) >= n else tr[i % len(tr)], pos[i * len(pos) // n % len(pos)])
             for i in range(n)]
    assert pairs[0][0] == 0 and len({r for r, _ in pairs}) >= min(2, m)
    for r, p in pairs:
        stored = rec.copy()
        stored[r, p] ^= np.uint8(1 << int(rng.integers(0, 8)))
        syn = lhverify.syndrome(k, m, nbytes, data, stored, rows)
        assert _bad_rows(syn) == [r], (r, p)
        assert int(np.count_nonzero(syn)) == 1
    for p in pos[::-(-len(pos) // max(2, budget // 2))]:
        stored = data.copy()
        stored[int(rng.integers(0, k)), p] ^= np.uint8(1 << int(rng.integers(0, 8)))
        assert _bad_rows(lhverify.syndrome(k, m, nbytes, stored, rec, rows)) == list(range(m)), p
        status, bad = lhverify.expected(oracle, k, m, nbytes, stored[None], rec[None])
        assert status.tolist() == [1] and bad.tolist() == [[1] * m]
    status, bad = lhverify.expected(oracle, k, m, nbytes, data[None], rec[None])
    assert status.tolist() == [0] and not bad.any()


GENERATOR_SHAPES = SHAPES + [(29, 4, b) for b in (8, 24, 40, 64, 136, 1304, 4104)] + [(4, 2, 16)]


@pytest.mark.parametrize("k,m,nbytes", GENERATOR_SHAPES, ids=[f"k{k}m{m}b{b}" for k, m, b in GENERATOR_SHAPES])
def test_positions_hit_every_lane_class(k, m, nbytes):
    ns, span, lane, nch = lhverify.geometry(k, m, nbytes)
    pos = lhverify.positions(k, m, nbytes, 1)
    assert pos == sorted(set(pos)) and 0 <= pos[0] and pos[-1] < nbytes
    fixed = lhverify.positions(k, m, nbytes, 1, extra=0)
    hit = set().union(*(lhverify.lane_class(k, m, nbytes, p) for p in fixed))
    want = {"first", "last"}
    want.add("piecewise" if span < lane else "whole")
    if span > lane and span % lane:
        want |= {"overlap", "tail"}
        for y in range(ns):
            assert "overlap" in lhverify.lane_class(k, m, nbytes, y * span + span - lane)
            assert lhverify.lane_class(k, m, nbytes, y * span + (nch - 1) * lane) >= {"tail"}
            assert lhverify.lane_class(k, m, nbytes, y * span + (nch - 1) * lane - 1) >= {"whole", "overlap"}
    assert hit == want, (hit, want)
    for y in range(ns):   # every sub-block gets its first and last byte
        assert y * span in fixed and y * span + span - 1 in fixed
    assert nch == -(-span // lane) and lhverify.stripes_per_workgroup(k, m, nbytes) == max(1, 256 // nch)


def test_tile_rows():
    assert lhverify.tile_rows(1) == [0]
    assert lhverify.tile_rows(4) == [0, 3]
    assert lhverify.tile_rows(13) == [0, 3, 4, 7, 8, 11, 12]
    assert lhverify.tile_rows(56)[-2:] == [52, 55] and len(lhverify.tile_rows(56)) == 28


@pytest.mark.parametrize("k,m,nbytes", [(29, 4, 56), (10, 13, 24), (5, 1, 13), (1, 3, 16)])
def test_corrupt_case_covers_its_styles(oracle, k, m, nbytes):
    data, rec, status, bad, plan = lhverify.corrupt_case(oracle, k, m, nbytes, 40, 7)
    assert {style for style, _ in plan} == set(lhverify.STYLES)
    clean = [s for s, (style, _) in enumerate(plan) if style == "clean"]
    assert clean and not status[clean].any() and status.sum() == 40 - len(clean)
    if m > 1:
        assert any(style == "two-rows" and len(meant) == 2 for style, meant in plan)
        assert any(style == "data-bit" and len(meant) == m for style, meant in plan)
    used = {r for style, meant in plan if style == "rec-byte" for r in meant}
    assert used == set(lhverify.tile_rows(m)[:len(used)]) or used <= set(lhverify.tile_rows(m))
