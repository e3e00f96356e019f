"""The locate contract in numpy against the C oracle (no GPU, no symbol of the library).

`lhlocate.model_locate` answers from the syndromes; `lhlocate.definition_locate` asks the contract's
own question of the oracle, with no syndrome arithmetic: rebuild block x from the others -- does
the stripe then encode to its stored recovery?  The two must agree on every single-block plant and
(m >= 3) on every pair of blocks.  Also pinned here: the coefficients of row 1 of the generator are
pairwise distinct over the columns and non-zero, which is what the kernel's column search rests
on, and the self-tests of lhlocate's generators.  (The kernel searches wordwise; it has no scalar
division route, so there is no change of basis to pin.)"""
import itertools

import numpy as np
import pytest

import lhlocate
import lhutil
import lhverify

SHAPES = [(2, 2, 16), (3, 2, 16), (4, 3, 16), (5, 4, 24)]
IDS = [f"k{k}m{m}b{b}" for k, m, b in SHAPES]


def _stripes(oracle, k, m, nbytes):
    data, rec = lhverify.encoded(oracle, k, m, nbytes, 2, k * 100 + m)
    return data, rec


def _both(oracle, k, m, nbytes, data, rec, rows):
    got = lhlocate.model_locate(k, m, nbytes, data, rec, rows)
    want = lhlocate.definition_locate(oracle, k, m, nbytes, data, rec)
    return got, want


@pytest.mark.parametrize("k,m,nbytes", SHAPES, ids=IDS)
def test_model_equals_definition_single_block(oracle, k, m, nbytes):
    """Every block of the stored word, corrupt in one bit, in one byte and as a whole (the next
    stripe's block in its place): the model and the definition both name it."""
    data0, rec0 = _stripes(oracle, k, m, nbytes)
    rows = oracle.cauchy_rows(k, m)
    assert _both(oracle, k, m, nbytes, data0[0], rec0[0], rows) == ((0, 0xFF), (0, 0xFF))
    n = 0
    for x in range(k + m):
        for style in ("bit", "byte", "block"):
            for p in lhverify.positions(k, m, nbytes, 5, extra=1):
                data, rec = data0.copy(), rec0.copy()
                if style == "bit":
                    lhlocate.plant_bit(data, rec, 0, x, p, n)
                elif style == "byte":
                    lhlocate.plant_byte(data, rec, 0, x, p, n)
                else:
                    lhlocate.plant_block(data, rec, 0, x, data0, rec0)
                n += 1
                got, want = _both(oracle, k, m, nbytes, data[0], rec[0], rows)
                assert got == want == (1, x), (x, style, p, got, want)
                if style == "block":
                    break


@pytest.mark.parametrize("k,m,nbytes", [s for s in SHAPES if s[1] >= 3], ids=[i for i, s in zip(IDS, SHAPES) if s[1] >= 3])
def test_model_equals_definition_pairs(oracle, k, m, nbytes):
    """Every pair of blocks corrupt, at the same byte and at different offsets of the span: two
    corrupt blocks are within the code's distance for m >= 3, so both say 2, never a row."""
    data0, rec0 = _stripes(oracle, k, m, nbytes)
    rows = oracle.cauchy_rows(k, m)
    for n, (x, y) in enumerate(itertools.combinations(range(k + m), 2)):
        p = lhverify.positions(k, m, nbytes, 9)[n % 4]
        for q in (p, lhlocate.other_offset(k, m, nbytes, p, n)):
            data, rec = data0.copy(), rec0.copy()
            lhlocate.plant_byte(data, rec, 0, x, p, n)
            lhlocate.plant_bit(data, rec, 0, y, q, n)
            got, want = _both(oracle, k, m, nbytes, data[0], rec[0], rows)
            assert got == want == (2, 0xFF), (x, y, p, q, got, want)


@pytest.mark.parametrize("k,m,nbytes", [(2, 2, 16), (3, 2, 16)], ids=IDS[:2])
def test_model_equals_definition_pairs_m2(oracle, k, m, nbytes):
    """m == 2, two corrupt blocks: beyond what the code guarantees, so the answer is whatever the
    definition gives -- the model must still give the same."""
    data0, rec0 = _stripes(oracle, k, m, nbytes)
    rows = oracle.cauchy_rows(k, m)
    seen = set()
    for n, (x, y) in enumerate(itertools.combinations(range(k + m), 2)):
        for q in (3, 4):
            data, rec = data0.copy(), rec0.copy()
            lhlocate.plant_byte(data, rec, 0, x, 3, n)
            lhlocate.plant_byte(data, rec, 0, y, q, n + 1)
            got, want = _both(oracle, k, m, nbytes, data[0], rec[0], rows)
            assert got == want, (x, y, q, got, want)
            seen.add(got[0])
    assert 2 in seen


GRID = [(k, m) for k in (1, 2, 3, 29, 128, 200, 253) for m in (2, 3, 4, 32, 55) if k + m <= 255]


def test_row_one_coefficients_are_distinct(oracle):
    """For every (k, m) of the grid: row 1 of the generator has k pairwise distinct non-zero
    entries, so B(G[1][j]) s_0 == s_1 has at most one solution j for s_0 != 0."""
    assert len(GRID) == 35 - 4 and (253, 2) in GRID and (200, 55) in GRID and (1, 55) in GRID
    for k, m in GRID:
        row1 = oracle.cauchy_rows(k, m)[0]
        assert row1.shape == (k,)
        assert (row1 != 0).all(), (k, m)
        assert len(set(row1.tolist())) == k, (k, m)


def test_mul_is_the_update_model():
    """lhlocate.mul(e, d) is what one column of lhupdate.model_update adds to a zero row."""
    import lhupdate
    k, m, nbytes = 4, 3, 24
    d = lhutil.fill(3, nbytes)
    rows = np.array([[5, 6, 7, 8], [9, 10, 11, 12]], dtype=np.uint8)
    out = lhupdate.model_update(k, m, nbytes, np.zeros((m, nbytes), dtype=np.uint8), [2], [d], rows)
    for r in range(m):
        assert np.array_equal(out[r], lhlocate.mul(k, m, nbytes, lhupdate.coefficient(rows, r, 2), d))
    assert np.array_equal(lhlocate.mul(k, m, nbytes, 1, d), d)


@pytest.mark.parametrize("k,m,nbytes", [(29, 4, 1296), (4, 2, 16), (10, 13, 24)])
def test_mixed_case_covers_its_styles(oracle, k, m, nbytes):
    data, rec, status, rows, plan = lhlocate.mixed_case(oracle, k, m, nbytes, 24, 7)
    assert {style for style, _ in plan} == set(lhlocate.STYLES)
    for s, (style, blocks) in enumerate(plan):
        if style == "clean":
            assert (status[s], rows[s]) == (0, 0xFF)
        elif len(blocks) == 1:
            assert (status[s], rows[s]) == (1, blocks[0])
        else:
            assert len(set(blocks)) == 2 and (status[s], rows[s]) == (2, 0xFF)
    assert any(style == "rec0-byte" and blocks == [k] for style, blocks in plan)
    vstatus, _ = lhverify.expected(oracle, k, m, nbytes, data, rec)
    assert (vstatus != 0).tolist() == (status != 0).tolist()   # locate's 0 is verify's 0


@pytest.mark.parametrize("k,m,nbytes", [(29, 4, 24), (5, 1, 13), (1, 3, 13)])
def test_bit_sweep_against_model(oracle, k, m, nbytes):
    data, rec, status, rows = lhlocate.bit_sweep(oracle, k, m, nbytes, 11)
    S = data.shape[0]
    assert S == len(lhverify.positions(k, m, nbytes, 11)) * (k + m)
    pick = list(range(0, S, max(1, S // 40))) + [S - 1]
    got = lhlocate.expected(oracle, k, m, nbytes, data[pick], rec[pick])
    assert got[0].tolist() == status[pick].tolist() and got[1].tolist() == rows[pick].tolist()
    if m > 1:
        assert set(rows.tolist()) == set(range(k + m))
    else:
        assert set(status.tolist()) == {2} and set(rows.tolist()) == {0xFF}


def test_lane_bytes():
    assert lhlocate.lane_bytes(5, 3, 128, 0) == list(range(0, 8)) and lhlocate.lane_bytes(5, 3, 128, 1) == list(range(8, 16))
    assert lhverify.geometry(3, 2, 16448)[3] == 257
    assert lhlocate.lane_bytes(3, 2, 16448, 256) == list(range(2048, 2056))
    assert lhlocate.lane_bytes(29, 4, 136, 1) == [8] and lhlocate.lane_bytes(29, 4, 136, 2) == [16]
