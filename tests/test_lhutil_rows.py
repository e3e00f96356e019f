"""lhutil.invalidate_rows / rows_valid (test infrastructure): the GPU tests of untouched
invalid stripes (tests/test_gpu_untouched.py) rely on the generator really producing invalid
stripes, and on erasure_case never producing one.  No GPU needed."""
import numpy as np
import pytest

import lhutil
import test_gpu_untouched as tu

SHAPES = sorted({(c[1], c[2]) for c in tu.MIXED})


def _valid_stripes(k, m, n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    for _ in range(n):
        e = int(rng.integers(0, min(k, m) + 1))
        yield e, lhutil.erasure_case(int(rng.integers(0, 2**31)), k, m, e)[1]


def test_rows_valid_is_the_headers_rule():
    assert lhutil.rows_valid([0, 1, 2, 3], 4, 2)
    assert lhutil.rows_valid([5, 1, 4, 3], 4, 2)
    assert not lhutil.rows_valid([0, 1, 1, 3], 4, 2)      # duplicate original
    assert not lhutil.rows_valid([4, 1, 4, 3], 4, 2)      # duplicate recovery row
    assert not lhutil.rows_valid([0, 1, 2, 6], 4, 2)      # row = k + m
    assert not lhutil.rows_valid([0, 1, 2, 255], 4, 2)
    assert not lhutil.rows_valid([0, 1, 2], 4, 2)         # not k rows


@pytest.mark.parametrize("k,m", SHAPES)
def test_erasure_case_is_always_valid(k, m):
    n = 0
    for e, rows in _valid_stripes(k, m, 200, k * 300 + m):
        assert lhutil.rows_valid(rows, k, m), (e, rows)
        assert sum(r >= k for r in rows) == e
        n += 1
    assert n == 200


@pytest.mark.parametrize("k,m", SHAPES)
def test_invalidate_rows_every_kind_and_position(k, m):
    kinds = lhutil.invalid_kinds(k, m)
    assert kinds == list(lhutil.INVALID_KINDS)  # every shape of the table takes every kind
    assert sorted(set(lhutil.invalid_pairs(k, m))) == sorted((a, b) for a in kinds for b in lhutil.INVALID_WHERE)
    rng = np.random.Generator(np.random.PCG64(k + m))
    e_max = min(k, m)
    # e = 0 (no recovery row: 'dup-rec' puts row k in two slots), e_max (k <= m: no original, so
    # 'dup-orig' acts as 'dup-rec'), and random e
    stripes = [lhutil.erasure_case(1, k, m, 0)[1], lhutil.erasure_case(2, k, m, e_max)[1],
               lhutil.erasure_case(3, k, m, 1)[1]] + [r for _, r in _valid_stripes(k, m, 20, k * m)]
    slot = {"first": 0, "last": k - 1, "wave": 63 if k > 63 else k - 1, "wave+1": 64 if k > 64 else 0}
    for rows in stripes:
        for kind in kinds:
            for where in lhutil.INVALID_WHERE:
                before = list(rows)
                out = lhutil.invalidate_rows(rows, k, m, kind, where, rng)
                assert rows == before                       # a copy: the input is not changed
                assert not lhutil.rows_valid(out, k, m), (rows, kind, where)
                diff = [i for i in range(k) if out[i] != rows[i]]
                two_k = kind.startswith("dup") and out.count(k) == 2
                assert len(diff) == 1 or (two_k and 1 <= len(diff) <= 2), (rows, out, kind, where)
                if where in slot and not (two_k and len(diff) == 1 and rows[slot[where]] == k):
                    assert slot[where] in diff, (rows, out, kind, where)
                if kind == "range":
                    assert out[diff[0]] == k + m
                if kind == "range255":
                    assert out[diff[0]] == 255
                if kind.startswith("dup"):
                    assert len(set(out)) < k and max(out) < k + m
                if kind == "dup-orig" and len(diff) == 1 and any(rows[i] < k for i in range(k) if i != diff[0]):
                    assert out[diff[0]] < k
                if kind == "dup-rec" and not two_k:
                    assert out[diff[0]] >= k


def test_invalidate_rows_refuses_what_does_not_apply():
    rng = np.random.Generator(np.random.PCG64(0))
    rows = lhutil.erasure_case(5, 200, 56, 10)[1]          # k + m = 256: no row is out of range
    for kind in ("range", "range255"):
        with pytest.raises(ValueError):
            lhutil.invalidate_rows(rows, 200, 56, kind, "first", rng)
    assert lhutil.invalid_kinds(200, 56) == ["dup-orig", "dup-rec"]
    with pytest.raises(ValueError):
        lhutil.invalidate_rows([0], 1, 3, "dup-orig", "first", rng)   # k = 1: nothing to repeat
    with pytest.raises(ValueError):
        lhutil.invalidate_rows(rows, 200, 56, "swap", "first", rng)
    with pytest.raises(ValueError):
        lhutil.invalidate_rows(rows, 200, 56, "dup-rec", "middle", rng)
    with pytest.raises(ValueError):
        lhutil.invalidate_rows([0, 0, 2], 3, 2, "dup-rec", "first", rng)  # input already invalid


def test_mixed_batch_layout_of_invalid_stripes():
    """pick_invalid: stripe 0, the last stripe, an adjacent interior pair, about a quarter."""
    for _, k, m, nbytes, stripes, _, _ in tu.MIXED:
        for seed in (1, 2, k * 1000 + m * 10 + nbytes):
            bad = tu.pick_invalid(stripes, seed)
            assert bad[0] == 0 and bad[-1] == stripes - 1 and len(set(bad)) == len(bad)
            assert any(a + 1 == b and 0 < a and b < stripes - 1 for a, b in zip(bad, bad[1:]))
            assert len(bad) == max(4, (stripes + 2) // 4) and len(bad) < stripes


def test_guard_check_sees_every_stray_byte():
    """Guarded.check (on a host tensor here): intact after the payloads are rewritten, and an
    assertion for one changed byte in the front guard, the offset head, a stripe's pad, the
    last stripe's pad and the back guard."""
    payload = lhutil.fill(3, 4 * 40).reshape(4, 40)
    off, pad = 3, 5
    g = tu.Guarded(payload, off, pad, tu.C_BLOCKS, device="cpu")
    assert np.array_equal(g.check("clean"), payload)
    g.view().copy_(g.view() ^ 0xFF)                      # what a decode may write: the payloads
    assert np.array_equal(g.check("payloads rewritten"), payload ^ 0xFF)
    end = tu.GUARD + off + 4 * 45
    assert g.buf.numel() == end + tu.GUARD
    for at in (0, tu.GUARD - 1, tu.GUARD, tu.GUARD + off - 1, tu.GUARD + off + 40, tu.GUARD + off + 44,
               end - 5, end - 1, end, end + tu.GUARD - 1):
        g.buf[at] ^= 1
        with pytest.raises(AssertionError):
            g.check(at)
        g.buf[at] ^= 1
    g.check("restored")
