"""The far-address planner (tests/lhfar.py) against fake arena addresses, on the CPU: every plan
tests/test_gpu_far.py builds -- the same functions build them here -- keeps the planner's five
properties, so a kernel's wrong 32-bit arithmetic there is a failed comparison and not a fault:

  1. some touched offset from a batch base is >= 2^31 and some >= 2^32 (layouts A, B0, B, T);
  2. both wrap images of every touched offset (mod 2^32; truncated to 32 bits and sign-extended)
     lie inside the arena;
  3. a wrap image that moved overlaps no touched block of the call, except blocks of another
     stripe, whose bytes differ (a misread is a wrong answer, a miswrite lands on the canary or on
     bytes that are compared); it never overlaps a pointer table;
  4. the payloads of different stripes differ;
  5. layout V's address = 0 (mod 2^32) lies where the layout says.

The fake addresses: one just below a multiple of 2^32, one far from any, one 2^31 past one (the
batch bases then sit on the boundary).  The library is loaded for its stripes per wave and per
workgroup (cauchy_256_batch_path, no device needed)."""
import numpy as np
import pytest

import lhfar
import lhutil
import test_gpu_far as tf
import test_gpu_stripe_counts as sc

BASES = [0x7F3F00000000 - 0x200000, 0x7F4165400000, 0x7F4280000000]
IDS = ["below-2^32-multiple", "far-from-any", "2^31-past"]


class _Lanes:
    """The package with the generic jump kernel's lane width fixed (it asks the device)."""

    def __init__(self, lh, lanes):
        self._lh, self._lanes = lh, lanes

    def __getattr__(self, name):
        return getattr(self._lh, name)

    def jump_lanes(self, k, m, nbytes, decode=False):
        return self._lanes


def _check(plan, base, far):
    bad = lhfar.problems(plan, base, far)
    assert not bad, (plan.label, bad)
    for b in plan.all():
        assert b.offs.min() >= lhfar.FRONT and b.base >= lhfar.FRONT, (plan.label, b.name)


def _cases():
    return [(d, c, layout) for d, cases in ((True, sc.DECODE), (False, sc.ENCODE)) for c in cases for layout in tf._layouts(c, d)]


@pytest.mark.parametrize("base", BASES, ids=IDS)
def test_catalogue_plans(monkeypatch, base):
    """Every (case, layout) of test_decode_far / test_encode_far."""
    import longhair_amd
    seen = set()
    for decode, case, layout in _cases():
        with monkeypatch.context() as mp:
            case = sc._resolve(longhair_amd, mp, case)
            for lanes in (1, 2) if layout == "V" else (1,):
                for plan in tf.catalogue_plans(_Lanes(longhair_amd, lanes), case, layout, decode, base):
                    _check(plan, base, far=layout != "V")
                    assert (plan.zero is not None) == (layout == "V")
                    assert bool(plan.tables) == (case.form == "table")
                    seen.add(layout)
    assert seen == {"A", "B0", "B", "B-odd", "B-out", "T", "V"}


def test_guard_strides():
    """Layouts A and B0: the largest multiple of 16 the guard admits, the smallest it refuses."""
    for spw in (0, 1, 2, 3, 5, 32, 64):
        a, b0 = lhfar.guard_strides(spw)
        w = max(1, spw)
        assert a % 16 == 0 and b0 == a + 16 and a * w < 2**31 <= b0 * w
        for stride in (a, b0):
            n = lhfar.stripes_for(stride)
            assert (n - 1) * stride >= 2**32 > (n - 2) * stride
    assert lhfar.guard_strides(1) == (2**31 - 16, 2**31) and lhfar.stripes_for(2**31) == 3
    assert lhfar.guard_strides(64) == (2**25 - 16, 2**25) and lhfar.stripes_for(2**25 - 16) == 130


@pytest.mark.parametrize("base", BASES, ids=IDS)
def test_entry_point_plans(base):
    """The buffers of test_update_far, test_verify_far, test_reconstruct_far and
    test_frame_unframe_far in every form they run, layout V with and without pointer tables."""
    seen = set()
    for what, specs, outs, forms, tile in tf.entry_points():
        for form in forms:
            S = tf.entry_stripes(form, tile)
            assert S == (max(3, tile + 1) if form.startswith("V") else 6 if form == "T" else 4)
            for plan in tf.entry_plans(specs, S, form, outs, base, 7):
                _check(plan, base, far=not form.startswith("V"))
                assert bool(plan.tables) == (form in ("T", "V-table")) and (plan.zero is not None) == form.startswith("V")
                seen.add((what, form))
                if form == "B-out":   # only the outputs are far
                    assert [b.name for b in plan.bufs.values() if b.rel().max() >= 2**32] == outs, (what, form)
    assert {(w, "V-table") for w in ("update", "verify", "reconstruct")} <= seen and ("frame", "V") in seen


@pytest.mark.parametrize("base", BASES, ids=IDS)
def test_boundary_places(base):
    """Property 5 for every place: the address = 0 (mod 2^32) lies on a 16-byte-aligned byte of a
    block, 5 bytes into an 8-byte lane, exactly between two blocks of a stripe, exactly between
    two stripes -- and a shape without such a byte has no such plan."""
    specs = [tf.spec("data", 10, 64), tf.spec("recovery", 4, 1304), tf.spec("status", 1, 1, True)]
    for subject, n, B in (("data", 10, 64), ("recovery", 4, 1304)):
        for place in lhfar.PLACES:
            plan = lhfar.boundary("V", specs, 7, base, subject, place, tables=True)
            _check(plan, base, far=False)
            s, j, x = lhfar.boundary_at(plan, base, subject)
            addr = base + plan[subject].offs[s, j] + x
            assert addr % 2**32 == 0 and s == 3
            if place == "aligned16":
                assert 0 < x < B and x % 16 == 0 and (base + plan[subject].offs[s, j]) % 16 == 0
            elif place == "lane5":
                assert x % 8 == 5 and x < B
            elif place == "between-blocks":
                assert x == 0 and j >= 1
            else:
                assert x == 0 and j == 0
            for t in plan.tables.values():
                assert t.base >= 2**32 and (base + t.base) % 8 == 0
    assert lhfar.boundary("V", [tf.spec("x", 1, 16)], 3, base, "x", "aligned16") is None        # no byte inside
    assert lhfar.boundary("V", [tf.spec("x", 1, 16)], 3, base, "x", "between-blocks") is None   # one block
    assert lhfar.boundary("V", [tf.spec("x", 5, 13)], 3, base, "x", "lane5") is not None


@pytest.mark.parametrize("base", BASES, ids=IDS)
def test_table_layout(base):
    """Layout T's own promises (lhfar.table_properties), and that `problems` sees a clash."""
    specs = [tf.spec("data", 29, 1296), tf.spec("recovery", 4, 1296), tf.spec("status", 1, 1, True)]
    plan = lhfar.table("T", specs, 6, base, 3)
    _check(plan, base, far=True)
    assert not lhfar.table_properties(plan, base)
    addr = base + plan["data"].offs
    assert ((addr[:, 1:] >> 32) != (addr[:, :-1] >> 32)).all() and (addr % 2 == 1).any()
    assert addr.max() - addr.min() > 2**32 and all(t.base >= 2**32 for t in plan.tables.values())
    # a plan whose uint32 image falls on a block of the same stripe is refused
    bad = lhfar.Buf("x", [[lhfar.FRONT, lhfar.FRONT + 2**32 + 8]], 64, lhfar.FRONT, stripe=0)
    assert any("same stripe" in p for p in lhfar.problems(lhfar.Plan("bad", [bad]), base, far=True))
    # ... and one that leaves the arena, or starts before FRONT
    for offs in ([[lhfar.FRONT - 64]], [[lhfar.ARENA_BYTES - 8]]):
        assert lhfar.problems(lhfar.Plan("bad", [lhfar.Buf("x", offs, 64, offs[0][0])]), base, far=False)
    # ... and a far layout with nothing beyond 2^32
    assert lhfar.problems(lhfar.Plan("bad", [lhfar.Buf("x", [[lhfar.FRONT], [lhfar.FRONT + 2**31]], 64, lhfar.FRONT)]), base, far=True)


def test_wrap_images():
    b = lhfar.Buf("x", [[lhfar.FRONT + r] for r in (0, 2**31 - 1, 2**31, 2**31 + 80, 2**32 - 1, 2**32, 2**32 + 160, 2**32 + 2**31 + 5)],
                  16, lhfar.FRONT)
    u, s = b.wraps()
    assert (u - lhfar.FRONT).reshape(-1).tolist() == [0, 2**31 - 1, 2**31, 2**31 + 80, 2**32 - 1, 0, 160, 2**31 + 5]
    assert (s - lhfar.FRONT).reshape(-1).tolist() == [0, 2**31 - 1, -2**31, -2**31 + 80, -1, 0, 160, -2**31 + 5]
    assert lhfar.ARENA_BYTES % 8 == 0 and lhfar.ARENA_BYTES == 2**31 + 2**32 + 2**31 + lhfar.SLACK


def test_payloads_differ():
    """Property 4: the stripes of one lhutil.fill payload, and fills of distinct seeds, differ."""
    a = lhutil.fill(11, 6 * 13).reshape(6, 13)
    assert len({r.tobytes() for r in a}) == 6
    assert len({lhutil.fill(seed, 13).tobytes() for seed in range(64)}) == 64
    with pytest.raises(AssertionError):
        tf._distinct(np.zeros((2, 3, 8), dtype=np.uint8))
