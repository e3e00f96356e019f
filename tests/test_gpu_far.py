"""Batch offsets past 2^31 and 2^32 bytes through every kernel chain and entry point.

Every batch entry point takes 64-bit strides or per-block pointers; the register-network kernels
read a wave's stripes through one 32-bit buffer range and are kept off strides that would not
fit by codec.cpp route().  The cases here are sparse: a few stripes at a huge stride, or blocks
scattered over the whole allocation, inside one arena of about 8 GiB filled with a canary byte
(tests/lhfar.py; its planner's properties are proved in tests/test_lhfar.py).  The batch base
always lies 2^31 bytes into the arena, so an offset truncated to 32 bits, as unsigned or as signed,
still lands inside it: on the canary, or on a block of another stripe with other bytes.

Layouts (lhfar.far / table / boundary):
  A   the largest stride the range guard admits (stride * stripes per wave < 2^31, the figure from
      the library: cauchy_256_batch_path what = 12 / 13), ceil(2^32 / stride) + 1 stripes: the
      specialised kernel ran, its range at the maximum, its last wave's base beyond 2^32;
  B0  the first stride the guard refuses: the bytes are still the oracle's and no strided
      register-network kernel is in the trace (B0_DECODE / B0_ENCODE hold what route() yields;
      LONGHAIR_AMD_JIT_COMPILE=0 so that the refused shape does not compile the windowed module
      route() would offer it next -- no case here compiles a module);
  B   stripes at stride 2^31 + 80 (offsets 0, 2^31 + 80, 2^32 + 160, and a fourth stripe so that
      the stripes at those two far offsets can all be ones with work to do), again at the odd
      stride 2^31 + 3, and once with only the output argument far;
  T   pointer tables whose neighbouring entries differ in the high word of the address, with
      entries more than 2^32 apart and odd addresses, the tables themselves beyond 2^32;
  V   dense batches of one workgroup tile plus one stripe, placed so that an address = 0 (mod
      2^32) falls on a 16-byte-aligned byte of a block, 5 bytes into an 8-byte lane, exactly
      between two blocks and exactly between two stripes, for each block buffer of the call.

The kernel catalogue is test_gpu_stripe_counts.DECODE / ENCODE (shapes, env, traces, form); the
register-network cases take A, B0 and V, the other strided cases B and V, the table cases T and
V.  Then update, verify, reconstruct (B, T, and V in the strided and the table form, V over one
workgroup tile of the entry point's kernel plus one stripe), frame / unframe and the Python
wrappers.  Every run asserts
the bytes of every buffer against the C oracle's (read-only inputs: what went in), status and
rows, the launch trace, and that every other byte of the arena still holds the canary.
`-m gpu`: needs an MI355X with 9 GiB free; every module is compiled at build time."""
import collections
import ctypes

import numpy as np
import pytest

import lhfar
import lhreconstruct
import lhupdate
import lhutil
import lhverify
import test_gpu_reconstruct as tr
import test_gpu_stripe_counts as sc
import test_gpu_update as tg
import test_gpu_untouched as tu
from lhfar import spec
from test_gpu_boundaries import JUMP, JUMP2, PS4_JUMP, PS4_JUMP2, PS8_JUMP
from test_gpu_untouched import C_ROWS, C_STATUS

pytestmark = pytest.mark.gpu

vp, ll = ctypes.c_void_p, ctypes.c_longlong

# What route() yields at the first refused stride (layout B0), per catalogue case: the planner
# of the shape's e_max and the in-place jump apply (two-dword lanes from sub = 512 with at most
# four outputs), the flat jump apply for the encode (two-dword lanes: m <= 4).
B0_DECODE = {
    "fused-1lane": PS4_JUMP, "fused-k29": PS4_JUMP, "fused-64lane": PS4_JUMP2, "fused-family": PS4_JUMP,
    "fused-family-k4": PS4_JUMP, "small4-planner": PS4_JUMP, "small4-k65": PS4_JUMP, "small8-planner": PS8_JUMP,
    "two-waves-per-stripe": PS4_JUMP2,
}
B0_ENCODE = {"jit-1lane": JUMP2, "jit-lds-k29": JUMP2, "jit-k8m3": JUMP2, "jit-family": JUMP2}
NO_COMPILE = {"LONGHAIR_AMD_JIT_COMPILE": "0"}
# Layout B: offsets 0, 2^31 + 80, 2^32 + 160 and one stripe more at 3 * 2^31 + 240, so that the two
# far offsets the layout is about can both hold stripes with work to do (a decode's invalid
# stripe, an update's unchanged one sit at the ends)
FAR_STRIPES = 4


@pytest.fixture(scope="module")
def lh():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    import longhair_amd
    assert longhair_amd.cauchy_256_init() == 0
    return longhair_amd


@pytest.fixture(scope="module")
def arena(lh):
    a = lhfar.Arena()   # (an allocation failure is the test's failure, with the allocator's message)
    yield a
    a.free()


def _stream():
    import torch
    return vp(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------ one run
Job = collections.namedtuple("Job", "specs stripes payload call")
# specs: lhfar.spec per buffer; payload: {name: (before, after)} uint8 [S, n, B]; call(A) -> rc,
# with A.p(name) the buffer's pointer (its table's, in a table plan) and A.s(name) its stride


class Args:
    def __init__(self, arena, plan):
        self.arena, self.plan = arena, plan

    def p(self, name):
        t = self.plan.tables.get(name + " table")
        return vp(self.arena.ptr(t if t is not None else self.plan[name]))

    def s(self, name):
        return ll(self.plan[name].stride)

    def view(self, name):
        """The buffer as a strided view of the arena [S, n, B] (the Python wrappers' argument)."""
        b = self.plan[name]
        S, n = b.offs.shape
        return self.arena.t[b.base:].as_strided((S, n, b.nbytes), (b.stride, b.nbytes, 1))


def run(lh, arena, plan, job, trace, what):
    """Places the job's buffers by the plan, calls, and asserts the bytes, the trace and the
    canary; see the module docstring."""
    import torch
    assert plan is not None
    bad = lhfar.problems(plan, arena.base, far=plan.zero is None)
    assert not bad, (what, plan.label, bad)
    for name, (before, after) in job.payload.items():
        assert before.shape == after.shape == plan[name].shape, (name, before.shape, plan[name].shape)
    tables = {}
    try:
        for name, (before, after) in job.payload.items():
            arena.put(plan[name], before)
        for t in plan.tables.values():
            ptrs = np.ascontiguousarray(arena.base + plan[t.name[:-len(" table")]].offs).view(np.uint8)
            tables[t.name] = ptrs.reshape(t.shape)
            arena.put(t, tables[t.name])
        torch.cuda.synchronize()
        rc = job.call(Args(arena, plan))
        got_trace = lh.last_launch()
    finally:   # (whatever happened, the arena is clean for the next case)
        got, dirty = arena.sweep(plan)
    assert rc in (0, None), (what, plan.label, rc, lh.lib().cauchy_256_last_error())
    errors = []
    for name, (before, after) in {**job.payload, **{n: (t, t) for n, t in tables.items()}}.items():
        exp = torch.from_numpy(np.array(after)).cuda()
        if torch.equal(got[name], exp):
            continue
        g = got[name].cpu().numpy()
        s, j, x = (int(v[0]) for v in np.nonzero(g != after))
        same = "read-only, written" if np.array_equal(before, after) else ("still what it was before the call"
                                                                            if np.array_equal(g[s, j], before[s, j]) else "wrong")
        errors.append(f"{name}: stripe {s} block {j} byte {x} {same}: got {int(g[s, j, x]):#04x}, expected "
                      f"{int(after[s, j, x]):#04x}; {int((g != after).any(axis=2).sum())} of {g.shape[0] * g.shape[1]} blocks differ "
                      f"(arena offset {int({**plan.bufs, **plan.tables}[name].offs[s, j])})")
    if got_trace != trace:
        errors.append(f"launch trace {got_trace}, expected {trace}")
    if dirty:
        errors.append(dirty)
    if errors:
        pytest.fail(f"{what} [{plan.label}]: " + "; ".join(errors), pytrace=False)


def _distinct(a):
    """Planner property 4 for the bytes actually used: no two stripes hold the same payload."""
    assert len({a[s].tobytes() for s in range(a.shape[0])}) == a.shape[0], "two stripes hold the same bytes"


# ------------------------------------------------------------------ the catalogue's jobs
def _select(rows, invalid, k, N, far):
    """N stripes of a prepared pool of at least N + 8.  A stripe at a far offset shows a wrong
    address only if the decode has work there, so `far` (layouts A, B0, B) puts stripes with
    erasures ("good": valid, a recovery row among their rows) at the far end: below 8 stripes
    one invalid stripe first, then good ones, the pool's first valid stripe (at e_max) leading;
    from 8 on the pool's order, its last three stripes exchanged for good ones where they are
    not.  Otherwise (T, V): below 8 stripes good and invalid ones by turns, else the pool's order."""
    good = np.nonzero(~invalid & (rows >= k).any(axis=1))[0].tolist()
    inv = np.nonzero(invalid)[0].tolist()
    if N >= 8:
        sel = list(range(N))
        spare = [g for g in good if g >= N] + [g for g in good if g < N - 3][::-1]
        for pos in range(N - 3, N) if far else ():
            if sel[pos] not in good:
                g = spare.pop(0)
                if g < N:
                    sel[g] = sel[pos]
                sel[pos] = g
        return np.array(sel)
    if far:
        out = inv[:1] + good
    else:
        out = [s[i] for i in range(N) for s in (good, inv) if i < len(s)]
    assert len(out) >= N, ("too few stripes with erasures in the pool", len(good), len(inv), N)
    return np.array(out[:N])


def decode_job(oracle, case, N, far=False):
    k, m, B = case.k, case.m, case.nbytes
    pool = tu.mixed_case(oracle, k, m, B, max(N + 8, 24), sc._seed(case), case.mode)
    sel = _select(pool[1], pool[2], k, N, far)
    assert len(set(sel.tolist())) == N
    blocks, rows, invalid, exp_blocks, exp_rows = (a[sel] for a in pool)
    if pool[2].any():
        assert invalid.any() and not invalid.all()
    if far:   # the stripes beyond 2^31 and 2^32 have work to do
        assert ((rows >= k).any(axis=1) & ~invalid)[-2:].all(), (case.id, "far stripes without erasures")
    _distinct(exp_blocks)
    specs = decode_specs(k, m, B)
    payload = {"blocks": (blocks, exp_blocks), "rows": (rows.reshape(N, 1, k), exp_rows.reshape(N, 1, k)),
               "status": (np.full((N, 1, 1), C_STATUS, dtype=np.uint8), np.where(invalid, 0xFF, 0).astype(np.uint8).reshape(N, 1, 1))}

    def call(A):
        import longhair_amd
        lib = longhair_amd.lib()
        if case.form == "table":
            return lib.cauchy_256_decode_batch_ptrs(k, m, B, N, A.p("blocks"), A.p("rows"), A.p("status"), _stream())
        return lib.cauchy_256_decode_batch(k, m, B, N, A.p("blocks"), A.s("blocks"), A.p("rows"), A.p("status"), _stream())
    return Job(specs, N, payload, call)


def encode_job(oracle, case, N):
    k, m, B = case.k, case.m, case.nbytes
    data, rec = tu._encoded(oracle, k, m, B, N, sc._seed(case))
    _distinct(data)
    _distinct(rec)
    specs = encode_specs(k, m, B)
    payload = {"data": (data, data), "recovery": (np.full((N, m, B), C_ROWS, dtype=np.uint8), rec)}

    def call(A):
        import longhair_amd
        lib = longhair_amd.lib()
        if case.form == "table":
            return lib.cauchy_256_encode_batch_ptrs(k, m, B, N, A.p("data"), A.p("recovery"), _stream())
        return lib.cauchy_256_encode_batch(k, m, B, N, A.p("data"), A.s("data"), A.p("recovery"), A.s("recovery"), _stream())
    return Job(specs, N, payload, call)


def _is_register(case):
    return case.form == "strided" and (case.id.startswith(("fused-", "small4-", "small8-", "jit-")) or case.id == "two-waves-per-stripe")


def _layouts(case, decode):
    if case.form == "table":
        return ["T", "V"]
    if _is_register(case):
        return ["A", "B0", "V"]
    return ["B", "B-odd", "V"] if decode else ["B", "B-odd", "B-out", "V"]


def decode_specs(k, m, B):
    return [spec("blocks", k, B), spec("rows", 1, k, True), spec("status", 1, 1, True)]


def encode_specs(k, m, B):
    return [spec("data", k, B), spec("recovery", m, B)]


def boundary_plans(specs, S, base, tables=False):
    """Layout V for every block buffer of a call and every place its shape has."""
    out = []
    for name, n, nbytes, side in specs:
        for place in () if side else lhfar.PLACES:
            plan = lhfar.boundary(f"V {name} {place}", specs, S, base, name, place, tables)
            if plan is None:
                continue
            s, j, x = lhfar.boundary_at(plan, base, name)
            assert s == S // 2 and j * nbytes + x == lhfar.block_points(n, nbytes)[place], (plan.label, s, j, x)
            out.append(plan)
    assert len(out) >= 2, (specs, "boundary placements", len(out))
    return out


def catalogue_plans(lh, case, layout, decode, base):
    """The plans of one catalogue case (resolved, its env set) in one layout, arena at `base`."""
    k, m, B = case.k, case.m, case.nbytes
    specs = (decode_specs if decode else encode_specs)(k, m, B)
    if layout in ("A", "B0"):
        spw = lh.stripes_per_wave(k, m, B, decode)
        assert lh.stripes_per_workgroup(k, m, B, decode) >= 1, (case.id, "no specialised configuration")
        stride = lhfar.guard_strides(spw)[layout == "B0"]
        N = lhfar.stripes_for(stride)
        plan = lhfar.far(f"{layout} stride {stride} x {N}, {spw} stripes per wave", specs, N, stride)
        assert (stride * max(1, spw) < (1 << 31)) == (layout == "A")
        assert plan["blocks" if decode else "data"].rel()[-1, 0] >= (1 << 32), "the last stripe starts beyond 2^32"
        return [plan]
    if layout in ("B", "B-odd", "B-out"):
        stride = lhfar.FAR_ODD if layout == "B-odd" else lhfar.FAR
        return [lhfar.far(f"{layout} stride {stride}", specs, FAR_STRIPES, stride, {"recovery"} if layout == "B-out" else None)]
    if layout == "T":
        plan = lhfar.table("T", specs, 6, base, sc._seed(case))
        assert not lhfar.table_properties(plan, base), (case.id, lhfar.table_properties(plan, base))
        return [plan]
    return boundary_plans(specs, case.tile(lh, k, m, B) + 1, base, case.form == "table")


def entry_plans(specs, S, form, out_names, base, seed):
    """The plans of another entry point: layout B (all far / odd / only `out_names` far), T or V."""
    if form == "T":
        plan = lhfar.table("T", specs, S, base, seed)
        assert not lhfar.table_properties(plan, base), (specs, lhfar.table_properties(plan, base))
        return [plan]
    if form in ("V", "V-table"):
        return boundary_plans(specs, S, base, tables=form == "V-table")
    stride = lhfar.FAR_ODD if form == "B-odd" else lhfar.FAR
    return [lhfar.far(f"{form} stride {stride}", specs, S, stride, set(out_names) if form == "B-out" else None)]


def entry_stripes(form, tile):
    """Layout V: one workgroup tile of the entry point's kernel plus one stripe (at least the
    three stripes the cases give a role); T: 6; B: FAR_STRIPES."""
    return max(3, tile + 1) if form.startswith("V") else 6 if form == "T" else FAR_STRIPES


def update_specs(k, m, B, delta, changes=2):
    return [spec("old", changes, B)] + ([] if delta else [spec("new", changes, B)]) + [
        spec("recovery", m, B), spec("cols", 1, changes, True), spec("status", 1, 1, True)]


def verify_specs(k, m, B):
    return [spec("data", k, B), spec("recovery", m, B), spec("status", 1, 1, True), spec("bad_rows", 1, m, True)]


def reconstruct_specs(k, m, B, want=5):
    return [spec("blocks", k, B), spec("out", want, B), spec("rows", 1, k, True), spec("want_rows", 1, want, True),
            spec("status", 1, 1, True)]


def frame_specs(k, m, B):
    return [spec("data", k, B), spec("recovery", m, B), spec("packets", k + m, B + 1)]


def unframe_specs(k, B):
    return [spec("packets", k, B + 1), spec("blocks", k, B), spec("rows", 1, k, True)]


def frame_tile(packets, B):
    """kernels.hip launch_frame: one thread per 4 bytes of a packet's block, 256 per workgroup."""
    return max(1, 256 // (packets * -(-B // 4)))


def entry_points():
    """(name, specs, the output buffers, forms, the kernel's workgroup tile) of every case of
    test_update_far, test_verify_far, test_reconstruct_far and test_frame_unframe_far
    (tests/test_lhfar.py proves the planner's properties for each)."""
    out = [("update", update_specs(k, m, B, delta), ["recovery"], FORMS, tg._t_update(None, k, m, B))
           for k, m, B in UPDATE for delta in (False, True)]
    out += [("verify", verify_specs(k, m, B), ["recovery"], FORMS, lhverify.stripes_per_workgroup(k, m, B)) for k, m, B in VERIFY]
    out += [("reconstruct", reconstruct_specs(k, m, B), ["out"], FORMS, lhreconstruct.stripes_per_workgroup(k, m, B))
            for k, m, B in RECONSTRUCT]
    k, m, B = FRAME
    return out + [("frame", frame_specs(k, m, B), ["packets"], FRAME_FORMS, frame_tile(k + m, B)),
                  ("unframe", unframe_specs(k, B), ["blocks"], FRAME_FORMS, frame_tile(k, B))]


def catalogue(lh, oracle, monkeypatch, arena, case, layout, decode):
    case = sc._resolve(lh, monkeypatch, case)
    k, m, B = case.k, case.m, case.nbytes
    what = f"{'decode' if decode else 'encode'} {case.id} k {k} m {m} {B} B"
    trace = case.trace
    if layout == "B0":
        tu._set_env(monkeypatch, NO_COMPILE)
        fixed = (B0_DECODE if decode else B0_ENCODE).get(case.id)
        trace = fixed or (JUMP2 if lh.jump_lanes(k, m, B) == 2 else JUMP)   # (the two shapes taken from JIT_SAMPLE)
        assert not any(t.startswith("lh_jit_") for t in trace)
    for plan in catalogue_plans(lh, case, layout, decode, arena.base):
        N = plan["blocks" if decode else "data"].offs.shape[0]
        job = decode_job(oracle, case, N, far=layout in ("A", "B0", "B", "B-odd")) if decode else encode_job(oracle, case, N)
        run(lh, arena, plan, job, trace, what)


def _params(cases, decode):
    return [pytest.param(c, layout, id=f"{c.id}-{layout}") for c in cases for layout in _layouts(c, decode)]


@pytest.mark.parametrize("case,layout", _params(sc.DECODE, True))
def test_decode_far(lh, oracle, monkeypatch, arena, case, layout):
    """cauchy_256_decode_batch / _ptrs, every chain of the catalogue, on a mixed batch of valid and
    invalid stripes (test_gpu_untouched.mixed_case): blocks, rows and status against the oracle's,
    invalid stripes as they were."""
    catalogue(lh, oracle, monkeypatch, arena, case, layout, True)


@pytest.mark.parametrize("case,layout", _params(sc.ENCODE, False))
def test_encode_far(lh, oracle, monkeypatch, arena, case, layout):
    """cauchy_256_encode_batch / _ptrs, every chain of the catalogue: the recovery blocks the
    oracle's, the data as it was."""
    catalogue(lh, oracle, monkeypatch, arena, case, layout, False)


# ------------------------------------------------------------------ the other entry points
FORMS = ("B", "B-odd", "B-out", "T", "V", "V-table")   # (V-table: layout V through the pointer-table form)
FRAME_FORMS = ("B", "B-odd", "B-out", "V")
FRAME = (10, 4, 64)


def entry_point(lh, arena, job, form, out_names, trace, trace_table, what, seed):
    for plan in entry_plans(job.specs, job.stripes, form, out_names, arena.base, seed):
        run(lh, arena, plan, job, trace_table if plan.tables else trace, what)


UPDATE = [(29, 4, 64), (29, 4, 1304), (5, 1, 13), (1, 3, 16)]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("delta", [False, True], ids=["plain", "delta"])
@pytest.mark.parametrize("k,m,B", UPDATE, ids=[f"k{k}m{m}b{b}" for k, m, b in UPDATE])
def test_update_far(lh, oracle, arena, k, m, B, delta, form):
    """cauchy_256_update_batch / _ptrs, two changed blocks per stripe, with a stripe of no change
    (style 'none', the first) and an invalid one (the last): recovery against the oracle's encode of the patched data
    (lhupdate.update_case), old and new as they were."""
    S, changes, seed = entry_stripes(form, tg._t_update(None, k, m, B)), 2, k * 1000 + m * 10 + B
    data, rec = lhverify.encoded(oracle, k, m, B, S + 2, seed)
    cols, old, new, exp, status = lhupdate.update_case(oracle, data, rec, k, m, B, changes, seed, invalid=(1,) if k < 255 else ())
    # pool stripes: 0 plain, 1 invalid, 2 hole, 3 no change, 4 plain, 5 dup, ...  The unchanged and
    # the invalid stripe at the ends, so that the stripes beyond 2^31 and 2^32 of layout B are patched
    sel = np.array([3] + [s for s in range(S + 2) if s not in (1, 3)][:S - 2] + [1])
    assert status[1] == -1 and (cols[3] == lhupdate.NONE).all() and (exp[[0, 2]] != np.array(rec)[[0, 2]]).any(axis=(1, 2)).all()
    cols, old, new, exp, status, rec = cols[sel], old[sel], new[sel], exp[sel], status[sel], np.array(rec)[sel]
    first = old ^ new if delta else old
    _distinct(first)
    _distinct(exp)
    specs = update_specs(k, m, B, delta, changes)
    payload = {"old": (first, first), "recovery": (rec, exp), "cols": (cols.reshape(S, 1, changes),) * 2,
               "status": (np.full((S, 1, 1), C_STATUS, dtype=np.uint8), status.view(np.uint8).reshape(S, 1, 1))}
    if not delta:
        payload["new"] = (new, new)

    def call(A):
        lib = lh.lib()
        if "old table" in A.plan.tables:
            return lib.cauchy_256_update_batch_ptrs(k, m, B, S, changes, A.p("cols"), A.p("old"), None if delta else A.p("new"),
                                                    A.p("recovery"), A.p("status"), _stream())
        return lib.cauchy_256_update_batch(k, m, B, S, changes, A.p("cols"), A.p("old"), A.s("old"),
                                           None if delta else A.p("new"), ll(0) if delta else A.s("new"), A.p("recovery"),
                                           A.s("recovery"), A.p("status"), _stream())
    entry_point(lh, arena, Job(specs, S, payload, call), form, ["recovery"], ["lh_update_kernel"],
                ["lh_update_kernel(pointer table)"], f"update k {k} m {m} {B} B {'delta' if delta else 'plain'}", seed)


VERIFY = [(29, 4, 64), (29, 4, 1304), (200, 56, 64), (5, 1, 13), (1, 3, 16)]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("k,m,B", VERIFY, ids=[f"k{k}m{m}b{b}" for k, m, b in VERIFY])
def test_verify_far(lh, oracle, arena, k, m, B, form):
    """cauchy_256_verify_batch / _ptrs: a stripe with a flipped data bit, a clean one, one with a
    flipped recovery bit in the last row, and clean ones; status and bad_rows, which live in the arena too,
    against lhverify.expected; data and recovery as they were."""
    S, seed = entry_stripes(form, lhverify.stripes_per_workgroup(k, m, B)), k * 1000 + m * 10 + B + 1
    data, rec = (np.array(a) for a in lhverify.encoded(oracle, k, m, B, S, seed))
    # (the clean stripes at layout B's far offsets 2^31 + 80 and 3 * 2^31 + 240, the one bad row at
    # 2^32 + 160: a stripe read from elsewhere is neither clean nor bad in its last row only)
    data[0, k // 2, B // 2] ^= 0x01
    rec[2, m - 1, B - 1] ^= 0x10
    status, bad = lhverify.expected(oracle, k, m, B, data, rec)
    assert status.tolist() == [1, 0, 1] + [0] * (S - 3) and bad[2].tolist() == [0] * (m - 1) + [1]
    _distinct(data)
    _distinct(rec)
    specs = verify_specs(k, m, B)
    payload = {"data": (data, data), "recovery": (rec, rec),
               "status": (np.full((S, 1, 1), C_STATUS, dtype=np.uint8), status.view(np.uint8).reshape(S, 1, 1)),
               "bad_rows": (np.full((S, 1, m), C_STATUS, dtype=np.uint8), bad.reshape(S, 1, m))}

    def call(A):
        lib = lh.lib()
        if "data table" in A.plan.tables:
            return lib.cauchy_256_verify_batch_ptrs(k, m, B, S, A.p("data"), A.p("recovery"), A.p("status"), A.p("bad_rows"), _stream())
        return lib.cauchy_256_verify_batch(k, m, B, S, A.p("data"), A.s("data"), A.p("recovery"), A.s("recovery"),
                                           A.p("status"), A.p("bad_rows"), _stream())
    # (verify writes no block: "only the output far" is its recovery argument, the second input)
    entry_point(lh, arena, Job(specs, S, payload, call), form, ["recovery"], ["lh_verify_kernel"],
                ["lh_verify_kernel(pointer table)"], f"verify k {k} m {m} {B} B", seed)


RECONSTRUCT = [(4, 2, 72), (29, 4, 1296), (20, 12, 64), (5, 1, 13)]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("k,m,B", RECONSTRUCT, ids=[f"k{k}m{m}b{b}" for k, m, b in RECONSTRUCT])
def test_reconstruct_far(lh, oracle, arena, k, m, B, form):
    """cauchy_256_reconstruct_batch / _ptrs, want = 5 with one 0xFF entry in the second stripe, the
    last stripe invalid: out against lhreconstruct.case (the canary where nothing is written), blocks,
    rows and want_rows as they were."""
    S, want, seed = entry_stripes(form, lhreconstruct.stripes_per_workgroup(k, m, B)), 5, k * 1000 + m * 10 + B + 2
    cw = lhreconstruct.codewords(oracle, k, m, B, S, seed)
    rows, wr = lhreconstruct.random_batch(k, m, S, want, seed)
    wr[1, 2] = lhreconstruct.NONE
    rows[S - 1, 0] = rows[S - 1, k - 1] if k > 1 else k + m      # invalid: a duplicate survivor (k = 1: out of range)
    blocks, exp, status = lhreconstruct.case(cw, k, m, rows, wr, lhfar.CANARY)
    assert status.tolist() == [0] * (S - 1) + [-1] and (exp[:S - 1] != lhfar.CANARY).any(axis=(1, 2)).all()
    _distinct(blocks)
    _distinct(exp[:S - 1])
    specs = reconstruct_specs(k, m, B, want)
    payload = {"blocks": (blocks, blocks), "out": (np.full((S, want, B), lhfar.CANARY, dtype=np.uint8), exp),
               "rows": (rows.reshape(S, 1, k),) * 2, "want_rows": (wr.reshape(S, 1, want),) * 2,
               "status": (np.full((S, 1, 1), C_STATUS, dtype=np.uint8), status.view(np.uint8).reshape(S, 1, 1))}

    def call(A):
        lib = lh.lib()
        if "blocks table" in A.plan.tables:
            return lib.cauchy_256_reconstruct_batch_ptrs(k, m, B, S, A.p("blocks"), A.p("rows"), want, A.p("want_rows"),
                                                         A.p("out"), A.p("status"), _stream())
        return lib.cauchy_256_reconstruct_batch(k, m, B, S, A.p("blocks"), A.s("blocks"), A.p("rows"), want, A.p("want_rows"),
                                                A.p("out"), A.s("out"), A.p("status"), _stream())
    entry_point(lh, arena, Job(specs, S, payload, call), form, ["out"], tr.trace_of(k, m), tr.trace_of(k, m, table=True),
                f"reconstruct k {k} m {m} {B} B", seed)


@pytest.mark.parametrize("form", FRAME_FORMS)
def test_frame_unframe_far(lh, oracle, arena, form):
    """cauchy_256_frame_batch and cauchy_256_unframe_batch at k 10, m 4, 64-byte blocks: packets,
    data, recovery and blocks all far; packet i = [row i][block i], and back."""
    (k, m, B), S = FRAME, entry_stripes(form, frame_tile(FRAME[0] + FRAME[1], FRAME[2]))
    data, rec = tu._encoded(oracle, k, m, B, S, 77)
    both = np.concatenate([data, rec], axis=1)
    packets = np.concatenate([np.broadcast_to(np.arange(k + m, dtype=np.uint8)[None, :, None], (S, k + m, 1)), both], axis=2)
    _distinct(packets)
    specs = frame_specs(k, m, B)
    payload = {"data": (data, data), "recovery": (rec, rec), "packets": (np.full_like(packets, C_ROWS), packets)}

    def frame(A):
        return lh.lib().cauchy_256_frame_batch(k, m, B, S, A.p("data"), A.s("data"), A.p("recovery"), A.s("recovery"),
                                               A.p("packets"), A.s("packets"), _stream())
    entry_point(lh, arena, Job(specs, S, payload, frame), form, ["packets"], ["lh_frame_kernel"], None, "frame", 1)
    # the k packets received per stripe: a seeded choice of the k + m, in any order
    rng = np.random.Generator(np.random.PCG64(5))
    pick = np.stack([rng.permutation(k + m)[:k] for _ in range(S)])
    recv = np.ascontiguousarray(packets[np.arange(S)[:, None], pick])
    _distinct(recv)
    specs = unframe_specs(k, B)
    payload = {"packets": (recv, recv), "blocks": (np.full((S, k, B), C_ROWS, dtype=np.uint8), recv[:, :, 1:]),
               "rows": (np.full((S, 1, k), C_STATUS, dtype=np.uint8), pick.astype(np.uint8).reshape(S, 1, k))}

    def unframe(A):
        return lh.lib().cauchy_256_unframe_batch(k, B, S, A.p("packets"), A.s("packets"), A.p("blocks"), A.s("blocks"),
                                                 A.p("rows"), _stream())
    entry_point(lh, arena, Job(specs, S, payload, unframe), form, ["blocks"], ["lh_frame_kernel"], None, "unframe", 2)


def test_python_wrappers_far(lh, oracle, arena):
    """encode_batch, decode_batch and verify_batch on as_strided views of the arena at layout B's
    stride: the wrappers pass stride(0) through unclipped (the jump kernels serve k 10, m 13)."""
    import torch
    N = FAR_STRIPES
    case = sc._case("wrappers", 10, 13, 64, {}, sc._t_one, JUMP)
    job = encode_job(oracle, case, N)
    plan = lhfar.far(f"B stride {lhfar.FAR}", job.specs, N, lhfar.FAR)

    def encode(A):
        lh.encode_batch(A.view("data"), 13, recovery=A.view("recovery"))
    run(lh, arena, plan, job._replace(call=encode), JUMP, "encode_batch wrapper")
    job = decode_job(oracle, case._replace(mode="valid"), N, far=True)
    plan = lhfar.far(f"B stride {lhfar.FAR}", job.specs, N, lhfar.FAR)

    def decode(A):
        lh.decode_batch(A.view("blocks"), A.view("rows").reshape(N, 10), 13, status=A.view("status").reshape(N).view(torch.int8))
    run(lh, arena, plan, job._replace(call=decode), ["lh_plan_kernel(closed form)", "lh_order_kernel", "lh_apply_jump_kernel"],
        "decode_batch wrapper")
    data, rec = tu._encoded(oracle, 10, 13, 64, N, 9)
    specs = [spec("data", 10, 64), spec("recovery", 13, 64), spec("status", 1, 1, True)]
    payload = {"data": (data, data), "recovery": (rec, rec),
               "status": (np.full((N, 1, 1), C_STATUS, dtype=np.uint8), np.zeros((N, 1, 1), dtype=np.uint8))}
    plan = lhfar.far(f"B stride {lhfar.FAR}", specs, N, lhfar.FAR)

    def verify(A):
        lh.verify_batch(A.view("data"), A.view("recovery"), status=A.view("status").reshape(N).view(torch.int8))
    run(lh, arena, plan, Job(specs, N, payload, verify), ["lh_verify_kernel"], "verify_batch wrapper")
