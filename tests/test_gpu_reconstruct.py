"""cauchy_256_reconstruct_batch / _ptrs on the GPU (include/cauchy_256_reconstruct.h;
lh_reconstruct_coef_kernel and lh_reconstruct_kernel in kernels.hip): chosen rows of a stripe's
codeword, data or recovery, from its k survivors and out of place.

The expectation is always first principles (lhreconstruct.case): the codeword is the data followed
by the C oracle's encode of it, the survivors are rows taken from it, and every wanted row must
equal the codeword's row.  Covered: every survivor set of a small code; every lane form with one
tile of wanted rows, a full tile and a tile plus one, the batch one workgroup tile and one stripe
either side; the planner families; the flat 16-byte lanes of m == 1 and k == 1; what must stay
untouched (guards, skipped entries, invalid stripes, the inputs); pointer tables; the product's own
encode and verify; the launch trace; hipGraph capture.  `-m gpu`: needs an MI355X; no case compiles
a module of its own."""
import ctypes
import functools

import numpy as np
import pytest

import lhreconstruct as lr
import lhutil
import test_gpu_ptrs as tp
import test_gpu_untouched as tu
from test_gpu_untouched import C_BLOCKS, C_STATUS

pytestmark = pytest.mark.gpu

KERNELS, KERNELS_PTR = (["lh_reconstruct_coef_kernel", "lh_reconstruct_kernel"],
                        ["lh_reconstruct_coef_kernel", "lh_reconstruct_kernel(pointer table)"])


def planner(k, m):
    """The planner's own entry of the trace (kernels.hip launch_plan; none for m == 1, k == 1)."""
    if lr.is_flat(k, m):
        return []
    e_max = min(k, m)
    if e_max <= 8:
        return ["lh_plan_small_kernel<4>" if e_max <= 4 else "lh_plan_small_kernel<8>"]
    return ["lh_plan_kernel(closed form)" if m >= 7 else "lh_plan_kernel"]


def trace_of(k, m, table=False):
    return planner(k, m) + (KERNELS_PTR if table else KERNELS)


@pytest.fixture(scope="module")
def lh():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    import longhair_amd
    assert longhair_amd.cauchy_256_init() == 0
    return longhair_amd


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def run_strided(lh, k, m, nbytes, cw, rows, want_rows, layout=(0, 0), status=True, counts=None):
    """The C call on guarded buffers: survivors, out and status each between 256-byte guards,
    `layout` = (odd base offset, pad bytes between stripes); out starts as canaries.  For each n
    of `counts` (default: the whole batch) the first n stripes: asserts the wanted rows, that
    skipped entries, invalid stripes, stripes from n on, the guards and the pads keep their
    canaries, the status bytes, and that blocks, rows and want_rows are bit-identical afterwards.
    Returns the launch trace."""
    import torch
    rows, want_rows = np.array(rows, dtype=np.uint8), np.array(want_rows, dtype=np.uint8)
    S, want = want_rows.shape
    blocks, exp, exp_status = lr.case(cw, k, m, rows, want_rows, C_BLOCKS)
    off, pad = layout
    gb = tu.Guarded(blocks.reshape(S, k * nbytes), off, pad, 0x5E)
    d_rows, d_want = torch.from_numpy(rows).cuda(), torch.from_numpy(want_rows).cuda()
    before = gb.buf.clone()
    trace = None
    for n in counts or [S]:
        go = tu.Guarded(np.full((S, want * nbytes), C_BLOCKS, dtype=np.uint8), off + 2 if off else 0, pad, C_BLOCKS)
        gs = tu.Guarded(np.full((1, S), C_STATUS, dtype=np.uint8), 1 if off else 0, 0, C_STATUS)
        torch.cuda.synchronize()
        rc = lh.lib().cauchy_256_reconstruct_batch(k, m, nbytes, n, ctypes.c_void_p(gb.ptr), ctypes.c_longlong(gb.stride),
                                                   ctypes.c_void_p(d_rows.data_ptr()), want,
                                                   ctypes.c_void_p(d_want.data_ptr()), ctypes.c_void_p(go.ptr),
                                                   ctypes.c_longlong(go.stride),
                                                   ctypes.c_void_p(gs.ptr) if status else None, _stream())
        assert rc == 0, (rc, lh.lib().cauchy_256_last_error())
        trace = lh.last_launch()
        torch.cuda.synchronize()
        tag = (k, m, nbytes, want, n, layout)
        got = go.check((tag, "out")).reshape(S, want, nbytes)
        got_status = gs.check((tag, "status")).reshape(S)
        e_out, e_status = exp.copy(), exp_status.view(np.uint8).copy()
        e_out[n:], e_status[n:] = C_BLOCKS, C_STATUS
        wrong = [(s, j) for s in range(S) for j in range(want) if got[s, j].tobytes() != e_out[s, j].tobytes()]
        assert not wrong, (tag, "out blocks (stripe, entry)", wrong[:8], "rows", rows[wrong[0][0]].tolist(),
                           "want", want_rows[wrong[0][0]].tolist())
        if status:
            assert got_status.tolist() == e_status.tolist(), tag
        else:
            assert (got_status == C_STATUS).all(), (tag, "absent status written")
        assert torch.equal(gb.buf, before), (tag, "blocks written")
        assert np.array_equal(d_rows.cpu().numpy(), rows) and np.array_equal(d_want.cpu().numpy(), want_rows), tag
    return trace


# ------------------------------------------------------------------ exhaustive small code
def test_every_survivor_set_of_k4m2(lh, oracle):
    """k4/m2/64: all C(6, 4) = 15 survivor sets x the 24 orders of their slots, all six rows wanted
    at once, one batch of 360 stripes."""
    import itertools
    k, m, nbytes = 4, 2, 64
    rows = [list(p) for c in lr.survivor_sets(k, m) for p in itertools.permutations(c)]
    assert len(rows) == 360
    cw = lr.codewords(oracle, k, m, nbytes, len(rows), 4264)
    assert run_strided(lh, k, m, nbytes, cw, rows, [list(range(k + m))] * len(rows)) == trace_of(k, m)


# ------------------------------------------------------------------ lane forms
# k4/m2 sub-blocks of 1 and 7 bytes (piecewise), 8 (one whole lane), 9 (an overlapping last lane)
# and 162 bytes (21 lanes, a tail of 2); 512 bytes: 64 lanes, a stripe is whole waves and the
# coefficient a scalar
LANES = [8, 56, 64, 72, 1296, 4096]


@pytest.mark.parametrize("want", [1, 4, 5])
@pytest.mark.parametrize("nbytes", LANES)
def test_lane_forms(lh, oracle, nbytes, want):
    """One tile of wanted rows, a full tile, a tile plus one; T - 1, T and T + 1 stripes (T stripes
    per workgroup of lh_reconstruct_kernel)."""
    k, m = 4, 2
    T = lr.stripes_per_workgroup(k, m, nbytes)
    assert T == {8: 256, 56: 256, 64: 256, 72: 128, 1296: 12, 4096: 4}[nbytes]
    S = T + 1
    cw = lr.codewords(oracle, k, m, nbytes, S, 42 + nbytes)
    rows, want_rows = lr.random_batch(k, m, S, want, nbytes * 10 + want)
    assert run_strided(lh, k, m, nbytes, cw, rows, want_rows, counts=[T - 1, T, T + 1]) == trace_of(k, m)


# ------------------------------------------------------------------ planner families
def _family_case(rng, k, m, e):
    """Survivors with e erasures; wanted: a lost recovery row (where one is lost: not with e == m),
    a lost data row (where one is lost, else a second lost recovery row), a present row, and the
    first again."""
    rows = lr.pick_rows(rng, k, m, e)
    lost_rec = [r for r in range(k, k + m) if r not in rows]
    lost_data = [r for r in range(k) if r not in rows]
    first = lost_rec[int(rng.integers(0, len(lost_rec)))] if lost_rec else lost_data[0]
    second = lost_data[int(rng.integers(0, len(lost_data)))] if lost_data else lost_rec[-1]
    return rows, [first, second, rows[int(rng.integers(0, k))], first]


FAMILIES = [(29, 4, 1296, None), (20, 12, 64, None), (128, 32, 64, [32, 1, 0]), (5, 7, 16, None)]


@pytest.mark.parametrize("k,m,nbytes,erasures", FAMILIES, ids=[f"k{k}m{m}b{b}" for k, m, b, _ in FAMILIES])
def test_planner_families(lh, oracle, k, m, nbytes, erasures):
    """lh_plan_small_kernel<4> (k29/m4), lh_plan_kernel with e > 8 (k20/m12; k128/m32: 32 erasures,
    one, none), k < m (k5/m7, lh_plan_small_kernel<8>); every number of erasures of the smaller codes."""
    rng = np.random.Generator(np.random.PCG64(k * 1000 + m))
    erasures = erasures or [e % (min(k, m) + 1) for e in range(2 * min(k, m) + 2)]
    cases = [_family_case(rng, k, m, e) for e in erasures]
    assert any(w[0] >= k for _, w in cases) and any(w[1] < k for _, w in cases) and any(w[1] >= k for _, w in cases)
    cw = lr.codewords(oracle, k, m, nbytes, len(cases), k * 100 + m)
    trace = run_strided(lh, k, m, nbytes, cw, [r for r, _ in cases], [w for _, w in cases], (1, 3))
    assert trace == trace_of(k, m)
    assert trace[0] == {29: "lh_plan_small_kernel<4>", 20: "lh_plan_kernel(closed form)",
                        128: "lh_plan_kernel(closed form)", 5: "lh_plan_small_kernel<8>"}[k]


# ------------------------------------------------------------------ flat lanes
@pytest.mark.parametrize("k,m,nbytes", [(5, 1, 13), (5, 1, 16), (1, 3, 7)], ids=["k5m1b13", "k5m1b16", "k1m3b7"])
def test_flat_shapes(lh, oracle, k, m, nbytes):
    """m == 1: the absent row is the XOR of the survivors; k == 1: every row is the survivor.  Every
    survivor set in two slot orders, every row wanted (a tile plus one or two; one full tile)."""
    sets = lr.survivor_sets(k, m)
    rows = [order for c in sets for order in (c, c[::-1])]
    cw = lr.codewords(oracle, k, m, nbytes, len(rows), 51 + nbytes)
    assert run_strided(lh, k, m, nbytes, cw, rows, [list(range(k + m))] * len(rows), (1, 3)) == KERNELS


def test_m1_repeated_survivor_row_is_invalid(lh, oracle):
    """m == 1, where the planner alone lets any rows pass: a repeated survivor row, a row of k + m
    and a wanted row of k + m are status -1 and write nothing; the valid stripes between them do."""
    k, m, nbytes = 5, 1, 16
    rows = [[0, 1, 2, 3, 4], [0, 1, 1, 3, 4], [5, 1, 2, 3, 4], [5, 1, 5, 3, 4], [0, 6, 2, 3, 4], [0, 1, 2, 3, 5], [0, 1, 2, 3, 5]]
    want = [[5, 0], [5, 0], [0, 5], [0, 5], [5, 0], [4, 6], [4, lr.NONE]]
    cw = lr.codewords(oracle, k, m, nbytes, len(rows), 5116)
    assert lr.case(cw, k, m, rows, want, 0)[2].tolist() == [0, -1, 0, -1, -1, -1, 0]
    for status in (True, False):
        assert run_strided(lh, k, m, nbytes, cw, rows, want, (3, 5), status) == KERNELS


# ------------------------------------------------------------------ what stays untouched
@functools.lru_cache(maxsize=None)
def _mixed(k, m, stripes, want, seed):
    """Valid stripes, stripes with invalid survivor rows (a repeated row; a row of k + m), stripes
    with a wanted row of k + m or 0xFE, and stripes of 0xFF entries only, cycling."""
    rows, wr = lr.random_batch(k, m, stripes, want, seed)
    kinds = []
    for s in range(stripes):
        kind = ("valid", "dup", "valid", "range", "want-range", "none", "valid", "want-fe")[s % 8]
        if kind == "dup":
            rows[s, (s // 8) % k] = rows[s, (s // 8 + 1) % k]
        elif kind == "range":
            rows[s, s % k] = k + m
        elif kind == "want-range":
            wr[s, s % want] = k + m
        elif kind == "want-fe":
            wr[s, s % want] = 0xFE
        elif kind == "none":
            wr[s] = lr.NONE
        kinds.append(kind)
    for a in (rows, wr):
        a.setflags(write=False)
    return rows, wr, kinds


UNTOUCHED = [(29, 4, 1296, 5), (4, 2, 72, 3), (10, 13, 24, 6), (5, 1, 13, 2), (6, 3, 8192, 5)]


@pytest.mark.parametrize("status", [True, False], ids=["status", "no-status"])
@pytest.mark.parametrize("k,m,nbytes,want", UNTOUCHED, ids=[f"k{k}m{m}b{b}" for k, m, b, _ in UNTOUCHED])
def test_untouched_contract(lh, oracle, k, m, nbytes, want, status):
    """40 mixed stripes, out blocks between canary guards at an odd base and a padded out_stride,
    with and without d_status: guards, pads, skipped entries and every out block of an invalid
    stripe keep their canary; blocks, rows and want_rows compare equal to their clones."""
    S = 40
    rows, wr, kinds = _mixed(k, m, S, want, k * 100 + m)
    cw = lr.codewords(oracle, k, m, nbytes, S, k * 1000 + m * 10 + nbytes)
    blocks, exp, exp_status = lr.case(cw, k, m, rows, wr, C_BLOCKS)
    for s, kind in enumerate(kinds):
        assert (exp_status[s] == 0) == (kind in ("valid", "none")), (s, kind)
        if kind != "valid":
            assert (exp[s] == C_BLOCKS).all()
    assert any((exp[s] != C_BLOCKS).any() for s in range(S))
    assert run_strided(lh, k, m, nbytes, cw, rows, wr, (3, 5), status) == trace_of(k, m)


# ------------------------------------------------------------------ pointer tables
PTRS = [(29, 4, 1304, 5), (4, 2, 56, 4), (20, 12, 64, 3), (5, 1, 13, 2), (1, 3, 7, 4), (6, 3, 4096, 5)]


@pytest.mark.parametrize("k,m,nbytes,want", PTRS, ids=[f"k{k}m{m}b{b}" for k, m, b, _ in PTRS])
def test_pointer_tables(lh, oracle, k, m, nbytes, want):
    """Every survivor and every out block at a random place and byte offset of a pool; the out
    pointer of a 0xFF entry points into a buffer of its own that nothing may touch."""
    import torch
    S = 40
    rows, wr, kinds = _mixed(k, m, S, want, k * 100 + m + 1)
    cw = lr.codewords(oracle, k, m, nbytes, S, k * 1000 + m * 10 + nbytes + 1)
    blocks, exp, exp_status = lr.case(cw, k, m, rows, wr, 0xA5)   # (tp._scatter fills its pool with 0xA5)
    bpool, bptrs, bplace = tp._scatter(torch.from_numpy(blocks).cuda(), 31)
    opool, optrs, oplace = tp._scatter(torch.full((S, want, nbytes), 0xA5, dtype=torch.uint8, device="cuda"), 32)
    assert int((bptrs % 2).sum()) > 0 and int((optrs % 2).sum()) > 0   # odd addresses among them
    unread = torch.full((nbytes + 64,), 0x3C, dtype=torch.uint8, device="cuda")
    skipped = torch.from_numpy(wr == lr.NONE).cuda()
    assert int(skipped.sum()) > 0
    optrs = torch.where(skipped, torch.full_like(optrs, unread.data_ptr() + 1), optrs).contiguous()
    d_rows, d_want = torch.from_numpy(np.array(rows)).cuda(), torch.from_numpy(np.array(wr)).cuda()
    before = [t.clone() for t in (bpool, bptrs, optrs, d_rows, d_want)]
    status = torch.full((S,), C_STATUS, dtype=torch.int8, device="cuda")
    got_status = lh.reconstruct_batch_ptrs(k, m, nbytes, bptrs, d_rows, d_want, optrs, status=status)
    assert lh.last_launch() == trace_of(k, m, table=True)
    torch.cuda.synchronize()
    assert got_status is status and status.cpu().numpy().tolist() == exp_status.tolist()
    got = tp._gather(opool, oplace).cpu().numpy()
    wrong = [(s, j) for s in range(S) for j in range(want) if got[s, j].tobytes() != exp[s, j].tobytes()]
    assert not wrong, ((k, m, nbytes), "out blocks (stripe, entry)", wrong[:8])
    tp._gaps_untouched(opool, oplace)
    assert int((unread != 0x3C).sum()) == 0, "the out block of a 0xFF entry was written"
    for t, b in zip((bpool, bptrs, optrs, d_rows, d_want), before):
        assert torch.equal(t, b), "an input was written"


# ------------------------------------------------------------------ the product's own encode and verify
def test_encode_reconstruct_verify(lh):
    """k29/m4/1296, 24 stripes, through the wrappers: encode_batch; each stripe loses four of its 33
    blocks (the first walks over data and recovery rows, the others are random); reconstruct_batch
    of the four; the reassembled stripe verifies clean and equals the encoded one.  The survivors
    are bit-identical afterwards."""
    import torch
    k, m, nbytes, S, W = 29, 4, 1296, 24, 4
    rng = np.random.Generator(np.random.PCG64(2908))
    d_data = torch.from_numpy(lhutil.fill(2908, S * k * nbytes).reshape(S, k, nbytes)).cuda()
    rec = lh.encode_batch(d_data, m)
    full = torch.cat([d_data, rec], dim=1)
    rows = np.empty((S, k), dtype=np.uint8)
    want = np.empty((S, W), dtype=np.uint8)
    for s in range(S):
        lost = [(s * 7) % (k + m)] + [int(x) for x in rng.permutation(k + m)]
        lost = list(dict.fromkeys(lost))[:W]
        rows[s] = rng.permutation([r for r in range(k + m) if r not in lost])
        want[s] = lost
    assert {int(w) for w in want[:, 0]} & set(range(k, k + m)) and {int(w) for w in want[:, 0]} & set(range(k))
    d_rows, d_want = torch.from_numpy(rows).cuda(), torch.from_numpy(want).cuda()
    idx = d_rows.long()[:, :, None].expand(S, k, nbytes)
    blocks = torch.gather(full, 1, idx).contiguous()
    keep_blocks, keep_rows = blocks.clone(), d_rows.clone()
    out, status = lh.reconstruct_batch(blocks, d_rows, m, d_want)
    assert lh.last_launch() == trace_of(k, m)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (S, W, nbytes) and status.dtype == torch.int8
    torch.cuda.synchronize()
    assert int((status != 0).sum()) == 0
    assert torch.equal(blocks, keep_blocks) and torch.equal(d_rows, keep_rows)
    # reassemble: the survivors and the rebuilt rows back at their places of a zeroed codeword
    again = torch.zeros_like(full)
    again.scatter_(1, idx, blocks)
    again.scatter_(1, d_want.long()[:, :, None].expand(S, W, nbytes), out)
    bad = torch.full((S, m), 0x5E, dtype=torch.uint8, device="cuda")
    vstatus = lh.verify_batch(again[:, :k].contiguous(), again[:, k:].contiguous(), bad_rows=bad)
    torch.cuda.synchronize()
    assert int((vstatus != 0).sum()) == 0 and int((bad != 0).sum()) == 0
    assert torch.equal(again, full)
    # a skipped entry of an allocated `out` reads as zeros
    d_want[:, 1] = lr.NONE
    out2, _ = lh.reconstruct_batch(blocks, d_rows, m, d_want)
    torch.cuda.synchronize()
    assert int((out2[:, 1] != 0).sum()) == 0 and torch.equal(out2[:, 0], out[:, 0]) and torch.equal(out2[:, 2], out[:, 2])


def test_last_launch_trace(lh, oracle):
    """The planner's own entry, then lh_reconstruct_coef_kernel and lh_reconstruct_kernel, in
    launch order; no planner for m == 1; `(pointer table)` on the table form."""
    assert trace_of(29, 4) == ["lh_plan_small_kernel<4>", "lh_reconstruct_coef_kernel", "lh_reconstruct_kernel"]
    assert trace_of(5, 1) == ["lh_reconstruct_coef_kernel", "lh_reconstruct_kernel"]
    assert trace_of(200, 55, True) == ["lh_plan_kernel(closed form)", "lh_reconstruct_coef_kernel",
                                       "lh_reconstruct_kernel(pointer table)"]
    import torch
    for k, m, nbytes in ((29, 4, 64), (5, 1, 13), (10, 13, 24)):
        cw = lr.codewords(oracle, k, m, nbytes, 3, 9)
        rows, wr = lr.random_batch(k, m, 3, 2, 9)
        blocks, exp, _ = lr.case(cw, k, m, rows, wr, 0)
        d_blocks, d_rows, d_want = (torch.from_numpy(a).cuda() for a in (blocks, rows, wr))
        out, status = lh.reconstruct_batch(d_blocks, d_rows, m, d_want)
        assert lh.last_launch() == trace_of(k, m)
        ptrs = lambda t: (t.data_ptr() + torch.arange(t.shape[0] * t.shape[1], device="cuda") * nbytes).reshape(t.shape[:2])   # noqa: E731
        out2 = torch.zeros_like(out)
        lh.reconstruct_batch_ptrs(k, m, nbytes, ptrs(d_blocks), d_rows, d_want, ptrs(out2))
        assert lh.last_launch() == trace_of(k, m, table=True)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), exp) and torch.equal(out, out2)


# ------------------------------------------------------------------ hipGraph
def test_reconstruct_captures_in_a_graph(lh, oracle):
    """A capture on a stream without an earlier call of the size returns -3, launches nothing and
    leaves the stream usable; after one uncaptured call the same call captures without running
    (the canaries stay), and two replays follow the survivors' contents."""
    import torch
    k, m, nbytes, S, want = 29, 4, 1296, 24, 2
    cws = [lr.codewords(oracle, k, m, nbytes, S, seed) for seed in (81, 82, 83)]
    rows, wr = lr.random_batch(k, m, S, want, 81)
    cases = [lr.case(cw, k, m, rows, wr, C_BLOCKS) for cw in cws]
    d_blocks = torch.from_numpy(cases[0][0]).cuda()
    d_rows, d_want = torch.from_numpy(rows).cuda(), torch.from_numpy(wr).cuda()
    out = torch.full((S, want, nbytes), C_BLOCKS, dtype=torch.uint8, device="cuda")
    status = torch.full((S,), C_STATUS, dtype=torch.int8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    failed = None
    try:
        with torch.cuda.graph(torch.cuda.CUDAGraph(), stream=s):
            try:
                lh.reconstruct_batch(d_blocks, d_rows, m, d_want, out=out, status=status, stream=s)
            except lh.LonghairError as e:
                failed = e
                assert lh.last_launch() == []
    except RuntimeError:
        pass  # an empty capture may be rejected by torch; what matters is the codec's error
    assert failed is not None and failed.code == -3 and "capture" in str(failed)
    torch.cuda.synchronize()
    assert int((out != C_BLOCKS).sum()) == 0 and int((status != C_STATUS).sum()) == 0
    # the stream is usable: the uncaptured call of the same size
    lh.reconstruct_batch(d_blocks, d_rows, m, d_want, out=out, status=status, stream=s)
    s.synchronize()
    assert np.array_equal(out.cpu().numpy(), cases[0][1]) and int((status != 0).sum()) == 0
    out.fill_(C_BLOCKS)
    status.fill_(C_STATUS)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        lh.reconstruct_batch(d_blocks, d_rows, m, d_want, out=out, status=status, stream=s)
        assert lh.last_launch() == trace_of(k, m)
    torch.cuda.synchronize()
    assert int((out != C_BLOCKS).sum()) == 0 and int((status != C_STATUS).sum()) == 0   # capture runs nothing
    for blocks, exp, exp_status in cases[1:]:
        d_blocks.copy_(torch.from_numpy(blocks))
        out.fill_(C_BLOCKS)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), exp) and status.cpu().numpy().tolist() == exp_status.tolist()
    assert np.array_equal(d_rows.cpu().numpy(), rows) and np.array_equal(d_want.cpu().numpy(), wr)
