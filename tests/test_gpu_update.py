"""cauchy_256_update_batch / _ptrs on the GPU (include/cauchy_256_update.h; lh_update_kernel in
kernels.hip): the recovery blocks of encoded stripes patched after a few data blocks changed.

The expected recovery is always the C oracle's encode of the patched data, byte for byte
(lhupdate.update_case; tests/test_update_model.py pins the same identity on the CPU).  Covered:
every lane form of the kernel (whole 8-byte lanes, a last lane of 1..7 bytes, sub-blocks under
a lane, the flat 16-byte lanes of m == 1 and k == 1 with their byte tails), mixed batches of
valid, unchanged and invalid stripes between canary guards, the batch size swept over the
kernel's workgroup tile, the delta form, pointer tables, the composition encode / update /
decode, and hipGraph capture.  `-m gpu`: needs an MI355X; no case compiles a module of its own."""
import ctypes
import functools

import numpy as np
import pytest

import lhupdate
import lhutil
import test_gpu_ptrs as tp
import test_gpu_stripe_counts as tsc
import test_gpu_untouched as tu
from test_gpu_untouched import C_BLOCKS, C_STATUS

pytestmark = pytest.mark.gpu

TRACE, TRACE_PTR = ["lh_update_kernel"], ["lh_update_kernel(pointer table)"]
# block sizes at (29, 4): sub-blocks of 1, 3, 5, 7 (under a lane), 8, 17, 162, 163 and 513 bytes
WIDTHS = [(29, 4, b) for b in (8, 24, 40, 56, 64, 136, 1296, 1304, 4104)] + [
    (4, 2, 16), (10, 13, 24), (200, 56, 64), (5, 1, 13), (255, 1, 8), (1, 3, 16)]
# one shape per class of the kernel's lanes, for the mixed batches
CLASSES = [("sub7", 29, 4, 56), ("lane-and-tail", 29, 4, 1304), ("wider-than-a-wave", 29, 4, 4104),
           ("m56-tiles", 200, 56, 64), ("m13-sub3", 10, 13, 24), ("flat-m1", 5, 1, 13), ("flat-k1", 1, 3, 16)]


@pytest.fixture(scope="module")
def lh():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    import longhair_amd
    assert longhair_amd.cauchy_256_init() == 0
    return longhair_amd


def _t_update(lh, k, m, nbytes):
    """kernels.hip launch_update: ceil(stripes * nch / 256) workgroups, nch = ceil(span / lane)
    lanes per stripe: 8-byte lanes over the sub-block (bytes / 8), or, for m == 1 and k == 1,
    16-byte lanes over the whole block."""
    nch = -(-nbytes // 16) if (m == 1 or k == 1) else -(-(nbytes // 8) // 8)
    return max(1, 256 // nch)


@functools.lru_cache(maxsize=None)
def _case(oracle, k, m, nbytes, stripes, changes, seed, mixed):
    """One batch and its expectation, computed once: (rec, cols, old, new, expected, status)."""
    data, rec = tu._encoded(oracle, k, m, nbytes, stripes, seed)
    bad = tu.pick_invalid(stripes, seed) if mixed and k < 255 else []
    return tu._frozen(rec, *lhupdate.update_case(oracle, data, rec, k, m, nbytes, changes, seed, bad))


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def run_strided(lh, k, m, nbytes, case, layout=(0, 0), status=True, delta=False):
    """The C call on guarded buffers: recovery, status, old and new each between 256-byte guards,
    `layout` = (odd base offset, pad bytes between stripes).  Asserts the expectation, the guards
    and that old / new are not written.  Returns the launch trace."""
    import torch
    rec, cols, old, new, exp, exp_status = case
    S, c = cols.shape
    off, pad = layout
    if delta:
        old, new = old ^ new, None
    gr = tu.Guarded(rec.reshape(S, m * nbytes), off, pad, C_BLOCKS)
    gs = tu.Guarded(np.full((1, S), C_STATUS, dtype=np.uint8), 1 if off else 0, 0, C_STATUS)
    go = tu.Guarded(old.reshape(S, c * nbytes), off, pad, 0x5E)
    gn = tu.Guarded(new.reshape(S, c * nbytes), off + 1 if off else 0, pad, 0x5E) if new is not None else None
    d_cols = torch.from_numpy(np.array(cols)).cuda()
    before = [g.buf.clone() for g in (go, gn) if g is not None]
    torch.cuda.synchronize()
    rc = lh.lib().cauchy_256_update_batch(k, m, nbytes, S, c, ctypes.c_void_p(d_cols.data_ptr()),
                                          ctypes.c_void_p(go.ptr), ctypes.c_longlong(go.stride),
                                          ctypes.c_void_p(gn.ptr) if gn else None, ctypes.c_longlong(gn.stride if gn else 0),
                                          ctypes.c_void_p(gr.ptr), ctypes.c_longlong(gr.stride),
                                          ctypes.c_void_p(gs.ptr) if status else None, _stream())
    assert rc == 0, (rc, lh.lib().cauchy_256_last_error())
    trace = lh.last_launch()
    torch.cuda.synchronize()
    tag = (k, m, nbytes, c, layout, "delta" if delta else "old+new")
    got = gr.check((tag, "recovery")).reshape(S, m, nbytes)
    got_status = gs.check((tag, "status")).reshape(S).view(np.int8)
    for s in range(S):
        wrong = [r for r in range(m) if got[s, r].tobytes() != exp[s, r].tobytes()]
        assert not wrong, (tag, "stripe", s, "cols", cols[s].tolist(), "status", int(exp_status[s]), "recovery blocks", wrong)
    if status:
        assert got_status.tolist() == exp_status.tolist(), tag
    else:
        assert (got_status.view(np.uint8) == C_STATUS).all(), tag
    for g, b in zip([g for g in (go, gn) if g is not None], before):
        assert torch.equal(g.buf, b), (tag, "old / new written")
    assert torch.equal(d_cols.cpu(), torch.from_numpy(np.array(cols))), (tag, "cols written")
    return trace


@pytest.mark.parametrize("k,m,nbytes", WIDTHS, ids=[f"k{k}m{m}b{b}" for k, m, b in WIDTHS])
def test_lane_widths_and_tails(lh, oracle, k, m, nbytes):
    """Every lane form, 40 stripes of two changes (distinct, repeated, with a 0xFF entry, none)."""
    case = _case(oracle, k, m, nbytes, 40, 2, k * 1000 + m * 10 + nbytes, False)
    assert (case[5] == 0).all() and not np.array_equal(case[0], case[4])
    assert run_strided(lh, k, m, nbytes, case) == TRACE


@pytest.mark.parametrize("status", [True, False], ids=["status", "no-status"])
@pytest.mark.parametrize("changes", [1, 3])
@pytest.mark.parametrize("name,k,m,nbytes", CLASSES, ids=[c[0] for c in CLASSES])
def test_mixed_batch(lh, oracle, name, k, m, nbytes, changes, status):
    """Valid stripes (repeated columns, 0xFF entries), stripes of 0xFF entries only (untouched,
    status 0) and invalid ones (stripe 0, the last, two adjacent, a column of k and of 0xFE: untouched,
    status -1), from an odd base with pad bytes between stripes; d_status may be NULL."""
    S = 40
    case = _case(oracle, k, m, nbytes, S, changes, k * 1000 + m * 10 + nbytes + changes, True)
    rec, cols, old, new, exp, exp_status = case
    bad = np.nonzero(exp_status)[0].tolist()
    assert 0 in bad and S - 1 in bad and any(b + 1 in bad for b in bad) and S // 5 <= len(bad) <= S // 3
    assert {int(cols[s][cols[s] != lhupdate.NONE].max()) for s in bad} == {k, 0xFE}
    none = [s for s in range(S) if (cols[s] == lhupdate.NONE).all()]
    assert none and all(exp_status[s] == 0 for s in none)
    for s in bad + none:
        assert np.array_equal(exp[s], rec[s])
    if changes == 3:
        assert any(exp_status[s] == 0 and cols[s][0] == cols[s][2] != lhupdate.NONE for s in range(S))
    assert run_strided(lh, k, m, nbytes, case, (3, 5), status) == TRACE


@pytest.mark.parametrize("k,m,nbytes", [(29, 4, 1304), (29, 4, 56), (5, 1, 13), (200, 56, 64)])
def test_delta_form(lh, oracle, k, m, nbytes):
    """new == NULL: old holds the deltas; the same recovery as the old + new form."""
    case = _case(oracle, k, m, nbytes, 40, 3, k * 1000 + m * 10 + nbytes + 3, True)
    assert run_strided(lh, k, m, nbytes, case, (3, 5), delta=True) == TRACE


# ------------------------------------------------------------------ batch sizes
COUNTS = [("packed-small-blocks", 29, 4, 64), ("wider-than-a-wave", 29, 4, 4104)]


@pytest.mark.parametrize("name,k,m,nbytes", COUNTS, ids=[c[0] for c in COUNTS])
def test_update_counts(lh, oracle, name, k, m, nbytes):
    """Every prefix length lhutil.stripe_counts(T) of one mixed batch (T stripes per workgroup:
    256 one-lane stripes; 3 stripes of 65 lanes): stripes < n are patched or, invalid, untouched
    with status -1; every byte from stripe n on -- recovery, status, guards -- is what it was."""
    import torch
    T = _t_update(lh, k, m, nbytes)
    assert T == (256 if nbytes == 64 else 3)
    counts = lhutil.stripe_counts(T)
    N, c = counts[-1] + 1, 2
    rec, cols, old, new, exp, exp_status = _case(oracle, k, m, nbytes, N, c, k * 1000 + m * 10 + nbytes + 5, True)
    R, gr = tsc._strided("recovery", rec.reshape(N, m * nbytes), exp.reshape(N, m * nbytes), C_BLOCKS, nbytes)
    S, gs = tsc._strided("status", np.full((N, 1), C_STATUS, dtype=np.uint8), exp_status.view(np.uint8).reshape(N, 1),
                         C_STATUS, 1)
    d_cols, d_old, d_new = (torch.from_numpy(np.array(a)).cuda() for a in (cols, old, new))
    lib = lh.lib()
    vp, ll = ctypes.c_void_p, ctypes.c_longlong

    def call(n):
        rc = lib.cauchy_256_update_batch(k, m, nbytes, n, c, vp(d_cols.data_ptr()), vp(d_old.data_ptr()), ll(c * nbytes),
                                         vp(d_new.data_ptr()), ll(c * nbytes), vp(gr.ptr), ll(gr.stride), vp(gs.ptr),
                                         _stream())
        assert rc == 0, (name, n, rc, lib.cauchy_256_last_error())
    case = tsc._case("update-" + name, k, m, nbytes, {}, _t_update, TRACE)
    failing, traces, calls, seconds, ran = tsc.sweep(lh, case, counts, [R, S], call)
    assert calls == len(counts) and sorted(ran) == counts
    assert traces[counts[-1]] == TRACE and traces[1] == TRACE
    if failing:
        pytest.fail(tsc._report(case, T, counts, failing, ran, [R, S], call), pytrace=False)


# ------------------------------------------------------------------ pointer tables
@pytest.mark.parametrize("delta", [False, True], ids=["old+new", "delta"])
@pytest.mark.parametrize("k,m,nbytes", [(29, 4, 1304), (29, 4, 56), (200, 56, 64), (5, 1, 13), (1, 3, 16)])
def test_pointer_tables(lh, oracle, k, m, nbytes, delta):
    """Every old, new and recovery block at a random place and byte offset of a pool: the same
    recovery, the pools' gaps and the old / new blocks untouched."""
    import torch
    S, c = 40, 3
    rec, cols, old, new, exp, exp_status = _case(oracle, k, m, nbytes, S, c, k * 1000 + m * 10 + nbytes + 3, True)
    if delta:
        old, new = old ^ new, None
    rpool, rptrs, rplace = tp._scatter(torch.from_numpy(np.array(rec)).cuda(), 11)
    opool, optrs, _ = tp._scatter(torch.from_numpy(np.array(old)).cuda(), 12)
    npool, nptrs = None, None
    if new is not None:
        npool, nptrs, _ = tp._scatter(torch.from_numpy(np.array(new)).cuda(), 13)
    d_cols = torch.from_numpy(np.array(cols)).cuda()
    status = torch.full((S,), C_STATUS, dtype=torch.int8, device="cuda")
    before = [t.clone() for t in (opool, npool) if t is not None]
    got_status = lh.update_batch_ptrs(k, m, nbytes, d_cols, optrs, nptrs, rptrs, status=status)
    assert lh.last_launch() == TRACE_PTR
    torch.cuda.synchronize()
    assert got_status is status and status.cpu().numpy().tolist() == exp_status.tolist()
    got = tp._gather(rpool, rplace).cpu().numpy()
    for s in range(S):
        wrong = [r for r in range(m) if got[s, r].tobytes() != exp[s, r].tobytes()]
        assert not wrong, ((k, m, nbytes), "stripe", s, "cols", cols[s].tolist(), "recovery blocks", wrong)
    tp._gaps_untouched(rpool, rplace)
    for t, b in zip([t for t in (opool, npool) if t is not None], before):
        assert torch.equal(t, b), "old / new written"


def test_wrapper_strided_trace(lh, oracle):
    """longhair_amd.update_batch on plain tensors: returns the status it allocated."""
    import torch
    k, m, nbytes, S, c = 29, 4, 1296, 24, 3
    rec, cols, old, new, exp, exp_status = _case(oracle, k, m, nbytes, S, c, 77, True)
    d_rec, d_cols, d_old, d_new = (torch.from_numpy(np.array(a)).cuda() for a in (rec, cols, old, new))
    status = lh.update_batch(k, d_rec, d_cols, d_old, d_new)
    assert lh.last_launch() == TRACE
    assert status.dtype == torch.int8 and status.cpu().numpy().tolist() == exp_status.tolist()
    assert np.array_equal(d_rec.cpu().numpy(), exp)


# ------------------------------------------------------------------ composition
def test_encode_update_decode(lh):
    """k29/m4/1296, 24 stripes: encode, change two blocks per stripe and patch the recovery, lose
    exactly those two blocks, decode from recovery rows: the decode yields the new data."""
    import torch
    k, m, nbytes, S = 29, 4, 1296, 24
    rng = np.random.Generator(np.random.PCG64(2904))
    data = lhutil.fill(2904, S * k * nbytes).reshape(S, k, nbytes)
    new = lhutil.fill(2905, S * 2 * nbytes).reshape(S, 2, nbytes)
    cols = np.stack([np.sort(rng.choice(k, size=2, replace=False)) for _ in range(S)]).astype(np.uint8)
    d_data = torch.from_numpy(data).cuda()
    rec = lh.encode_batch(d_data, m)
    assert lh.last_launch() == ["lh_jit_encode"]
    d_cols = torch.from_numpy(cols).cuda()
    idx = d_cols.long()[:, :, None].expand(S, 2, nbytes)
    d_old = torch.gather(d_data, 1, idx).contiguous()
    status = lh.update_batch(k, rec, d_cols, d_old, torch.from_numpy(new).cuda())
    assert lh.last_launch() == TRACE and int((status != 0).sum()) == 0
    patched = data.copy()
    for s in range(S):
        patched[s, cols[s]] = new[s]
    assert np.array_equal(lh.encode_batch(torch.from_numpy(patched).cuda(), m).cpu().numpy(), rec.cpu().numpy())
    blocks = torch.from_numpy(patched).cuda()
    rows = torch.arange(k, dtype=torch.uint8, device="cuda").repeat(S, 1)
    use = [(1, 3), (0, 2), (3, 0)]
    for s in range(S):
        for j in range(2):
            r = use[s % 3][j]
            blocks[s, int(cols[s, j])] = rec[s, r]
            rows[s, int(cols[s, j])] = k + r
    st = lh.decode_batch(blocks, rows, m)
    torch.cuda.synchronize()
    assert int((st != 0).sum()) == 0
    got, got_rows = blocks.cpu().numpy(), rows.cpu().numpy()
    for s in range(S):
        assert sorted(got_rows[s].tolist()) == list(range(k)), s
        for i in range(k):
            assert got[s, i].tobytes() == patched[s, got_rows[s, i]].tobytes(), (s, i)


# ------------------------------------------------------------------ hipGraph
def test_update_captures_in_a_graph(lh, oracle):
    """On a prepared stream one update captures without running; a replay patches the recovery,
    a second replay gives the original bytes back (XOR is an involution)."""
    import torch
    k, m, nbytes, S, c = 29, 4, 1296, 24, 2
    rec, cols, old, new, exp, exp_status = _case(oracle, k, m, nbytes, S, c, 78, False)
    d_rec, d_cols, d_old, d_new = (torch.from_numpy(np.array(a)).cuda() for a in (rec, cols, old, new))
    status = torch.full((S,), C_STATUS, dtype=torch.int8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    lh.prepare(k, m, nbytes, S, stream=s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        lh.update_batch(k, d_rec, d_cols, d_old, d_new, status=status, stream=s)
        assert lh.last_launch() == TRACE
    torch.cuda.synchronize()
    assert np.array_equal(d_rec.cpu().numpy(), rec) and int((status != C_STATUS).sum()) == 0   # capture runs nothing
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(d_rec.cpu().numpy(), exp) and int((status != 0).sum()) == 0
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(d_rec.cpu().numpy(), rec)


def test_update_capture_never_allocates(lh):
    """A code whose generator is not on the device yet: the call made during capture returns -3
    and enqueues nothing (the recovery is untouched after the capture ends).  The generators are
    kept per (k, m) for the life of the process, so the first of a few codes no other test names
    that is still unloaded serves (one of them must be)."""
    import torch
    nbytes, S, c = 64, 8, 1
    failed = None
    for k, m in ((151, 23), (173, 29), (211, 37)):
        d_rec = torch.full((S, m, nbytes), 0x3C, dtype=torch.uint8, device="cuda")
        d_cols = torch.zeros((S, c), dtype=torch.uint8, device="cuda")
        d_old = torch.full((S, c, nbytes), 0xFF, dtype=torch.uint8, device="cuda")
        status = torch.full((S,), C_STATUS, dtype=torch.int8, device="cuda")
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(graph, stream=s):
                try:
                    lh.update_batch(k, d_rec, d_cols, d_old, status=status, stream=s)
                except lh.LonghairError as e:
                    failed = e
                    assert lh.last_launch() == []
        except RuntimeError:
            pass  # an empty capture may be rejected by torch; what matters is the codec's error
        torch.cuda.synchronize()
        assert int((d_rec != 0x3C).sum()) == 0 and int((status != C_STATUS).sum()) == 0   # capture runs nothing
        if failed is not None:
            break
    assert failed is not None and failed.code == -3 and "capture" in str(failed)
    # outside a capture the same call loads the generator and runs
    lh.update_batch(k, d_rec, d_cols, d_old, status=status)
    torch.cuda.synchronize()
    assert lh.last_launch() == TRACE and int((status != 0).sum()) == 0 and int((d_rec[:, 0] != 0xC3).sum()) == 0
