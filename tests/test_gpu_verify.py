"""cauchy_256_verify_batch / _ptrs on the GPU (include/cauchy_256_verify.h; lh_verify_kernel in
kernels.hip): do the stored recovery blocks still belong to the stored data?

The expectation is always first principles (lhverify.expected): row r of stripe s is bad iff the
stored recovery bytes differ from the C oracle's encode of the stored data.  Covered: every
byte of every block is looked at (one flipped bit per stripe, recovery side and data side, at
block sizes whose sub-blocks are under a lane, one lane, and a lane and a tail, and the flat
16-byte lanes of m == 1 and k == 1); large blocks and every row tile with mixed corruption
styles between canary guards, either output absent, inputs bit-identical afterwards; the batch
size swept over the kernel's workgroup tile; pointer tables; the product's own encoder and
update; hipGraph capture.  `-m gpu`: needs an MI355X; no case compiles a module of its own."""
import ctypes
import functools

import numpy as np
import pytest

import lhutil
import lhverify
import test_gpu_ptrs as tp
import test_gpu_stripe_counts as tsc
import test_gpu_untouched as tu
from test_gpu_untouched import C_BLOCKS, C_STATUS

pytestmark = pytest.mark.gpu

TRACE, TRACE_PTR = ["lh_verify_kernel"], ["lh_verify_kernel(pointer table)"]
C_ROWS = 0x5E   # canary of bad_rows: neither 0 nor 1
# sub-blocks of 1, 3, 5, 7 (under a lane), 8 (one lane) and 17 bytes (a lane and a 1-byte tail)
BYTES = [(29, 4, b) for b in (8, 24, 40, 56, 64, 136)]
FLAT = [(5, 1, 13), (255, 1, 8), (1, 3, 16)]
LARGE = [(29, 4, 1296), (29, 4, 1304), (29, 4, 4104), (200, 56, 64), (10, 13, 24), (4, 2, 16)]


def _ids(shapes):
    return [f"k{k}m{m}b{b}" for k, m, b in shapes]


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


def run_strided(lh, k, m, nbytes, data, rec, exp_status, exp_bad, layout=(0, 0), status=True, bad_rows=True):
    """The C call on guarded buffers: data, recovery, status and bad_rows each between 256-byte
    guards, `layout` = (odd base offset, pad bytes between stripes).  Asserts the expectation,
    every guard and pad, that an absent output's buffer keeps its canaries and that data and
    recovery are bit-identical afterwards.  Returns the launch trace."""
    import torch
    S = data.shape[0]
    off, pad = layout
    gd = tu.Guarded(data.reshape(S, k * nbytes), off, pad, C_BLOCKS)
    gr = tu.Guarded(rec.reshape(S, m * nbytes), off + 2 if off else 0, pad, C_BLOCKS)
    gs = tu.Guarded(np.full((1, S), C_STATUS, dtype=np.uint8), 1 if off else 0, 0, C_STATUS)
    gb = tu.Guarded(np.full((1, S * m), C_ROWS, dtype=np.uint8), 3 if off else 0, 0, C_ROWS)
    before = [g.buf.clone() for g in (gd, gr)]
    torch.cuda.synchronize()
    rc = lh.lib().cauchy_256_verify_batch(k, m, nbytes, S, ctypes.c_void_p(gd.ptr), ctypes.c_longlong(gd.stride),
                                          ctypes.c_void_p(gr.ptr), ctypes.c_longlong(gr.stride),
                                          ctypes.c_void_p(gs.ptr) if status else None,
                                          ctypes.c_void_p(gb.ptr) if bad_rows else None, _stream())
    assert rc == 0, (rc, lh.lib().cauchy_256_last_error())
    trace = lh.last_launch()
    torch.cuda.synchronize()
    tag = (k, m, nbytes, S, layout)
    got_status = gs.check((tag, "status")).reshape(S)
    got_bad = gb.check((tag, "bad_rows")).reshape(S, m)
    if status:
        wrong = np.nonzero(got_status.view(np.int8) != exp_status)[0]
        assert wrong.size == 0, (tag, "status of stripes", wrong.tolist()[:8], got_status[wrong][:8].tolist())
    else:
        assert (got_status == C_STATUS).all(), (tag, "absent status written")
    if bad_rows:
        wrong = np.argwhere(got_bad != exp_bad)
        assert wrong.size == 0, (tag, "bad_rows at (stripe, row)", wrong.tolist()[:8],
                                 [int(got_bad[s, r]) for s, r in wrong[:8]])
    else:
        assert (got_bad == C_ROWS).all(), (tag, "absent bad_rows written")
    for g, b, what in zip((gd, gr), before, ("data", "recovery")):
        assert torch.equal(g.buf, b), (tag, what, "written")
    return trace


# ------------------------------------------------------------------ every byte is looked at
@functools.lru_cache(maxsize=None)
def _sweeps(oracle, k, m, nbytes):
    seed = k * 1000 + m * 10 + nbytes
    clean = lhverify.encoded(oracle, k, m, nbytes, nbytes * m, seed)
    rec_side = lhverify.byte_sweep_recovery(oracle, k, m, nbytes, seed)
    data_side = lhverify.byte_sweep_data(oracle, k, m, nbytes, seed + 1)
    return [(d, r) + lhverify.expected(oracle, k, m, nbytes, d, r) for d, r in (clean, rec_side, data_side)]


@pytest.mark.parametrize("k,m,nbytes", BYTES + FLAT, ids=_ids(BYTES + FLAT))
def test_every_byte_is_looked_at(lh, oracle, k, m, nbytes):
    """One flipped bit per stripe: byte p of recovery row r (stripe p m + r: that row alone is
    bad), byte p of data block p % k (stripe p: every row is bad); the clean batch first."""
    clean, rec_side, data_side = _sweeps(oracle, k, m, nbytes)
    assert not clean[2].any() and not clean[3].any()
    d, r, status, bad = rec_side
    assert status.all() and np.array_equal(bad.reshape(nbytes, m, m), np.broadcast_to(np.eye(m, dtype=np.uint8), (nbytes, m, m)))
    assert data_side[2].all() and data_side[3].all() and data_side[0].shape[0] == nbytes
    for case in (clean, rec_side, data_side):
        assert run_strided(lh, k, m, nbytes, *case) == TRACE


# ------------------------------------------------------------------ large blocks and row tiles
@functools.lru_cache(maxsize=None)
def _mixed(oracle, k, m, nbytes, stripes=40):
    return lhverify.corrupt_case(oracle, k, m, nbytes, stripes, k * 1000 + m * 10 + nbytes + 1)


@pytest.mark.parametrize("outputs", ["both", "no-status", "no-bad-rows"])
@pytest.mark.parametrize("k,m,nbytes", LARGE, ids=_ids(LARGE))
def test_mixed_batch_between_guards(lh, oracle, k, m, nbytes, outputs):
    """40 stripes, the corruption styles cycling (clean, one recovery byte, two recovery rows, one
    data bit, a recovery block of another stripe), positions and rows from lhverify; data and
    recovery from an odd base with pad bytes between stripes; either output may be NULL."""
    data, rec, status, bad, plan = _mixed(oracle, k, m, nbytes)
    rows = {r for style, meant in plan if style in ("rec-byte", "two-rows", "swapped-block") for r in meant}
    assert rows == set(lhverify.tile_rows(m)) or len(plan) < 2 * len(lhverify.tile_rows(m))
    if m == 13:
        assert 12 in rows
    assert run_strided(lh, k, m, nbytes, data, rec, status, bad, (3, 5), outputs != "no-status",
                       outputs != "no-bad-rows") == TRACE


def test_row_tiles_of_m56(lh, oracle):
    """(200, 56, 64): one flipped recovery bit in the first and the last row of every row tile
    (rows 0, 3, ..., 52, 55), one stripe each, among clean stripes."""
    k, m, nbytes = 200, 56, 64
    rows = lhverify.tile_rows(m)
    assert rows[-1] == 55 and len(rows) == 28
    data, rec0 = lhverify.encoded(oracle, k, m, nbytes, 2 * len(rows), 20056)
    rec = rec0.copy()
    pos = lhverify.positions(k, m, nbytes, 3)
    for i, r in enumerate(rows):
        rec[2 * i, r, pos[i % len(pos)]] ^= np.uint8(1 << (i % 8))
    status, bad = lhverify.expected(oracle, k, m, nbytes, data, rec)
    assert [np.nonzero(bad[2 * i])[0].tolist() for i in range(len(rows))] == [[r] for r in rows] and int(bad.sum()) == len(rows)
    assert run_strided(lh, k, m, nbytes, data, rec, status, bad, (1, 3)) == TRACE


# ------------------------------------------------------------------ batch sizes
COUNTS = [("packed-small-blocks", 29, 4, 64), ("wider-than-a-wave", 29, 4, 4104)]


def _t_verify(lh, k, m, nbytes):
    return lhverify.stripes_per_workgroup(k, m, nbytes)


@pytest.mark.parametrize("name,k,m,nbytes", COUNTS, ids=[c[0] for c in COUNTS])
def test_verify_counts(lh, oracle, name, k, m, nbytes):
    """Every prefix length lhutil.stripe_counts(T) of one mixed batch (T stripes per workgroup: 256
    one-lane stripes; 3 stripes of 65 lanes): stripes < n get their expected bytes, every status
    and bad_rows byte from stripe n on keeps its canary (the sizes of the clearing copies and the grid)."""
    import torch
    T = _t_verify(lh, k, m, nbytes)
    assert T == (256 if nbytes == 64 else 3)
    counts = lhutil.stripe_counts(T)
    N = counts[-1] + 1
    data, rec, status, bad, plan = _mixed(oracle, k, m, nbytes, N)
    assert status[:1].tolist() == [0] and status[1:5].all()
    S, gs = tsc._strided("status", np.full((N, 1), C_STATUS, dtype=np.uint8), status.view(np.uint8).reshape(N, 1), C_STATUS, 1)
    B, gb = tsc._strided("bad_rows", np.full((N, m), C_ROWS, dtype=np.uint8), bad, C_ROWS, 1)
    d_data, d_rec = (torch.from_numpy(np.array(a)).cuda() for a in (data, rec))
    lib = lh.lib()
    vp, ll = ctypes.c_void_p, ctypes.c_longlong

    def call(n):
        rc = lib.cauchy_256_verify_batch(k, m, nbytes, n, vp(d_data.data_ptr()), ll(k * nbytes), vp(d_rec.data_ptr()),
                                         ll(m * nbytes), vp(gs.ptr), vp(gb.ptr), _stream())
        assert rc == 0, (name, n, rc, lib.cauchy_256_last_error())
    case = tsc._case("verify-" + name, k, m, nbytes, {}, _t_verify, TRACE)
    failing, traces, calls, seconds, ran = tsc.sweep(lh, case, counts, [S, B], call)
    assert calls == len(counts) and sorted(ran) == counts
    assert traces[counts[-1]] == TRACE and traces[1] == TRACE
    if failing:
        pytest.fail(tsc._report(case, T, counts, failing, ran, [S, B], call), pytrace=False)
    assert torch.equal(d_data.cpu(), torch.from_numpy(np.array(data))) and torch.equal(d_rec.cpu(), torch.from_numpy(np.array(rec)))


# ------------------------------------------------------------------ pointer tables
PTRS = [(29, 4, 1304), (29, 4, 56), (200, 56, 64), (5, 1, 13), (1, 3, 16)]


@pytest.mark.parametrize("k,m,nbytes", PTRS, ids=_ids(PTRS))
def test_pointer_tables(lh, oracle, k, m, nbytes):
    """Every data and recovery block at a random place and byte offset of a pool: the same
    answers, the pointer-table kernel, the pools unchanged."""
    import torch
    S = 40
    data, rec, status, bad, plan = _mixed(oracle, k, m, nbytes)
    dpool, dptrs, dplace = tp._scatter(torch.from_numpy(np.array(data)).cuda(), 21)
    rpool, rptrs, rplace = tp._scatter(torch.from_numpy(np.array(rec)).cuda(), 22)
    assert int((dptrs % 2).sum()) > 0 and int((rptrs % 2).sum()) > 0   # odd addresses among them
    before = [t.clone() for t in (dpool, rpool, dptrs, rptrs)]
    d_status = torch.full((S,), C_STATUS, dtype=torch.int8, device="cuda")
    d_bad = torch.full((S, m), C_ROWS, dtype=torch.uint8, device="cuda")
    got = lh.verify_batch_ptrs(k, m, nbytes, dptrs, rptrs, status=d_status, bad_rows=d_bad)
    assert lh.last_launch() == TRACE_PTR
    torch.cuda.synchronize()
    assert got is d_status and d_status.cpu().numpy().tolist() == status.tolist()
    assert np.array_equal(d_bad.cpu().numpy(), bad)
    for t, b in zip((dpool, rpool, dptrs, rptrs), before):
        assert torch.equal(t, b), "a pool or a table was written"
    tp._gaps_untouched(dpool, dplace)
    tp._gaps_untouched(rpool, rplace)
    assert np.array_equal(tp._gather(dpool, dplace).cpu().numpy(), data)


# ------------------------------------------------------------------ the product's own encoder
def test_encode_update_verify(lh):
    """k29/m4/1296, 24 stripes, through the wrappers: what encode_batch wrote verifies clean;
    after update_batch of two blocks per stripe with the data patched likewise still clean; data
    patched without the update: every patched stripe bad in all rows."""
    import torch
    k, m, nbytes, S = 29, 4, 1296, 24
    rng = np.random.Generator(np.random.PCG64(2906))
    d_data = torch.from_numpy(lhutil.fill(2906, S * k * nbytes).reshape(S, k, nbytes)).cuda()
    rec = lh.encode_batch(d_data, m)
    assert lh.last_launch() == ["lh_jit_encode"]
    bad = torch.full((S, m), C_ROWS, dtype=torch.uint8, device="cuda")
    status = lh.verify_batch(d_data, rec, bad_rows=bad)
    assert lh.last_launch() == TRACE
    assert status.dtype == torch.int8 and tuple(status.shape) == (S,)
    assert int((status != 0).sum()) == 0 and int((bad != 0).sum()) == 0
    cols = np.stack([np.sort(rng.choice(k, size=2, replace=False)) for _ in range(S)]).astype(np.uint8)
    d_cols = torch.from_numpy(cols).cuda()
    idx = d_cols.long()[:, :, None].expand(S, 2, nbytes)
    d_old = torch.gather(d_data, 1, idx).contiguous()
    d_new = torch.from_numpy(lhutil.fill(2907, S * 2 * nbytes).reshape(S, 2, nbytes)).cuda()
    assert int((lh.update_batch(k, rec, d_cols, d_old, d_new) != 0).sum()) == 0
    patched = d_data.clone()
    patched.scatter_(1, idx, d_new)
    status = lh.verify_batch(patched, rec, bad_rows=bad)
    assert int((status != 0).sum()) == 0 and int((bad != 0).sum()) == 0
    # the update skipped for the odd stripes: their old recovery against the patched data
    stale = lh.encode_batch(d_data, m)
    mixed = torch.where((torch.arange(S, device="cuda") % 2 == 1)[:, None, None], stale, rec)
    status = lh.verify_batch(patched, mixed, bad_rows=bad)
    torch.cuda.synchronize()
    odd = (np.arange(S) % 2 == 1)
    assert status.cpu().numpy().tolist() == odd.astype(np.int8).tolist()
    assert np.array_equal(bad.cpu().numpy(), np.repeat(odd.astype(np.uint8)[:, None], m, axis=1))


# ------------------------------------------------------------------ hipGraph
def test_verify_captures_in_a_graph(lh, oracle):
    """On a prepared stream one verify captures without running (the canaries stay); replays
    give zeros on clean data, flag a byte flipped on the device, and clear the flag again once
    the byte is restored: the zeroing of the outputs is part of the graph."""
    import torch
    k, m, nbytes, S = 29, 4, 1296, 24
    data, rec = lhverify.encoded(oracle, k, m, nbytes, S, 79)
    d_data, d_rec = (torch.from_numpy(np.array(a)).cuda() for a in (data, rec))
    status = torch.full((S,), C_STATUS, dtype=torch.int8, device="cuda")
    bad = torch.full((S, m), C_ROWS, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    lh.prepare(k, m, nbytes, S, stream=s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        lh.verify_batch(d_data, d_rec, status=status, bad_rows=bad, stream=s)
        assert lh.last_launch() == TRACE
    torch.cuda.synchronize()
    assert int((status != C_STATUS).sum()) == 0 and int((bad != C_ROWS).sum()) == 0   # capture runs nothing
    graph.replay()
    torch.cuda.synchronize()
    assert int((status != 0).sum()) == 0 and int((bad != 0).sum()) == 0
    d_rec[17, 2, 1295] ^= 0x10
    graph.replay()
    torch.cuda.synchronize()
    exp_status, exp_bad = np.zeros(S, dtype=np.int8), np.zeros((S, m), dtype=np.uint8)
    exp_status[17], exp_bad[17, 2] = 1, 1
    assert status.cpu().numpy().tolist() == exp_status.tolist() and np.array_equal(bad.cpu().numpy(), exp_bad)
    d_rec[17, 2, 1295] ^= 0x10
    graph.replay()
    torch.cuda.synchronize()
    assert int((status != 0).sum()) == 0 and int((bad != 0).sum()) == 0   # the stale 1 is cleared
    assert np.array_equal(d_rec.cpu().numpy(), rec) and np.array_equal(d_data.cpu().numpy(), data)
