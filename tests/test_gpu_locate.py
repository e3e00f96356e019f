"""cauchy_256_locate_batch / _ptrs on the GPU (include/cauchy_256_locate.h; lh_locate_kernel and
lh_locate_finish_kernel in kernels.hip): which block of a bad stripe is the corrupt one?

The expectation is the plant and lhlocate.model_locate (the header's contract in numpy, pinned to
the C oracle by tests/test_locate_model.py), never the library.  Inputs sit between canary guards
and are compared after the call; outputs sit between guards too, and their canaries are no value a
status or a row can take, so an unwritten byte shows.  Covered: every lane form (one flipped bit
per stripe at every position class, in every data and recovery block); every row tile; mixed
batches with the batch size swept over the workgroup tile; lanes of one stripe that disagree, in
one wave and across workgroups; pointer tables; scrub, locate and heal with the product's own
encoder and repair; the launch trace; hipGraph capture.  `-m gpu`: needs an MI355X."""
import ctypes
import functools

import numpy as np
import pytest

import lhlocate
import lhutil
import lhverify
import test_gpu_ptrs as tp
import test_gpu_stripe_counts as tsc
import test_gpu_untouched as tu
from test_gpu_untouched import C_BLOCKS, C_STATUS

pytestmark = pytest.mark.gpu

TRACE = ["lh_verify_kernel", "lh_locate_kernel", "lh_locate_finish_kernel"]
TRACE_PTR = ["lh_verify_kernel(pointer table)", "lh_locate_kernel(pointer table)", "lh_locate_finish_kernel"]
TRACE_M1 = ["lh_verify_kernel", "lh_locate_finish_kernel"]                    # m == 1: nothing to search
TRACE_M1_PTR = ["lh_verify_kernel(pointer table)", "lh_locate_finish_kernel"]
C_ROWS = 0x5E   # canary of rows; with C_STATUS (0x77) neither 0, 1, 2 nor 0xFF
# sub-blocks of 1, 3, 5, 7 (under a lane), 8 (one lane) and 17 bytes (a lane and a 1-byte tail)
BYTES = [(29, 4, b) for b in (8, 24, 40, 56, 64, 136)]
FLAT = [(5, 1, 13), (1, 3, 16), (1, 3, 13)]


def _ids(shapes):
    return [f"k{k}m{m}b{b}" for k, m, b in shapes]


def _trace(m, table=False):
    return (TRACE_M1_PTR if table else TRACE_M1) if m == 1 else (TRACE_PTR if table else TRACE)


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


def _compare(tag, got_status, got_rows, exp_status, exp_rows):
    wrong = np.nonzero((got_status.view(np.int8) != exp_status) | (got_rows != exp_rows))[0]
    assert wrong.size == 0, (tag, "stripes", wrong.tolist()[:8], "got (status, row)",
                             list(zip(got_status[wrong][:8].tolist(), got_rows[wrong][:8].tolist())), "expected",
                             list(zip(exp_status[wrong][:8].tolist(), exp_rows[wrong][:8].tolist())))


def run_strided(lh, k, m, nbytes, data, rec, exp_status, exp_rows, layout=(0, 0)):
    """The C call on guarded buffers: data, recovery, status and rows each between 256-byte guards,
    `layout` = (odd base offset, pad bytes between stripes).  Asserts the expectation, every guard
    and pad, and that data and recovery are bit-identical afterwards.  Returns the launch trace."""
    import torch
    S = data.shape[0]
    off, pad = layout
    gd = tu.Guarded(data.reshape(S, k * nbytes), off, pad, C_BLOCKS)
    gr = tu.Guarded(rec.reshape(S, m * nbytes), off + 2 if off else 0, pad, C_BLOCKS)
    gs = tu.Guarded(np.full((1, S), C_STATUS, dtype=np.uint8), 1 if off else 0, 0, C_STATUS)
    gw = tu.Guarded(np.full((1, S), C_ROWS, dtype=np.uint8), 3 if off else 0, 0, C_ROWS)
    before = [g.buf.clone() for g in (gd, gr)]
    torch.cuda.synchronize()
    rc = lh.lib().cauchy_256_locate_batch(k, m, nbytes, S, ctypes.c_void_p(gd.ptr), ctypes.c_longlong(gd.stride),
                                          ctypes.c_void_p(gr.ptr), ctypes.c_longlong(gr.stride),
                                          ctypes.c_void_p(gs.ptr), ctypes.c_void_p(gw.ptr), _stream())
    assert rc == 0, (rc, lh.lib().cauchy_256_last_error())
    trace = lh.last_launch()
    torch.cuda.synchronize()
    tag = (k, m, nbytes, S, layout)
    _compare(tag, gs.check((tag, "status")).reshape(S), gw.check((tag, "rows")).reshape(S), exp_status, exp_rows)
    for g, b, what in zip((gd, gr), before, ("data", "recovery")):
        assert torch.equal(g.buf, b), (tag, what, "written")
    return trace


# ------------------------------------------------------------------ lane forms
@pytest.mark.parametrize("k,m,nbytes", BYTES + FLAT, ids=_ids(BYTES + FLAT))
def test_one_bit_anywhere_is_located(lh, oracle, k, m, nbytes):
    """One stripe per (byte position of lhverify.positions, block of the stored word), one bit
    flipped there: the block is named, data blocks and recovery blocks, recovery 0 among them
    (m == 1: status 2, no row).  The clean batch first."""
    data, rec, status, rows = lhlocate.bit_sweep(oracle, k, m, nbytes, k * 1000 + m * 10 + nbytes)
    S = data.shape[0]
    pick = list(range(0, S, max(1, S // 12)))   # the plants' answers are the model's (a sample here; CPU: test_locate_model)
    got = lhlocate.expected(oracle, k, m, nbytes, data[pick], rec[pick])
    assert got[0].tolist() == status[pick].tolist() and got[1].tolist() == rows[pick].tolist()
    clean = lhverify.encoded(oracle, k, m, nbytes, S, k * 1000 + m * 10 + nbytes)
    assert run_strided(lh, k, m, nbytes, clean[0], clean[1], np.zeros(S, dtype=np.int8),
                       np.full(S, 0xFF, dtype=np.uint8)) == _trace(m)
    assert run_strided(lh, k, m, nbytes, data, rec, status, rows) == _trace(m)


# ------------------------------------------------------------------ row tiles
TILES = [(10, 2, 24), (10, 4, 24), (10, 5, 24), (10, 9, 24), (200, 55, 64)]


@functools.lru_cache(maxsize=None)
def _tiles_case(oracle, k, m, nbytes):
    last = lhverify.tile_rows(m)[-1]                      # a row of the last row tile
    cols = sorted({0, k // 3, k - 1})
    S = 2 * len(cols) + 1
    data0, rec0 = lhverify.encoded(oracle, k, m, nbytes, S, k * 1000 + m * 10 + nbytes + 2)
    data, rec = data0.copy(), rec0.copy()
    pos = lhverify.positions(k, m, nbytes, 4)
    status, rows = np.zeros(S, dtype=np.int8), np.full(S, 0xFF, dtype=np.uint8)
    for i, x in enumerate(cols):
        p = pos[(3 * i + 1) % len(pos)]
        for s in (1 + 2 * i, 2 + 2 * i):
            lhlocate.plant_byte(data, rec, s, x, p, i)
        status[1 + 2 * i], rows[1 + 2 * i] = 1, x         # the data plant alone: survives every tile's check
        lhlocate.plant_bit(data, rec, 2 + 2 * i, k + last, lhlocate.other_offset(k, m, nbytes, p, i), i)
        status[2 + 2 * i] = 2                             # and a row of the last tile that does not fit it
    rws = oracle.cauchy_rows(k, m)
    for s in range(S):
        assert lhlocate.model_locate(k, m, nbytes, data[s], rec[s], rws) == (status[s], rows[s]), s
    return data, rec, status, rows


@pytest.mark.parametrize("k,m,nbytes", TILES, ids=_ids(TILES))
def test_every_row_tile_is_checked(lh, oracle, k, m, nbytes):
    """A corrupt data block is named only after the rows of every tile fit its column: alone it is
    located; with one more bit, at another offset, in a recovery row of the last tile, the answer
    is 2 (m 2, 4: one tile; 5: a tile and one row; 9 and 55: several)."""
    assert run_strided(lh, k, m, nbytes, *_tiles_case(oracle, k, m, nbytes), layout=(1, 3)) == TRACE


# ------------------------------------------------------------------ mixed batches, every batch size
MIXED = [(29, 4, 1296), (29, 4, 1304), (4, 2, 16), (10, 13, 24), (29, 4, 64)]


@functools.lru_cache(maxsize=None)
def _mixed(oracle, k, m, nbytes, stripes=40):
    check = 40 if k < 100 else 8   # (the model costs ~k m numpy operations a stripe: one cycle of the styles)
    return lhlocate.mixed_case(oracle, k, m, nbytes, stripes, k * 1000 + m * 10 + nbytes + 1, check=check)


@pytest.mark.parametrize("k,m,nbytes", MIXED, ids=_ids(MIXED))
def test_mixed_batch_between_guards(lh, oracle, k, m, nbytes):
    """40 stripes, the styles cycling (clean, data bit, data block replaced, recovery byte, recovery
    0 byte, two recovery rows, two data blocks at different offsets, a data and a recovery block),
    from an odd base with pad bytes between stripes.  At 16, 24 and 64-byte blocks a wave holds 64
    stripes with different answers."""
    data, rec, status, rows, plan = _mixed(oracle, k, m, nbytes)
    assert set(status.tolist()) == {0, 1, 2} and {s for s, _ in plan} == set(lhlocate.STYLES)
    assert run_strided(lh, k, m, nbytes, data, rec, status, rows, (3, 5)) == TRACE


@pytest.mark.parametrize("k,m,nbytes", MIXED[:4], ids=_ids(MIXED[:4]))
def test_locate_counts(lh, oracle, k, m, nbytes):
    """Every prefix length lhutil.stripe_counts(T) of one mixed batch (T the stripes per workgroup
    of the scrub's lanes): stripes < n get their expected bytes, every status and rows byte from
    stripe n on keeps its canary (the sizes of the clearing copies and of the three grids)."""
    import torch
    T = lhverify.stripes_per_workgroup(k, m, nbytes)
    assert T == {1296: 12, 1304: 12, 16: 256, 24: 256}[nbytes]
    counts = lhutil.stripe_counts(T)
    N = counts[-1] + 1
    data, rec, status, rows, plan = _mixed(oracle, k, m, nbytes, N)
    S, gs = tsc._strided("status", np.full((N, 1), C_STATUS, dtype=np.uint8), status.view(np.uint8).reshape(N, 1), C_STATUS, 1)
    W, gw = tsc._strided("rows", np.full((N, 1), C_ROWS, dtype=np.uint8), rows.reshape(N, 1), C_ROWS, 1)
    d_data, d_rec = (torch.from_numpy(np.array(a)).cuda() for a in (data, rec))
    lib = lh.lib()
    vp, ll = ctypes.c_void_p, ctypes.c_longlong

    def call(n):
        rc = lib.cauchy_256_locate_batch(k, m, nbytes, n, vp(d_data.data_ptr()), ll(k * nbytes), vp(d_rec.data_ptr()),
                                         ll(m * nbytes), vp(gs.ptr), vp(gw.ptr), _stream())
        assert rc == 0, (n, rc, lib.cauchy_256_last_error())
    case = tsc._case(f"locate-k{k}m{m}b{nbytes}", k, m, nbytes, {}, lambda *a: T, TRACE)
    failing, traces, calls, seconds, ran = tsc.sweep(lh, case, counts, [S, W], call)
    assert calls == len(counts) and sorted(ran) == counts
    assert traces[counts[-1]] == TRACE and traces[1] == TRACE
    if failing:
        pytest.fail(tsc._report(case, T, counts, failing, ran, [S, W], call), pytrace=False)
    assert torch.equal(d_data.cpu(), torch.from_numpy(np.array(data))) and torch.equal(d_rec.cpu(), torch.from_numpy(np.array(rec)))


# ------------------------------------------------------------------ lanes that disagree
DISAGREE = [(5, 3, 128, 0, 1), (3, 2, 16448, 0, 256)]   # both lanes in one wave; in two workgroups of one stripe


@functools.lru_cache(maxsize=None)
def _disagree_case(oracle, k, m, nbytes, la, lb):
    assert lhverify.geometry(k, m, nbytes)[3] > lb and (lb // 256 > 0) == (nbytes == 16448)
    a, b = lhlocate.lane_bytes(k, m, nbytes, la), lhlocate.lane_bytes(k, m, nbytes, lb)
    sub = nbytes // 8
    plants = []   # (x, byte in lane la or None, y, byte in lane lb)
    for x in range(k):
        y = (x + 1) % k
        plants += [(x, a[x % len(a)], y, b[-1 - x % len(b)] + 3 * sub), (y, a[-1] + 7 * sub, x, b[0]),   # x != y: 2
                   (x, a[0] + sub, x, b[-1] + 2 * sub),                                                # x == y: row x
                   (None, None, x, b[x % len(b)] + (x % 8) * sub)]                                      # the far lane alone
    S = 2 * len(plants) + 1
    data0, rec0 = lhverify.encoded(oracle, k, m, nbytes, S, 5 + nbytes)
    data, rec = data0.copy(), rec0.copy()
    status, rows = np.zeros(S, dtype=np.int8), np.full(S, 0xFF, dtype=np.uint8)
    for i, (x, p, y, q) in enumerate(plants):
        s = 1 + 2 * i
        if x is not None:
            lhlocate.plant_byte(data, rec, s, x, p, i)
        lhlocate.plant_byte(data, rec, s, y, q, i + 1)
        status[s], rows[s] = (1, y) if x in (None, y) else (2, 0xFF)
    exp = lhlocate.expected(oracle, k, m, nbytes, data, rec)
    assert exp[0].tolist() == status.tolist() and exp[1].tolist() == rows.tolist()
    assert sorted(set(status.tolist())) == [0, 1, 2]
    return data, rec, status, rows


@pytest.mark.parametrize("k,m,nbytes,la,lb", DISAGREE, ids=["one-wave", "two-workgroups"])
def test_lanes_that_disagree(lh, oracle, k, m, nbytes, la, lb):
    """Data block x corrupt only in bytes lane `la` reads, data block y only in bytes lane `lb`
    reads: each lane alone finds a consistent column, the stripe has none (2).  With x == y the
    two lanes agree and the block is named; so is a block corrupt in the far lane alone.  The
    stripes in between are clean."""
    assert run_strided(lh, k, m, nbytes, *_disagree_case(oracle, k, m, nbytes, la, lb), layout=(1, 3)) == TRACE


# ------------------------------------------------------------------ pointer tables
PTRS = [(29, 4, 1304), (29, 4, 56), (200, 55, 64), (5, 1, 13), (1, 3, 16)]


@pytest.mark.parametrize("k,m,nbytes", PTRS, ids=_ids(PTRS))
def test_pointer_tables(lh, oracle, k, m, nbytes):
    """Every data and recovery block at a random place and byte offset of a pool: the same
    answers, the pointer-table kernels, the pools unchanged."""
    import torch
    S = 40
    data, rec, status, rows, plan = _mixed(oracle, k, m, nbytes)
    dpool, dptrs, dplace = tp._scatter(torch.from_numpy(np.array(data)).cuda(), 21)
    rpool, rptrs, rplace = tp._scatter(torch.from_numpy(np.array(rec)).cuda(), 22)
    assert int((dptrs % 2).sum()) > 0 and int((rptrs % 2).sum()) > 0   # odd addresses among them
    before = [t.clone() for t in (dpool, rpool, dptrs, rptrs)]
    d_status = torch.full((S,), C_STATUS, dtype=torch.int8, device="cuda")
    d_rows = torch.full((S,), C_ROWS, dtype=torch.uint8, device="cuda")
    got = lh.locate_batch_ptrs(k, m, nbytes, dptrs, rptrs, status=d_status, rows=d_rows)
    assert lh.last_launch() == _trace(m, table=True)
    torch.cuda.synchronize()
    assert got[0] is d_status and got[1] is d_rows
    _compare((k, m, nbytes, "table"), d_status.cpu().numpy().view(np.uint8), d_rows.cpu().numpy(), status, rows)
    for t, b in zip((dpool, rpool, dptrs, rptrs), before):
        assert torch.equal(t, b), "a pool or a table was written"
    tp._gaps_untouched(dpool, dplace)
    tp._gaps_untouched(rpool, rplace)


# ------------------------------------------------------------------ scrub, locate, heal
def test_scrub_locate_heal(lh):
    """k29/m4/1296, 24 stripes through the wrappers: encode_batch; one corrupt block, data or
    recovery, in every third stripe; verify_batch flags those stripes and locate_batch names the
    blocks; reconstruct_batch_ptrs, with the first k rows other than the located one as survivors,
    rows.unsqueeze(1) as want_rows and the out pointer at the corrupt block itself, heals them."""
    import torch
    k, m, nbytes, S = 29, 4, 1296, 24
    d_data = torch.from_numpy(lhutil.fill(2911, S * k * nbytes).reshape(S, k, nbytes)).cuda()
    rec = lh.encode_batch(d_data, m)
    orig_data, orig_rec = d_data.clone(), rec.clone()
    blocks = {s: (7 * s + 3) % (k + m) for s in range(0, S, 3)}
    blocks[3], blocks[6] = k, k + m - 1   # recovery 0 and the last recovery row among them
    for s, x in blocks.items():
        t = d_data[s, x] if x < k else rec[s, x - k]
        if s % 2:
            t[(13 * s) % nbytes] ^= 1 << (s % 8)
        else:
            t.copy_(torch.from_numpy(lhutil.fill(s, nbytes)).cuda())
    exp_status = np.array([1 if s in blocks else 0 for s in range(S)], dtype=np.int8)
    exp_rows = np.array([blocks.get(s, 0xFF) for s in range(S)], dtype=np.uint8)
    assert lh.verify_batch(d_data, rec).cpu().numpy().tolist() == exp_status.tolist()
    status, rows = lh.locate_batch(d_data, rec)
    assert lh.last_launch() == TRACE
    assert status.dtype == torch.int8 and rows.dtype == torch.uint8 and tuple(status.shape) == tuple(rows.shape) == (S,)
    _compare("heal", status.cpu().numpy().view(np.uint8), rows.cpu().numpy(), exp_status, exp_rows)
    located = rows.cpu().numpy()
    surv = np.array([[x for x in range(k + m) if x != located[s]][:k] for s in range(S)], dtype=np.uint8)
    addr = lambda s, x: (d_data.data_ptr() + (s * k + x) * nbytes) if x < k else (rec.data_ptr() + (s * m + x - k) * nbytes)   # noqa: E731
    block_ptrs = torch.tensor([[addr(s, int(x)) for x in surv[s]] for s in range(S)], dtype=torch.int64, device="cuda")
    out_ptrs = torch.tensor([[addr(s, int(located[s])) if located[s] != 0xFF else 0] for s in range(S)],
                            dtype=torch.int64, device="cuda")
    st = lh.reconstruct_batch_ptrs(k, m, nbytes, block_ptrs, torch.from_numpy(surv).cuda(), rows.unsqueeze(1), out_ptrs)
    assert int((st != 0).sum()) == 0
    assert torch.equal(d_data, orig_data) and torch.equal(rec, orig_rec)
    assert int((lh.verify_batch(d_data, rec) != 0).sum()) == 0
    status, rows = lh.locate_batch(d_data, rec)
    assert int((status != 0).sum()) == 0 and int((rows != 0xFF).sum()) == 0


# ------------------------------------------------------------------ the launch trace
def test_launch_trace(lh, oracle):
    """cauchy_256_last_launch after the strided, the table and the flat forms, as the header says."""
    import torch
    for k, m, nbytes in ((4, 2, 16), (1, 3, 13), (5, 1, 13)):
        data, rec = (torch.from_numpy(np.array(a)).cuda() for a in lhverify.encoded(oracle, k, m, nbytes, 5, 77))
        status, rows = lh.locate_batch(data, rec)
        assert lh.last_launch() == _trace(m)
        dpool, dptrs, _ = tp._scatter(data, 1)
        rpool, rptrs, _ = tp._scatter(rec, 2)
        status2, rows2 = lh.locate_batch_ptrs(k, m, nbytes, dptrs, rptrs)
        assert lh.last_launch() == _trace(m, table=True)
        for t in (status, status2):
            assert t.cpu().numpy().tolist() == [0] * 5
        for t in (rows, rows2):
            assert t.cpu().numpy().tolist() == [0xFF] * 5
    header = open(lhutil.REPO + "/include/cauchy_256_locate.h").read()
    assert "lh_verify_kernel; lh_locate_kernel; lh_locate_finish_kernel" in header
    assert "lh_verify_kernel; lh_locate_finish_kernel" in header and '"(pointer table)"' in header


# ------------------------------------------------------------------ hipGraph
def test_locate_captures_in_a_graph(lh, oracle):
    """After an uncaptured call of the same size on the stream, one locate captures without running
    (the canaries stay); replays follow the bytes on the device: clean, a data block, then another
    stripe's recovery block, then clean again.  A captured call of a larger batch than was
    prepared returns -3 and enqueues nothing."""
    import torch
    k, m, nbytes, S = 29, 4, 1296, 24
    data, rec = lhverify.encoded(oracle, k, m, nbytes, 16 * S, 81)
    d_data, d_rec = (torch.from_numpy(np.array(a)).cuda() for a in (data, rec))
    status = torch.full((16 * S,), C_STATUS, dtype=torch.int8, device="cuda")
    rows = torch.full((16 * S,), C_ROWS, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    lh.locate_batch(d_data[:S], d_rec[:S], status=status[:S], rows=rows[:S], stream=s)   # provides generator, zero page, workspace
    s.synchronize()
    assert int((status[:S] != 0).sum()) == 0 and int((rows[:S] != 0xFF).sum()) == 0
    status.fill_(C_STATUS)
    rows.fill_(C_ROWS)
    torch.cuda.synchronize()
    lib, vp, ll = lh.lib(), ctypes.c_void_p, ctypes.c_longlong
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        lh.locate_batch(d_data[:S], d_rec[:S], status=status[:S], rows=rows[:S], stream=s)
        assert lh.last_launch() == TRACE
        rc = lib.cauchy_256_locate_batch(k, m, nbytes, 16 * S, vp(d_data.data_ptr()), ll(k * nbytes), vp(d_rec.data_ptr()),
                                         ll(m * nbytes), vp(status.data_ptr()), vp(rows.data_ptr()), vp(s.cuda_stream))
        assert rc == -3 and lh.last_launch() == [] and b"captured" in lib.cauchy_256_last_error()
    torch.cuda.synchronize()
    assert int((status != C_STATUS).sum()) == 0 and int((rows != C_ROWS).sum()) == 0   # capture runs nothing

    def replay(exp):
        graph.replay()
        torch.cuda.synchronize()
        es, er = np.zeros(S, dtype=np.int8), np.full(S, 0xFF, dtype=np.uint8)
        for at, (st, row) in exp.items():
            es[at], er[at] = st, row
        _compare(("graph", sorted(exp)), status[:S].cpu().numpy().view(np.uint8), rows[:S].cpu().numpy(), es, er)
        assert int((status[S:] != C_STATUS).sum()) == 0 and int((rows[S:] != C_ROWS).sum()) == 0
    replay({})
    d_data[17, 5, 1295] ^= 0x10
    replay({17: (1, 5)})
    d_rec[3, 2, 0] ^= 0x01
    replay({17: (1, 5), 3: (1, k + 2)})
    d_data[17, 6, 7] ^= 0x80          # a second data block of stripe 17, at another offset
    replay({17: (2, 0xFF), 3: (1, k + 2)})
    d_data[17, 5, 1295] ^= 0x10
    d_data[17, 6, 7] ^= 0x80
    d_rec[3, 2, 0] ^= 0x01
    replay({})                        # the stale answers are cleared
    assert np.array_equal(d_rec.cpu().numpy(), rec) and np.array_equal(d_data.cpu().numpy(), data)
