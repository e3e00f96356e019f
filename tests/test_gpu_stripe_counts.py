"""The batch size swept over every kernel's workgroup tile.

Every kernel maps stripes onto lanes, waves and workgroups in its own way -- up to 64 whole
stripes per wave with a partial last wave, four-wave workgroups whose last one has idle waves,
the XCD renumbering of the workgroups from 8 up, 64 / nch or 256 / nch stripes per workgroup of
the generic kernels, 256 per workgroup of the small planner, the one 1024-thread workgroup of
lh_order_kernel -- and an off-by-one there either drops the last stripes or writes past stripe n.
A stripe's result does not depend on the size of its batch, so one batch is prepared per case on
the CPU (the C oracle; test_gpu_untouched._encoded / mixed_case) and every prefix length n of it
has a known answer: stripes < n the oracle's, every byte from stripe n on -- the other stripes,
the pads, the guards -- what it was before the call.

Per case the counts are lhutil.stripe_counts(T) for the T stripes one workgroup of the case's
subject kernel covers (tests/test_lhutil_counts.py), run in a seeded shuffled order on one stream
(a small batch follows a large one and sees its plan and `order` workspace).  One stripe more
than the largest count is prepared, so "untouched from stripe n on" always has a stripe to look
at.  T comes from the library for the specialised kernels (cauchy_256_batch_path what = 10 / 11)
and from the launch arithmetic in kernels.hip for the others (the _t_* functions below).  Each
buffer is compared on the device with its expected image (one reduction per buffer and count,
the flags read once at the end); a failure names the failing counts and, for the smallest, the
first wrong byte.  The launch trace is asserted at the largest count and at n = 1.  Everything is
byte for byte.  `-m gpu`: needs an MI355X; every module is compiled at build time
(tools/precompile.py STRIPE_COUNT_JOBS and the older lists)."""
import collections
import ctypes
import time

import numpy as np
import pytest

import lhutil
import test_gpu_ptrs as tp
import test_gpu_untouched as tu
from test_gpu_boundaries import (FUSED, GEN, GENERIC_CF, GENERIC_S8, JIT_SAMPLE, JUMP, JUMP2, OLD_CF, PS4_JUMP, PS4_JUMP2,
                                 SMALL4, SMALL8, WIDE16)
from test_gpu_untouched import C_BLOCKS, C_ROWS, C_STATUS, FAMILY, FUSED_FAMILY, GUARD

pytestmark = pytest.mark.gpu

OUTSIDE = 1 << 30   # "stripe" of a byte outside every stripe (guards, pads, pool gaps): never written
ORDER_EXTRA = (1023, 1024, 1025, 2047, 2048, 2049)
# lh_plan_kernel with e_max > 8 runs four waves per stripe up to 4096 stripes, one above
# (kernels.hip launch_plan: `a.stripes <= 4096 && a.e_max > 8`)
PLAN_EXTRA = (4095, 4096, 4097)
PTR = "(pointer table)"
GATHER, SCATTER = "lh_ptr_copy_kernel(gather)", "lh_ptr_copy_kernel(scatter)"


# ------------------------------------------------------------------ T, per kernel
def _t_lib(decode):
    """The specialised kernels: the library's own figure (codec.cpp jit_encode_blocks / jit_blocks)."""
    def tile(lh, k, m, nbytes):
        t = lh.stripes_per_workgroup(k, m, nbytes, decode)
        assert t >= 1, ("no specialised configuration", k, m, nbytes)
        return t
    return tile


def _t_one(lh, k, m, nbytes):
    """One stripe or less per workgroup: the in-place jump apply (kernels.hip launch_apply_jump,
    per_stripe: wgs = stripes * wps), lh_plan_kernel (launch_plan: dim3(stripes)), phase B
    (launch_inverse: wgs = stripes * ...) and the windowed kernels (codec.cpp
    launch_jit_encode_win / launch_jit_decode_wide: blocks = stripes * (sub / (64 W)))."""
    return 1


def _t_flat_jump(lh, k, m, nbytes):
    """kernels.hip launch_apply_jump, flat: wgs = ceil(stripes * nch / 64), nch the dword or
    two-dword lanes of a sub-block (codec.cpp jump_layout)."""
    nch = -(-(nbytes // 8) // (4 * lh.jump_lanes(k, m, nbytes)))
    return max(1, 64 // nch)


def _t_bytewise(lh, k, m, nbytes):
    """kernels.hip launch_apply_generic: grid.x = ceil(stripes * nch / 256), nch = ceil(sub / W)
    with W = 4, 2 or 1 bytes (codec.cpp generic_word)."""
    sub = nbytes // 8
    w = 4 if sub >= 4 else 2 if sub >= 2 else 1
    return max(1, 256 // -(-sub // w))


def _t_xor(lh, k, m, nbytes):
    """kernels.hip launch_xor_reduce: ceil(stripes * nch / 256) workgroups, nch = ceil(bytes / 16)
    (codec.cpp xor_rows)."""
    return max(1, 256 // -(-nbytes // 16))


def _t_scatter(lh, k, m, nbytes):
    """kernels.hip launch_scatter: ceil(stripes * e_max * ceil(bytes / 16) / 256) workgroups."""
    return max(1, 256 // (min(k, m) * -(-nbytes // 16)))


def _t_plan_small(lh, k, m, nbytes):
    """kernels.hip launch_plan: blocks = ceil(stripes / 256) of lh_plan_small_kernel."""
    return 256


def _t_order(lh, k, m, nbytes):
    """kernels.hip order_stripes: one workgroup, dim3(1024), strides over the batch."""
    return 1024


Case = collections.namedtuple("Case", "id k m nbytes env form tile trace trace1 extra also mode")


def _case(id, k, m, nbytes, env, tile, trace, form="strided", trace1=None, extra=(), also=(), mode="quarter"):
    return Case(id, k, m, nbytes, env, form, tile, trace, trace1 or trace, extra, also, mode)


def _ptr(names):
    return [n + PTR for n in names]


CF_ONE = ["lh_plan_kernel(closed form)", "lh_apply_jump_kernel"]   # one stripe: nothing to order
WIDE_ONE = ["lh_plan_kernel(closed form)", "lh_jit_decode_wide", "lh_inverse_gt_kernel"]
PLAN = "lh_plan_kernel"
XOR = "lh_xor_reduce_kernel"
T_DEC, T_ENC = _t_lib(True), _t_lib(False)

# `tile`: the subject kernel's T; `also`: the chain's other kernels whose whole count set lies
# inside the subject's (asserted), so this case is theirs too.
DECODE = [
    _case("fused-1lane", 10, 4, 64, {}, T_DEC, FUSED),
    _case("fused-k29", 29, 4, 1296, {}, T_DEC, FUSED),
    _case("fused-64lane", 8, 4, 4096, {}, T_DEC, FUSED),
    _case("fused-family", 29, 4, 1312, FAMILY, T_DEC, FUSED_FAMILY),
    _case("fused-family-k4", 4, 5, 96, FAMILY, T_DEC, FUSED_FAMILY),
    # lh_plan_small_kernel<4> at the smallest block that keeps the chain (one lane per stripe)
    _case("small4-planner", 65, 4, 64, {}, _t_plan_small, SMALL4, also=[T_DEC]),
    _case("small4-k65", 65, 4, 1296, {}, T_DEC, SMALL4),
    _case("small8-planner", 10, 5, 64, {}, _t_plan_small, SMALL8, also=[T_DEC]),
    _case("two-waves-per-stripe", 8, 3, 8128, {}, T_DEC, SMALL4),
    # the order kernel's case: 1 .. 2049 and the grids of 1024; the planner (one workgroup per
    # stripe, four waves up to 4096 stripes and one above) and the in-place apply ride along
    _case("cf-order-jump", 9, 9, 64, {}, _t_order, GENERIC_CF, trace1=CF_ONE, extra=ORDER_EXTRA + PLAN_EXTRA,
          also=[_t_one]),
    _case("workspace-scatter", 30, 13, 24, {}, _t_bytewise, OLD_CF, also=[_t_scatter, _t_one]),
    _case("wide-m12", 40, 12, 2048, {}, _t_one, WIDE16, trace1=WIDE_ONE),
    _case("wide-m33", 40, 33, 2048, {}, _t_one, WIDE16, trace1=WIDE_ONE),
    _case("gen-s8", 20, 6, 64, GEN, _t_plan_small, GENERIC_S8, also=[_t_one]),
    _case("gen-jump", 40, 4, 64, GEN, _t_one, PS4_JUMP),
    _case("gen-jump2", 40, 4, 4160, GEN, _t_one, PS4_JUMP2),
    _case("m1-xor", 10, 1, 100, {}, _t_xor, [PLAN, XOR], mode="valid", also=[_t_one]),
    _case("k1", 1, 3, 40, {}, _t_one, [PLAN]),
    # the pointer-table forms (tests/test_gpu_ptrs.py DECODE / tools/precompile.py PTR_SHAPES)
    _case("ptrs-fused-k29", 29, 4, 1296, {}, T_DEC, _ptr(FUSED), form="table"),
    # (lh_jit_decode's own tile here is 128 -- the table form keeps the strided form's stripes per
    # wave, jit.cpp jit_ptr_config_for -- and its grids of 128 join the planner's counts)
    _case("ptrs-small8", 10, 6, 24, {}, _t_plan_small, ["lh_plan_small_kernel<8>", "lh_jit_decode" + PTR], form="table",
          extra=tuple(lhutil.stripe_counts(128)), also=[T_DEC]),
    _case("ptrs-wide", 40, 20, 4096, {}, _t_one, WIDE16[:1] + [WIDE16[1] + PTR] + WIDE16[2:], form="table",
          trace1=[WIDE_ONE[0], WIDE_ONE[1] + PTR, WIDE_ONE[2]]),
    _case("ptrs-cf-order-jump", 40, 20, 1024, {}, _t_one, GENERIC_CF[:2] + [GENERIC_CF[2] + PTR], form="table",
          trace1=[CF_ONE[0], CF_ONE[1] + PTR]),
    _case("ptrs-gather-sub3", 40, 20, 24, {}, _t_bytewise, [GATHER] + OLD_CF + [SCATTER], form="table",
          also=[_t_scatter, _t_one]),
    _case("ptrs-gather-m1", 10, 1, 100, {}, _t_xor, [GATHER, PLAN, XOR, SCATTER], form="table", mode="valid"),
    _case("ptrs-gather-k1", 1, 3, 40, {}, _t_one, [GATHER, PLAN, SCATTER], form="table"),
]

# the plain (no LDS staging) and the several-waves-per-stripe forms of lh_jit_encode, from the
# build's specialised sample (test_gpu_boundaries.JIT_SAMPLE): see _sample_shape
ENC = ["lh_jit_encode"]
ENCODE = [
    _case("jit-1lane", 10, 4, 64, {}, T_ENC, ENC),
    _case("jit-lds-k29", 29, 4, 1296, {}, T_ENC, ENC),
    _case("jit-plain", None, None, None, {}, T_ENC, ENC),
    _case("jit-waves-per-stripe", None, None, None, {}, T_ENC, ENC),
    _case("jit-k8m3", 8, 3, 8128, {}, T_ENC, ENC),
    _case("jit-family", 29, 4, 1312, FAMILY, T_ENC, ["lh_jit_encode(family)"]),
    _case("win-m13", 40, 13, 2048, {}, _t_one, ["lh_jit_encode_win"]),
    _case("jump", 10, 13, 64, {}, _t_flat_jump, JUMP),
    _case("jump2", 40, 4, 4160, GEN, _t_flat_jump, JUMP2),
    _case("jump2-packed", 40, 4, 64, GEN, _t_flat_jump, JUMP2),     # one two-dword lane per stripe: T = 64
    _case("bytewise", 30, 13, 24, {}, _t_bytewise, ["lh_apply_generic_kernel"]),
    _case("xor", 10, 1, 100, {}, _t_xor, [XOR]),
    _case("k1-copies", 1, 3, 40, {}, _t_xor, [XOR]),
    _case("ptrs-jit-k29", 29, 4, 1296, {}, T_ENC, _ptr(ENC), form="table"),
    _case("ptrs-jit-small", 10, 6, 24, {}, T_ENC, _ptr(ENC), form="table"),
    _case("ptrs-win", 40, 20, 4096, {}, _t_one, ["lh_jit_encode_win" + PTR], form="table"),
    _case("ptrs-jump", 40, 20, 1024, {}, _t_flat_jump, _ptr(JUMP), form="table"),
    _case("ptrs-gather-sub3", 40, 20, 24, {}, _t_bytewise, [GATHER, "lh_apply_generic_kernel", SCATTER], form="table"),
    _case("ptrs-gather-m1", 10, 1, 100, {}, _t_xor, [GATHER, XOR, SCATTER], form="table"),
    _case("ptrs-gather-k1", 1, 3, 40, {}, _t_xor, [GATHER, XOR, SCATTER], form="table"),
]


def _sample_shape(lh, which):
    """The first shape of JIT_SAMPLE whose encode is the plain form (no LDS staging, whole
    stripes per wave) / takes several waves per stripe (T = 1 with more lanes than a wave)."""
    for k, m, b in JIT_SAMPLE:
        t = lh.stripes_per_workgroup(k, m, b)
        if which == "jit-plain" and not lh.lds_staged(k, m, b) and t > 1:
            return k, m, b
        if which == "jit-waves-per-stripe" and t == 1:   # (no whole stripe per wave: more than 64 lanes)
            return k, m, b
    raise AssertionError(("no such shape in JIT_SAMPLE", which))


@pytest.fixture(scope="module")
def lh():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    import longhair_amd
    assert longhair_amd.cauchy_256_init() == 0
    return longhair_amd


# ------------------------------------------------------------------ buffers and their expected images
class Swept:
    """One buffer of a sweep, flat uint8 on the device: `buf` the calls work on, `pristine` what
    it holds before each call, `full` what it holds after a call on every prepared stripe, and
    `owner`, per byte the stripe it belongs to (OUTSIDE for guards, pads and gaps).  After a call
    on n stripes it must equal `full` where owner < n and `pristine` elsewhere."""

    def __init__(self, name, buf, full, owner, locate):
        assert buf.shape == full.shape == owner.shape and buf.dim() == 1
        self.name, self.buf, self.pristine, self.full, self.owner, self.locate = name, buf, buf.clone(), full, owner, locate

    def restore(self):
        self.buf.copy_(self.pristine)

    def expected(self, n):
        import torch
        return torch.where(self.owner < n, self.full, self.pristine)

    def wrong(self, n):
        return (self.buf != self.expected(n)).any()

    def first_wrong(self, n):
        """None, or a description of the first byte that differs from the expectation for n."""
        got, exp = self.buf.cpu().numpy(), self.expected(n).cpu().numpy()
        at = np.nonzero(got != exp)[0]
        if at.size == 0:
            return None
        where = self.locate(int(at[0]))
        if where is None:
            return f"{self.name}: byte {int(at[0])} of the allocation, outside every stripe (a guard, pad or gap), overwritten"
        s, blk, byte = where
        what = "overwritten beyond the batch" if s >= n else "wrong"
        return (f"{self.name}: stripe {s} block {blk} byte {byte} {what}: got {int(got[at[0]]):#04x}, "
                f"expected {int(exp[at[0]]):#04x} ({at.size} bytes differ)")


def _strided(name, before, after, canary, block):
    """A packed strided buffer between guards (test_gpu_untouched.Guarded): `before` / `after`
    uint8 [stripes, n], blocks of `block` bytes.  Returns (Swept, Guarded)."""
    import torch
    g = tu.Guarded(before, 0, 0, canary)
    full = tu.Guarded(after, 0, 0, canary).buf
    stripes, n = before.shape
    owner = torch.full((g.buf.numel(),), OUTSIDE, dtype=torch.int32, device="cuda")
    owner[GUARD:GUARD + stripes * n] = torch.arange(stripes, dtype=torch.int32, device="cuda").repeat_interleave(n)

    def locate(at):
        o = at - GUARD
        return (o // n, (o % n) // block, o % block) if 0 <= o < stripes * n else None
    return Swept(name, g.buf, full, owner, locate), g


def _place(rows2d, place, values):
    """values [S * n, ...] into the blocks' places of a pool viewed as [S * n, stride] (the loop
    of test_gpu_ptrs._scatter)."""
    import torch
    S, n, B, stride, order, offs = place
    for o in np.unique(offs):
        sel = np.nonzero(offs == o)[0]
        rows2d[torch.from_numpy(order[sel]).cuda(), int(o):int(o) + B] = values[torch.from_numpy(sel).cuda()]


def _pooled(name, before, after, seed):
    """Blocks scattered over a pool (test_gpu_ptrs._scatter: random places, random byte offsets)
    with their pointer table: `before` / `after` uint8 [stripes, n, B].  Returns (Swept of the
    pool, Swept of the table -- which no call may change --, the table)."""
    import torch
    pool, ptrs, place = tp._scatter(torch.from_numpy(np.ascontiguousarray(before)).cuda(), seed)
    S, n, B, stride, order, offs = place
    full = pool.clone()
    _place(full[:S * n * stride].view(S * n, stride), place, torch.from_numpy(np.ascontiguousarray(after)).cuda().reshape(S * n, B))
    owner = torch.full((pool.numel(),), OUTSIDE, dtype=torch.int32, device="cuda")
    stripe_of = (torch.arange(S * n, dtype=torch.int32, device="cuda") // n)[:, None].expand(S * n, B)
    _place(owner[:S * n * stride].view(S * n, stride), place, stripe_of)
    start = order * stride + offs            # block b = s * n + i starts here
    by_start = np.argsort(start)

    def locate(at):
        j = int(np.searchsorted(start[by_start], at, side="right")) - 1
        b = int(by_start[j]) if j >= 0 else -1
        return (b // n, b % n, at - int(start[b])) if b >= 0 and at < start[b] + B else None
    table = ptrs.view(torch.uint8).reshape(-1)
    nowhere = torch.full((table.numel(),), OUTSIDE, dtype=torch.int32, device="cuda")
    return (Swept(name, pool, full, owner, locate), Swept(name + " pointer table", table, table.clone(), nowhere, lambda at: None),
            ptrs)


# ------------------------------------------------------------------ the sweep
def sweep(lh, case, counts, bufs, call, shift=0):
    """Runs `call(n)` for every count in a seeded shuffled order, the buffers restored before and
    compared after each (on the device; one read of the flags at the end).  Returns (failing
    counts ascending, the launch trace per count, the number of calls made, seconds, the counts
    in the order they ran).  `shift`
    moves the expectation to n + shift stripes written: 0 is the test; -1 and +1 are the two
    mutations that must fail at every count (tests/test_gpu_stripe_counts.py docstring)."""
    import torch
    order = np.random.Generator(np.random.PCG64(case.k * 1000 + case.m * 10 + case.nbytes)).permutation(len(counts))
    flags = torch.zeros((len(counts), len(bufs)), dtype=torch.bool, device="cuda")
    traces, calls = {}, 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in order.tolist():
        n = counts[i]
        for b in bufs:
            b.restore()
        call(n)
        calls += 1
        traces[n] = lh.last_launch()
        for j, b in enumerate(bufs):
            flags[i, j] = b.wrong(n + shift)
    bad = flags.any(dim=1).cpu().numpy()       # (synchronises)
    seconds = time.perf_counter() - t0
    return [counts[i] for i in np.nonzero(bad)[0]], traces, calls, seconds, [counts[i] for i in order.tolist()]


def _report(case, T, counts, failing, ran, bufs, call, shift=0):
    """The failure message: the failing counts and, for the smallest -- run again after the count
    that preceded it in the sweep -- the first wrong byte of the first wrong buffer."""
    import torch
    n = failing[0]
    at = ran.index(n)
    if at > 0:
        for b in bufs:
            b.restore()
        call(ran[at - 1])
    for b in bufs:
        b.restore()
    call(n)
    torch.cuda.synchronize()
    first = next((w for w in (b.first_wrong(n + shift) for b in bufs) if w), "(did not fail again when run after its predecessor alone)")
    return (f"{case.id} (k {case.k} m {case.m} {case.nbytes} B, {case.form}, T {T}): {len(failing)} of {len(counts)} "
            f"stripe counts fail: {failing[:40]}{' ...' if len(failing) > 40 else ''}; stripes = {n}"
            f"{f' (after {ran[at - 1]})' if at > 0 else ''}: {first}")


TIMES = []   # (case, form, T, N_max, counts, prepare s, GPU s), printed by the last test


def _counts(lh, case):
    T = case.tile(lh, case.k, case.m, case.nbytes)
    counts = lhutil.stripe_counts(T, case.extra)
    for other in case.also:   # the chain's narrower tiles: their whole sets lie inside this one
        t = other(lh, case.k, case.m, case.nbytes)
        assert set(lhutil.stripe_counts(t)) <= set(counts), (case.id, "tile", t, "is not covered by the sweep of", T)
    return T, counts


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _seed(case):
    return case.k * 1000 + case.m * 10 + case.nbytes + 5


def decode_sweep(lh, oracle, case, shift=0, counts=None):
    """Prepares one decode case and sweeps it.  Returns what `sweep` returns plus what `_report`
    needs; test_decode_counts asserts on it (a script may call it with a shifted expectation)."""
    k, m, nbytes = case.k, case.m, case.nbytes
    T, all_counts = _counts(lh, case)
    counts = all_counts if counts is None else counts
    N = all_counts[-1] + 1
    t0 = time.perf_counter()
    blocks, rows, invalid, exp_blocks, exp_rows = tu.mixed_case(oracle, k, m, nbytes, N, _seed(case), case.mode)
    prepare = time.perf_counter() - t0
    if case.form == "table":
        B, tab, ptrs = _pooled("blocks", blocks, exp_blocks, _seed(case))
        bufs = [B, tab]
    else:
        B, gb = _strided("blocks", blocks.reshape(N, k * nbytes), exp_blocks.reshape(N, k * nbytes), C_BLOCKS, nbytes)
        bufs = [B]
    R, gr = _strided("rows", rows, exp_rows, C_ROWS, 1)
    status = np.where(invalid, 0xFF, 0).astype(np.uint8).reshape(N, 1)
    S, gs = _strided("status", np.full((N, 1), C_STATUS, dtype=np.uint8), status, C_STATUS, 1)
    bufs += [R, S]
    lib = lh.lib()

    def call(n):
        if case.form == "table":
            rc = lib.cauchy_256_decode_batch_ptrs(k, m, nbytes, n, ctypes.c_void_p(ptrs.data_ptr()), ctypes.c_void_p(gr.ptr),
                                                  ctypes.c_void_p(gs.ptr), _stream())
        else:
            rc = lib.cauchy_256_decode_batch(k, m, nbytes, n, ctypes.c_void_p(gb.ptr), ctypes.c_longlong(gb.stride),
                                             ctypes.c_void_p(gr.ptr), ctypes.c_void_p(gs.ptr), _stream())
        assert rc == 0, (case.id, n, rc, lib.cauchy_256_last_error())
    failing, traces, calls, seconds, ran = sweep(lh, case, counts, bufs, call, shift)
    TIMES.append((("decode", case.id), case.form, T, counts[-1], len(counts), prepare, seconds))
    return T, counts, failing, traces, calls, ran, bufs, call


def encode_sweep(lh, oracle, case, shift=0, counts=None):
    """As decode_sweep for an encode case: the recovery buffer a canary before each call, the data
    buffer never written."""
    k, m, nbytes = case.k, case.m, case.nbytes
    T, all_counts = _counts(lh, case)
    counts = all_counts if counts is None else counts
    N = all_counts[-1] + 1
    t0 = time.perf_counter()
    data, rec = tu._encoded(oracle, k, m, nbytes, N, _seed(case))
    prepare = time.perf_counter() - t0
    blank = np.full((N, m, nbytes), C_ROWS, dtype=np.uint8)
    if case.form == "table":
        D, dtab, dptrs = _pooled("data", data, data, _seed(case))
        O, otab, optrs = _pooled("recovery", blank, rec, _seed(case) + 1)
        bufs = [D, dtab, O, otab]
    else:
        D, gd = _strided("data", data.reshape(N, k * nbytes), data.reshape(N, k * nbytes), C_BLOCKS, nbytes)
        O, go = _strided("recovery", blank.reshape(N, m * nbytes), rec.reshape(N, m * nbytes), C_ROWS, nbytes)
        bufs = [D, O]
    lib = lh.lib()

    def call(n):
        if case.form == "table":
            rc = lib.cauchy_256_encode_batch_ptrs(k, m, nbytes, n, ctypes.c_void_p(dptrs.data_ptr()),
                                                  ctypes.c_void_p(optrs.data_ptr()), _stream())
        else:
            rc = lib.cauchy_256_encode_batch(k, m, nbytes, n, ctypes.c_void_p(gd.ptr), ctypes.c_longlong(gd.stride),
                                             ctypes.c_void_p(go.ptr), ctypes.c_longlong(go.stride), _stream())
        assert rc == 0, (case.id, n, rc, lib.cauchy_256_last_error())
    failing, traces, calls, seconds, ran = sweep(lh, case, counts, bufs, call, shift)
    TIMES.append((("encode", case.id), case.form, T, counts[-1], len(counts), prepare, seconds))
    return T, counts, failing, traces, calls, ran, bufs, call


def _check(case, result):
    T, counts, failing, traces, calls, ran, bufs, call = result
    assert calls == len(counts) and sorted(ran) == counts, (case.id, "calls", calls, "counts", len(counts))
    assert traces[counts[-1]] == case.trace, (case.id, "stripes", counts[-1], traces[counts[-1]])
    assert traces[1] == case.trace1, (case.id, "stripes 1", traces[1])
    if failing:
        pytest.fail(_report(case, T, counts, failing, ran, bufs, call), pytrace=False)


def _resolve(lh, monkeypatch, case):
    tu._set_env(monkeypatch, case.env)
    if case.k is None:
        return case._replace(**dict(zip(("k", "m", "nbytes"), _sample_shape(lh, case.id))))
    return case


@pytest.mark.parametrize("case", DECODE, ids=[c.id for c in DECODE])
def test_decode_counts(lh, oracle, monkeypatch, case):
    """cauchy_256_decode_batch / _ptrs on every prefix length of one mixed batch of valid and
    invalid stripes: stripes < n are mixed_case's expectation (blocks, rewritten rows, status 0 or
    -1), stripes >= n hold their input, their status bytes the canary, the guards theirs."""
    case = _resolve(lh, monkeypatch, case)
    _check(case, decode_sweep(lh, oracle, case))


@pytest.mark.parametrize("case", ENCODE, ids=[c.id for c in ENCODE])
def test_encode_counts(lh, oracle, monkeypatch, case):
    """cauchy_256_encode_batch / _ptrs on every prefix length of one batch: recovery blocks of
    stripes < n are the oracle's, every other byte of the recovery buffer (the stripes from n on,
    the guards, the pool's gaps) the canary it held, the data buffer byte-identical."""
    case = _resolve(lh, monkeypatch, case)
    _check(case, encode_sweep(lh, oracle, case))


def test_sample_shapes(lh):
    """The two cases taken from JIT_SAMPLE are what their names say."""
    k, m, b = _sample_shape(lh, "jit-plain")
    assert lh.batch_path(k, m, b) == "jit" and not lh.lds_staged(k, m, b) and lh.stripes_per_workgroup(k, m, b) > 1
    k, m, b = _sample_shape(lh, "jit-waves-per-stripe")
    assert lh.batch_path(k, m, b) == "jit" and lh.stripes_per_workgroup(k, m, b) == 1


def test_zero_stripes(lh, oracle):
    """stripes = 0 through every batch entry point (strided and table encode and decode, frame,
    unframe): 0 is returned, nothing is launched -- the trace, non-empty from the call before, is
    empty -- and no byte of any buffer or guard changes."""
    import torch
    k, m, nbytes, N = 10, 4, 64, 6
    lib = lh.lib()
    blocks, rows, invalid, exp_blocks, exp_rows = tu.mixed_case(oracle, k, m, nbytes, N, 7)
    data, rec = tu._encoded(oracle, k, m, nbytes, N, 7)
    gd = tu.Guarded(data.reshape(N, k * nbytes), 3, 5, C_BLOCKS)
    go = tu.Guarded(rec.reshape(N, m * nbytes), 3, 5, C_ROWS)
    gb = tu.Guarded(blocks.reshape(N, k * nbytes), 3, 5, C_BLOCKS)
    gr = tu.Guarded(rows.reshape(1, N * k), 0, 0, C_ROWS)
    gs = tu.Guarded(np.full((1, N), C_STATUS, dtype=np.uint8), 0, 0, C_STATUS)
    gp = tu.Guarded(lhutil.fill(3, N * (k + m) * (nbytes + 1)).reshape(N, (k + m) * (nbytes + 1)), 3, 5, C_STATUS)
    dpool, dptrs, _ = tp._scatter(torch.from_numpy(np.array(data)).cuda(), 1)
    opool, optrs, _ = tp._scatter(torch.from_numpy(np.array(rec)).cuda(), 2)
    bpool, bptrs, _ = tp._scatter(torch.from_numpy(np.array(blocks)).cuda(), 3)
    held = [gd.buf, go.buf, gb.buf, gr.buf, gs.buf, gp.buf, dpool, dptrs, opool, optrs, bpool, bptrs]
    before = [t.clone() for t in held]
    vp, ll = ctypes.c_void_p, ctypes.c_longlong
    calls = {
        "encode_batch": lambda n: lib.cauchy_256_encode_batch(k, m, nbytes, n, vp(gd.ptr), ll(gd.stride), vp(go.ptr),
                                                              ll(go.stride), _stream()),
        "decode_batch": lambda n: lib.cauchy_256_decode_batch(k, m, nbytes, n, vp(gb.ptr), ll(gb.stride), vp(gr.ptr),
                                                              vp(gs.ptr), _stream()),
        "encode_batch_ptrs": lambda n: lib.cauchy_256_encode_batch_ptrs(k, m, nbytes, n, vp(dptrs.data_ptr()),
                                                                        vp(optrs.data_ptr()), _stream()),
        "decode_batch_ptrs": lambda n: lib.cauchy_256_decode_batch_ptrs(k, m, nbytes, n, vp(bptrs.data_ptr()), vp(gr.ptr),
                                                                        vp(gs.ptr), _stream()),
        "frame_batch": lambda n: lib.cauchy_256_frame_batch(k, m, nbytes, n, vp(gd.ptr), ll(gd.stride), vp(go.ptr),
                                                            ll(go.stride), vp(gp.ptr), ll(gp.stride), _stream()),
        "unframe_batch": lambda n: lib.cauchy_256_unframe_batch(k, nbytes, n, vp(gp.ptr), ll(gp.stride), vp(gb.ptr),
                                                                ll(gb.stride), vp(gr.ptr), _stream()),
    }
    scratch = torch.zeros((N, k, nbytes), dtype=torch.uint8, device="cuda")
    for name, fn in calls.items():
        lh.encode_batch(scratch, m)                      # leaves a trace behind
        assert lh.last_launch() == ["lh_jit_encode"]
        assert fn(0) == 0, (name, lib.cauchy_256_last_error())
        assert lh.last_launch() == [], (name, lh.last_launch())
        torch.cuda.synchronize()
        for t, b in zip(held, before):
            assert torch.equal(t, b), (name, "stripes = 0 changed a buffer")
    # ... and each of them does write these buffers when it has a stripe (the test can fail)
    for name, fn in calls.items():
        assert fn(N) == 0, (name, lib.cauchy_256_last_error())
        assert lh.last_launch() != [], name
    torch.cuda.synchronize()
    assert not all(torch.equal(t, b) for t, b in zip(held, before))


def test_times(lh):
    """Prints what the sweeps above cost (pytest -s): per case T, the largest count, the number
    of counts, the CPU preparation and the GPU sweep."""
    for (what, cid), form, T, nmax, n, prepare, gpu in TIMES:
        print(f"stripe-counts {what:6s} {cid:22s} {form:7s} T {T:5d} N_max {nmax:6d} counts {n:5d} "
              f"prepare {prepare:6.2f} s  gpu {gpu:6.2f} s")
