"""Batch decode over deterministic erasure patterns, per kernel family.

Every other decode test draws its patterns from lhutil.erasure_case (random erased originals,
random recovery rows, shuffled slots), so which slot holds a recovery block, which originals
are missing, which rows stand in and how many is luck.  The decode kernels branch on exactly
those: the fused in-kernel plan (per-stripe ballots, the adjugate inverse padded to LH_EMAX),
lh_plan_small_kernel<4|8>, lh_plan_kernel (two rows per lane, slots classified in passes of 64,
the closed form's all-ones row 0), lh_order_kernel, phase B and the wide decode's used-row
ballot.  Here each row of ROWS is one batch whose stripes are every pattern x placement
(lhutil.pattern_cases) of its shape -- every pattern there is for the small codes ('x':
lhutil.exhaustive_patterns), the designed net for the others ('d': lhutil.designed_patterns) --
in a seeded shuffle of the stripe order, so that a wave holds mixed e.  One decode_batch call;
every status 0, rows and bytes of the whole batch the oracle's, the stripe count the
generator's (nothing sampled or capped) and the launch trace the row's.  A mismatch names the
first differing stripe with its (E, R, placement).  The oracle's own decode is pinned to the
reference over the same cases in tests/test_decode_patterns.py.

Placements: all five, except where a designed batch would hold more than 64 MiB of blocks and
at (128, 128), where the oracle's expectation of all five (4 400 stripes at e up to 128) takes
7 to 20 s depending on the CPU: there (a), (c) and (e) (KEEP); the pattern list is never thinned.

`-m gpu`: needs an MI355X.  Every module is compiled at build time (tools/precompile.py; the
tests run with LONGHAIR_AMD_JIT_COMPILE=0, so a missing one shows in the trace, not as a wait).
"""
import functools

import numpy as np
import pytest

import lhutil
import test_gpu_boundaries as tb
import test_gpu_untouched as tu
from test_gpu_boundaries import FUSED, GEN, GENERIC_CF, PS4_JUMP, PS8_JUMP, SMALL4, SMALL8

pytestmark = pytest.mark.gpu

NOFUSED = {"LONGHAIR_AMD_NO_FUSED_PLAN": "1"}
PLAN_GJ = {"LONGHAIR_AMD_PLAN_GJ": "1"}
GENERIC_GJ = ["lh_plan_kernel", "lh_order_kernel", "lh_apply_jump_kernel"]
PS8_BYTEWISE = ["lh_plan_small_kernel<8>", "lh_apply_generic_kernel", "lh_scatter_kernel"]
# m = 1 and k = 1 (codec.cpp kPathXor): the planner names the output slot, one XOR pass fills
# it; a lone block (k = 1) is already the original, only its row is rewritten
XOR_M1 = ["lh_plan_kernel", "lh_xor_reduce_kernel"]
XOR_K1 = ["lh_plan_kernel"]

# (id, k, m, bytes, set, env, decode kernels).  Exhaustive sets at the block size of
# tools/precompile.py sweep_shapes (8 * (1 + (7 k + m) % 8)).
ROWS = [
    ("x-k4m4-fused", 4, 4, 8, "x", {}, FUSED),
    ("x-k6m4-fused", 6, 4, 56, "x", {}, FUSED),
    ("x-k8m2-fused", 8, 2, 24, "x", {}, FUSED),
    ("x-k5m5-small8", 5, 5, 8, "x", {}, SMALL8),
    ("x-k6m6-small8", 6, 6, 8, "x", {}, SMALL8),
    ("x-k4m4-nofused", 4, 4, 8, "x", NOFUSED, SMALL4),
    ("x-k4m4-gen-jump", 4, 4, 32, "x", GEN, PS4_JUMP),
    ("x-k6m6-gen-jump", 6, 6, 32, "x", GEN, PS8_JUMP),
    ("x-k6m6-gen-bytewise", 6, 6, 8, "x", GEN, PS8_BYTEWISE),
    ("x-k8m1-xor", 8, 1, 8, "x", {}, XOR_M1),       # the oracle's bytes are the rule, quirk included
    ("x-k1m4-xor", 1, 4, 8, "x", {}, XOR_K1),
]
# The designed sets: the family rows of test_gpu_untouched.MIXED (their traces are written
# down there), two rows of test_gpu_boundaries.BOUNDARIES and RC = 128 with two rows per lane.
# Placements (a), (c), (e) only, the pattern list whole (KEEP below; all five would exceed
# 64 MiB of blocks): small4, wide-m12, wide-m20, wide-m33, gen-jump2 and, one code having one
# set of cases, gen-jump beside it; k128m128 (the oracle's expectation: 2 437 stripes take 4 s).
ROWS += [("d-" + name,) + tu.BY_ID[name][1:4] + ("d",) + tu.BY_ID[name][5:7] for name in (
    "fused-1lane", "fused-k29", "fused-64lane", "fused-family", "fused-family-k4", "small4", "small8-e8",
    "cf-jump", "workspace-sub3", "wide-m12", "wide-m20", "wide-m33", "gen-jump", "gen-jump2")]
ROWS += [("d-" + c[0],) + c[1:4] + ("d", c[5], c[7]) for c in tb.BOUNDARIES if c[0] in ("wide-m64", "generic-m65")]
ROWS += [
    ("d-cf-jump-gj", 9, 9, 64, "d", PLAN_GJ, GENERIC_GJ),
    ("d-k128m128", 128, 128, 64, "d", {}, GENERIC_CF),
    ("d-k128m128-gj", 128, 128, 64, "d", PLAN_GJ, GENERIC_GJ),
]
assert len(ROWS) == 11 + 14 + 2 + 3
BY_ID = {r[0]: r for r in ROWS}

# The pointer-table form (tools/precompile.py PTR_SHAPES): (id, k, m, bytes, set, decode kernels)
PTR_ROWS = [
    ("d-k29m4", 29, 4, 1296, "d", ["lh_jit_decode_fused(pointer table)"]),
    ("d-k40m20", 40, 20, 4096, "d", ["lh_plan_kernel(closed form)", "lh_jit_decode_wide(pointer table)",
                                     "lh_order_kernel", "lh_inverse_gt_kernel"]),
    ("x-k10m6", 10, 6, 24, "x", ["lh_plan_small_kernel<8>", "lh_jit_decode(pointer table)"]),
]
# The drop-in call, one call per case: (k, m, bytes)
DROPIN = [(4, 4, 8), (8, 1, 8)]

BATCH_LIMIT = 64 << 20


def patterns_of(k, m, kind):
    return lhutil.exhaustive_patterns(k, m) if kind == "x" else lhutil.designed_patterns(k, m)


def _keep():
    """(k, m, set) -> the placements of every row of that code: (a), (c), (e) where one of its
    designed batches would exceed BATCH_LIMIT with all five, and at (128, 128)."""
    keep = {}
    for k, m, nbytes, kind in [r[1:5] for r in ROWS] + [r[1:5] for r in PTR_ROWS] + [d + ("x",) for d in DROPIN]:
        keep.setdefault((k, m, kind), lhutil.PLACEMENTS)
        if kind == "d":
            full = len(lhutil.pattern_cases(k, m, patterns_of(k, m, kind), seed_of(k, m)))
            if full * k * nbytes > BATCH_LIMIT or (k, m) == (128, 128):
                keep[(k, m, kind)] = "ace"
    return keep


def seed_of(k, m):
    return k * 1000 + m


KEEP = _keep()
# Every (k, m, set, placements) above: what tests/test_decode_patterns.py and
# tools/make_golden.py run on the CPU at 8-byte blocks.
CODES = sorted((k, m, kind, keep) for (k, m, kind), keep in KEEP.items())


def cases_of(k, m, kind):
    return lhutil.pattern_cases(k, m, patterns_of(k, m, kind), seed_of(k, m), KEEP[(k, m, kind)])


CPU_BYTES = 8


def cpu_decode(codec, k, m, kind):
    """One code's cases at 8-byte blocks, encoded and decoded one call per case by `codec` (the
    oracle, the reference or a drop-in library), in generation order:
    (cases, return codes, rows out, blocks out)."""
    cases = cases_of(k, m, kind)
    blocks, rows = lhutil.pattern_batch(codec, k, m, CPU_BYTES, cases, seed_of(k, m))
    return (cases,) + lhutil.decode_all(codec, k, m, blocks, rows, CPU_BYTES)


@pytest.fixture(scope="module")
def lh():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    import longhair_amd
    assert longhair_amd.cauchy_256_init() == 0
    return longhair_amd


@pytest.fixture(params=["default", "gpu", "host-avx512bw", "host-avx2", "host-scalar"])
def policy(request, lh, monkeypatch):
    """Drop-in dispatch policy, as tests/test_gpu_parity.py: the library's default (AUTO), the
    GPU, and each instruction-set level of the host engine."""
    import os
    if request.param == "default":
        if "LONGHAIR_AMD_DISPATCH" not in os.environ:
            assert lh.dispatch_policy() == "auto"
        prev = lh.dispatch_policy()
    elif request.param == "gpu":
        prev = lh.set_dispatch("gpu")
    else:
        isa = request.param.split("-")[1]
        if isa == "avx512bw" and lh.host_isa() != "avx512bw":
            pytest.skip("host CPU without AVX-512BW")
        monkeypatch.setenv("LONGHAIR_AMD_HOST_ISA", isa)
        prev = lh.set_dispatch("host")
        assert lh.host_isa() == isa
    yield request.param
    lh.set_dispatch(prev)


@functools.lru_cache(maxsize=None)
def expected(oracle, k, m, nbytes, kind):
    """One shape's cases, received stripes and the oracle's decode of them, in generation
    order, computed once and shared read-only: (cases, blocks, rows, rows out, blocks out)."""
    cases = cases_of(k, m, kind)
    blocks, rows = lhutil.pattern_batch(oracle, k, m, nbytes, cases, seed_of(k, m) * 10 + 1)
    rcs, exp_rows, exp_blocks = lhutil.decode_all(oracle, k, m, blocks, rows, nbytes)
    assert (rcs == 0).all()
    for a in (blocks, rows, exp_rows, exp_blocks):
        a.setflags(write=False)
    return cases, blocks, rows, exp_rows, exp_blocks


def stripe_order(n, seed, shuffle=True):
    return np.random.Generator(np.random.PCG64(seed)).permutation(n) if shuffle else np.arange(n)


def compare(tag, cases, order, got_status, got_rows, got_blocks, exp_rows, exp_blocks):
    """Whole-batch comparison; `order[s]` is the case in stripe s.  The message names the first
    differing stripe and its case."""
    assert len(order) == len(cases) == got_rows.shape[0] == got_blocks.shape[0]
    assert sorted(order.tolist()) == list(range(len(cases)))
    bad = (got_status != 0) | (got_rows != exp_rows[order]).any(axis=1) | \
          (got_blocks != exp_blocks[order]).any(axis=(1, 2))
    if bad.any():
        s = int(np.argmax(bad))
        E, R, label, slots, rows = cases[int(order[s])]
        slots_bad = np.nonzero((got_blocks[s] != exp_blocks[order[s]]).any(axis=1))[0].tolist()
        # (and the differing case that comes first in generation order: the fewest erasures)
        E0, R0, label0 = cases[int(np.min(order[bad]))][:3]
        raise AssertionError((tag, f"{int(bad.sum())} of {len(cases)} stripes differ; first: stripe {s}",
                              {"E": list(E), "R": list(R), "placement": label, "rows in": rows,
                               "status": int(got_status[s]), "rows out": got_rows[s].tolist(),
                               "rows expected": exp_rows[order[s]].tolist(), "slots with wrong bytes": slots_bad},
                              "earliest differing case", {"E": list(E0), "R": list(R0), "placement": label0}))


def run_strided(lh, oracle, monkeypatch, name, shuffle=True):
    import torch
    _, k, m, nbytes, kind, env, kernels = BY_ID[name]
    monkeypatch.setenv("LONGHAIR_AMD_JIT_COMPILE", "0")
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    cases, blocks, rows, exp_rows, exp_blocks = expected(oracle, k, m, nbytes, kind)
    order = stripe_order(len(cases), seed_of(k, m) + nbytes, shuffle)
    d_blocks = torch.from_numpy(blocks[order]).cuda()
    d_rows = torch.from_numpy(rows[order]).cuda()
    status = lh.decode_batch(d_blocks, d_rows, m)
    torch.cuda.synchronize()
    trace = lh.last_launch()
    # the batch is the generator's whole output (a second run of it): nothing sampled or capped
    generated = cases_of(k, m, kind)
    assert status.numel() == d_rows.shape[0] == len(generated) and generated == cases
    if kind == "x":
        import math
        assert len({(c[0], c[1]) for c in cases}) == math.comb(k + m, k)
    compare((name, trace), cases, order, status.cpu().numpy(), d_rows.cpu().numpy(), d_blocks.cpu().numpy(),
            exp_rows, exp_blocks)
    assert trace == kernels, (name, trace)


@pytest.mark.parametrize("name", [r[0] for r in ROWS])
def test_pattern_batch(lh, oracle, monkeypatch, name):
    run_strided(lh, oracle, monkeypatch, name)


def test_pattern_batch_in_enumeration_order(lh, oracle, monkeypatch):
    """The exhaustive (4, 4) set unshuffled: a wave's stripes share e, and neighbours differ
    in one element of R or E."""
    run_strided(lh, oracle, monkeypatch, "x-k4m4-fused", shuffle=False)


@pytest.mark.parametrize("name,k,m,nbytes,kind,kernels", PTR_ROWS, ids=[r[0] for r in PTR_ROWS])
def test_pattern_batch_ptrs(lh, oracle, monkeypatch, name, k, m, nbytes, kind, kernels):
    """The same batches through decode_batch_ptrs, the blocks scattered in one arena as
    tests/test_gpu_ptrs.py lays them out (random place, random byte offset)."""
    import torch
    import test_gpu_ptrs as tp
    monkeypatch.setenv("LONGHAIR_AMD_JIT_COMPILE", "0")
    cases, blocks, rows, exp_rows, exp_blocks = expected(oracle, k, m, nbytes, kind)
    order = stripe_order(len(cases), seed_of(k, m) + nbytes + 1)
    pool, ptrs, place = tp._scatter(torch.from_numpy(blocks[order]).cuda(), seed=seed_of(k, m))
    d_rows = torch.from_numpy(rows[order]).cuda()
    status = lh.decode_batch_ptrs(k, m, nbytes, ptrs, d_rows)
    torch.cuda.synchronize()
    trace = lh.last_launch()
    compare((name, trace), cases, order, status.cpu().numpy(), d_rows.cpu().numpy(),
            tp._gather(pool, place).cpu().numpy(), exp_rows, exp_blocks)
    assert trace == kernels, (name, trace)
    tp._gaps_untouched(pool, place)


@pytest.mark.parametrize("k,m,nbytes", DROPIN, ids=[f"k{k}m{m}" for k, m, _ in DROPIN])
def test_pattern_dropin(lh, oracle, policy, k, m, nbytes):
    """cauchy_256_decode, one call per case of the exhaustive set, under every dispatch policy."""
    cases, blocks, rows, exp_rows, exp_blocks = expected(oracle, k, m, nbytes, "x")
    codec = lhutil._Codec(lh.lib(), lh.lib().cauchy_256_encode, lh.lib().cauchy_256_decode)
    rcs, got_rows, got_blocks = lhutil.decode_all(codec, k, m, blocks, rows, nbytes)
    compare((policy, k, m), cases, np.arange(len(cases)), rcs, got_rows, got_blocks, exp_rows, exp_blocks)
