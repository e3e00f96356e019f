"""What the batch calls must not write (include/cauchy_256_batch.h:33-38, README.md): an
invalid stripe (a duplicate row, or a row >= k + m) gets status -1 and is left untouched,
`d_status` may be NULL, and nothing outside the blocks, the rows and the status is written.

Per kernel family of the decode (the launch trace asserted, as in test_gpu_boundaries.py) one
batch mixes valid stripes (random e, the first valid one at e_max, shuffled slots) with invalid
ones -- stripe 0, the last stripe, two adjacent interior stripes and seeded-random others,
about a quarter in all, cycling through every (kind, position) pair of
lhutil.invalidate_rows, their blocks random bytes.  The blocks,
the rows and the status each sit between two 256-byte guards inside their allocation, filled
with canaries; the decode buffer starts `off` bytes past its guard with `pad` bytes between
stripes.  Valid stripes must equal the oracle's decode (called on valid stripes only: invalid
rows are undefined behaviour in the reference), invalid ones what went in, every canary byte
must survive.  The encode side runs the windowed, jump, jump2 and bytewise kernels between
guards in the same way.  All comparisons are byte for byte.  `-m gpu`: needs an MI355X; every
shape's module is compiled at build time for the existing tests (tools/precompile.py)."""
import ctypes
import functools

import numpy as np
import pytest

import lhutil
from test_gpu_boundaries import (FUSED, GEN, GENERIC_CF, GENERIC_S8, JUMP, JUMP2, OLD_CF, PS4_JUMP, PS4_JUMP2, SMALL4,
                                 SMALL8, WIDE16, WIDE64, _scenarios)

pytestmark = pytest.mark.gpu

GUARD = 256
C_BLOCKS, C_ROWS, C_STATUS = 0xC3, 0x5E, 0x77  # canaries (0x77: neither status 0 nor -1)
FAMILY = {"LONGHAIR_AMD_JIT_DEFINES": "LH_FAMILY=1"}
FUSED_FAMILY = ["lh_jit_decode_fused(family)"]

# (id, k, m, bytes, stripes, env, decode kernels)
MIXED = [
    ("fused-1lane", 10, 4, 64, 150, {}, FUSED),       # one lane per stripe, 64 stripes per wave
    ("fused-k29", 29, 4, 1296, 50, {}, FUSED),        # three stripes per wave
    ("fused-64lane", 8, 4, 4096, 12, {}, FUSED),
    ("fused-family", 29, 4, 1312, 40, FAMILY, FUSED_FAMILY),
    ("fused-family-k4", 4, 5, 96, 70, FAMILY, FUSED_FAMILY),
    ("small4", 65, 4, 1296, 24, {}, SMALL4),          # slots 63 and 64: the planner's second pass
    ("small8", 10, 5, 64, 100, {}, SMALL8),
    ("small8-e8", 9, 8, 64, 100, {}, SMALL8),
    ("cf-jump", 9, 9, 64, 100, {}, GENERIC_CF),
    ("cf-jump-516", 40, 20, 4128, 8, {}, GENERIC_CF),
    ("workspace-sub3", 30, 13, 24, 40, {}, OLD_CF),
    ("workspace-513", 40, 20, 4104, 8, {}, OLD_CF),
    ("wide-m12", 40, 12, 2048, 8, {}, WIDE16),
    ("wide-m20", 40, 20, 4096, 8, {}, WIDE16),
    ("wide-m33", 40, 33, 2048, 8, {}, WIDE64),
    ("gen-s8", 20, 6, 64, 64, GEN, GENERIC_S8),
    ("gen-jump", 40, 4, 64, 64, GEN, PS4_JUMP),
    ("gen-jump2", 40, 4, 4160, 8, GEN, PS4_JUMP2),
    # in place with the last lane shifted back over its neighbour's bytes: sub 7 (dword lanes,
    # one byte back) and sub 524 (two-dword lanes, 4 bytes back)
    ("gen-jump-sub7", 40, 4, 56, 64, GEN, PS4_JUMP),
    ("gen-jump2-sub524", 40, 4, 4192, 8, GEN, PS4_JUMP2),
]
MIXED_IDS = [c[0] for c in MIXED]
BY_ID = {c[0]: c for c in MIXED}

# (id, k, m, bytes, stripes, env, encode kernels)
ENCODE = [
    ("win-m13", 40, 13, 2048, 8, {}, ["lh_jit_encode_win"]),
    ("win-m20", 40, 20, 4096, 8, {}, ["lh_jit_encode_win"]),
    ("jump", 10, 13, 64, 32, {}, JUMP),
    ("jump2", 40, 4, 4160, 8, GEN, JUMP2),
    ("bytewise", 30, 13, 24, 40, {}, ["lh_apply_generic_kernel"]),
    ("jump-shifted-lane", 40, 20, 4104, 8, {}, JUMP),   # sub 513: the last lane shifted back
    ("jump2-shifted-lane", 40, 4, 4128, 8, GEN, JUMP2),  # sub 516: the last two-dword lane shifted back
]


@pytest.fixture(scope="module")
def lh():
    import torch
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    import longhair_amd
    assert longhair_amd.cauchy_256_init() == 0
    return longhair_amd


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _encoded(oracle, k, m, nbytes, stripes, seed):
    """`stripes` stripes of lhutil.fill data and the oracle's recovery blocks (computed once
    per shape and seed, shared read-only)."""
    data = lhutil.fill(seed, stripes * k * nbytes).reshape(stripes, k, nbytes)
    rec = np.empty((stripes, m, nbytes), dtype=np.uint8)
    for s in range(stripes):
        rc, r = oracle.encode(k, m, data[s], nbytes)
        assert rc == 0
        rec[s] = r.reshape(m, nbytes)
    return _frozen(data, rec)


def pick_invalid(stripes, seed, mode="quarter"):
    """The invalid stripes of a batch: stripe 0, the last stripe, two adjacent interior
    stripes, and seeded-random others up to about a quarter of the batch."""
    if mode == "all":
        return list(range(stripes))
    if mode in ("none", "valid"):
        return []
    assert stripes >= 5, "a mixed batch needs room for four invalid stripes and a valid one"
    rng = np.random.Generator(np.random.PCG64(seed ^ 0x1234))
    a = int(rng.integers(1, stripes - 2))          # a, a + 1 interior
    bad = {0, stripes - 1, a, a + 1}
    want = max(len(bad), (stripes + 2) // 4)
    rest = [s for s in rng.permutation(stripes).tolist() if s not in bad]
    bad.update(rest[: want - len(bad)])
    return sorted(bad)


@functools.lru_cache(maxsize=None)
def mixed_case(oracle, k, m, nbytes, stripes, seed, mode="quarter"):
    """One batch's input and expected output: (blocks, rows, invalid mask, expected blocks,
    expected rows), the expectation computed once (the oracle on valid stripes only).
    mode 'quarter': a mixed batch; 'all': every stripe invalid; 'none': every stripe valid
    with e = 0 (nothing to recover, so nothing may change); 'valid': every stripe valid with
    the mixed batch's random e (m = 1, which accepts any rows, has no invalid stripe)."""
    data, rec = _encoded(oracle, k, m, nbytes, stripes, seed)
    bad = pick_invalid(stripes, seed, mode)
    if mode == "none":
        scen = [lhutil.erasure_case(seed * 131 + s, k, m, 0) for s in range(stripes)]
    else:
        scen = _scenarios(k, m, stripes, seed)   # (stripe 0, at e_max there, is invalid here)
        first = min(set(range(stripes)) - set(bad), default=None)
        if first is not None:
            scen[first] = lhutil.erasure_case(seed * 131 + first, k, m, min(k, m))
    blocks = np.empty((stripes, k, nbytes), dtype=np.uint8)
    rows = np.empty((stripes, k), dtype=np.uint8)
    for s, (slots, rws) in enumerate(scen):
        for i, (kind, x) in enumerate(slots):
            blocks[s, i] = data[s, x] if kind == "d" else rec[s, x]
        assert lhutil.rows_valid(rws, k, m)
        rows[s] = rws
    pairs = lhutil.invalid_pairs(k, m)
    rng = np.random.Generator(np.random.PCG64(seed + 99))
    for j, s in enumerate(bad):
        kind, where = pairs[(j + seed * len(lhutil.invalid_kinds(k, m))) % len(pairs)]
        rows[s] = lhutil.invalidate_rows(list(rows[s]), k, m, kind, where, rng)
        blocks[s] = lhutil.fill(seed * 7919 + 1000 + s, k * nbytes).reshape(k, nbytes)  # random bytes
    invalid = np.zeros(stripes, dtype=bool)
    invalid[bad] = True
    for s in range(stripes):
        assert lhutil.rows_valid(rows[s], k, m) == (not invalid[s]), s
    exp_blocks, exp_rows = blocks.copy(), rows.copy()
    for s in np.nonzero(~invalid)[0]:
        bufs = [blocks[s, i].copy() for i in range(k)]
        rc, r = oracle.decode(k, m, bufs, [int(x) for x in rows[s]], nbytes)
        assert rc == 0
        exp_blocks[s] = np.stack(bufs)
        exp_rows[s] = r
    return _frozen(blocks, rows, invalid, exp_blocks, exp_rows)


class Guarded:
    """A device allocation [guard | off | stripes x (payload + pad) | guard] filled with a
    canary, the payloads copied in; `check` wants every byte outside the payloads intact."""

    def __init__(self, payload, off, pad, canary, device="cuda"):
        import torch
        self.stripes, self.n = payload.shape
        self.off, self.stride, self.canary = off, self.n + pad, canary
        self.buf = torch.full((GUARD + off + self.stripes * self.stride + GUARD,), canary, dtype=torch.uint8,
                              device=device)
        self.view().copy_(torch.from_numpy(np.array(payload)).to(device))

    def view(self):
        return self.buf[GUARD + self.off:].as_strided((self.stripes, self.n), (self.stride, 1))

    @property
    def ptr(self):
        return self.buf.data_ptr() + GUARD + self.off

    def check(self, what):
        """Returns the payloads; asserts the front guard (with the offset head), the back
        guard and every stripe's pad bytes."""
        raw = self.buf.cpu().numpy()
        lo, hi = GUARD + self.off, GUARD + self.off + self.stripes * self.stride
        front = np.nonzero(raw[:lo] != self.canary)[0]
        assert front.size == 0, (what, "front guard written at", (front - lo).tolist()[:8])
        back = np.nonzero(raw[hi:] != self.canary)[0]
        assert back.size == 0, (what, "back guard written at +", back.tolist()[:8])
        body = raw[lo:hi].reshape(self.stripes, self.stride)
        pads = np.argwhere(body[:, self.n:] != self.canary)
        assert pads.size == 0, (what, "pad bytes written at (stripe, byte)", pads.tolist()[:8])
        return body[:, :self.n].copy()


def _set_env(monkeypatch, env):
    for key, v in env.items():
        monkeypatch.setenv(key, v)


def mixed_roundtrip(lh, oracle, k, m, nbytes, stripes, layout, seed, status=True, mode="quarter"):
    """cauchy_256_decode_batch (the C call, torch's current stream) on a batch of valid and
    invalid stripes between guards; see the module docstring.  `oracle` computes the expected
    stripes (once per shape, seed and mode).  Returns the launch trace."""
    import torch
    blocks, rows, invalid, exp_blocks, exp_rows = mixed_case(oracle, k, m, nbytes, stripes, seed, mode)
    off, pad = layout
    gb = Guarded(blocks.reshape(stripes, k * nbytes), off, pad, C_BLOCKS)
    gr = Guarded(rows.reshape(1, stripes * k), 0, 0, C_ROWS)
    gs = Guarded(np.full((1, stripes), C_STATUS, dtype=np.uint8), 0, 0, C_STATUS)
    torch.cuda.synchronize()
    rc = lh.lib().cauchy_256_decode_batch(k, m, nbytes, stripes, ctypes.c_void_p(gb.ptr),
                                          ctypes.c_longlong(gb.stride), ctypes.c_void_p(gr.ptr),
                                          ctypes.c_void_p(gs.ptr) if status else None,
                                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, (rc, lh.lib().cauchy_256_last_error())
    trace = lh.last_launch()
    torch.cuda.synchronize()
    tag = (k, m, nbytes, layout, trace)
    got = gb.check((tag, "blocks")).reshape(stripes, k, nbytes)
    got_rows = gr.check((tag, "rows")).reshape(stripes, k)
    got_status = gs.check((tag, "status")).reshape(stripes).view(np.int8)
    for s in range(stripes):
        what = (tag, "invalid" if invalid[s] else "valid", "stripe", s, "rows in", rows[s].tolist())
        assert got_rows[s].tolist() == exp_rows[s].tolist(), what
        wrong = [i for i in range(k) if got[s, i].tobytes() != exp_blocks[s, i].tobytes()]
        assert not wrong, (what, "slots", wrong)
    if status:
        assert got_status.tolist() == [-1 if b else 0 for b in invalid], tag
    else:
        assert (got_status.view(np.uint8) == C_STATUS).all(), tag
    return trace


def _run(lh, oracle, monkeypatch, name, layout, seed, status=True):
    _, k, m, nbytes, stripes, env, dec_k = BY_ID[name]
    _set_env(monkeypatch, env)
    trace = mixed_roundtrip(lh, oracle, k, m, nbytes, stripes, layout, seed, status)
    assert trace == dec_k, (name, trace)


def _seed(name):
    _, k, m, nbytes, _, _, _ = BY_ID[name]
    return k * 1000 + m * 10 + nbytes


@pytest.mark.parametrize("name", MIXED_IDS)
def test_mixed_batch(lh, oracle, monkeypatch, name):
    """Valid and invalid stripes in one batch through each decode family, packed stripes from
    an aligned base, a status array."""
    _run(lh, oracle, monkeypatch, name, (0, 0), _seed(name))


@pytest.mark.parametrize("name", MIXED_IDS)
def test_mixed_batch_odd_layout(lh, oracle, monkeypatch, name):
    """The same from an odd base (3 bytes in) with 5 pad bytes between stripes: every stripe's
    pad and both guards survive.  (Another seed: the cycle of (kind, position) pairs starts
    one diagonal on, so a small batch sees other pairs here than in test_mixed_batch.)"""
    _run(lh, oracle, monkeypatch, name, (3, 5), _seed(name) + 1)


@pytest.mark.parametrize("name", MIXED_IDS)  # (fused-k29, small8, cf-jump, workspace-sub3, wide-m20 and the rest)
def test_mixed_batch_no_status(lh, oracle, monkeypatch, name):
    """d_status = NULL (the header allows it): valid stripes still decode, invalid ones stay
    untouched, and the status array that was not passed is not written."""
    _run(lh, oracle, monkeypatch, name, (0, 0), _seed(name), status=False)


def test_all_invalid_and_none_invalid(lh, oracle, monkeypatch):
    """A batch whose every stripe is invalid, and one whose every stripe is valid with e = 0:
    neither changes a byte of blocks or rows (mixed_case expects the input back: no stripe
    goes to the oracle in the first, the oracle returns its input in the second)."""
    for name in ("small8", "wide-m20", "workspace-sub3"):
        _, k, m, nbytes, stripes, env, dec_k = BY_ID[name]
        for mode in ("all", "none"):
            blocks, rows, invalid, exp_blocks, exp_rows = mixed_case(oracle, k, m, nbytes, stripes, _seed(name), mode)
            assert invalid.all() if mode == "all" else not invalid.any()
            assert np.array_equal(blocks, exp_blocks) and np.array_equal(rows, exp_rows)
            trace = mixed_roundtrip(lh, oracle, k, m, nbytes, stripes, (3, 5), _seed(name), mode=mode)
            assert trace == dec_k, (name, mode, trace)


@pytest.mark.parametrize("layout", [(0, 0), (3, 5)], ids=["packed", "odd"])
@pytest.mark.parametrize("case", ENCODE, ids=[c[0] for c in ENCODE])
def test_encode_guards(lh, oracle, monkeypatch, case, layout):
    """cauchy_256_encode_batch with the data and the recovery blocks each between guards, at
    an offset and with a padded stride: the recovery blocks are the oracle's, the data buffer
    is byte-identical afterwards (guards and pad bytes included), and the recovery buffer's
    guards and pad bytes are intact."""
    import torch
    name, k, m, nbytes, stripes, env, enc_k = case
    _set_env(monkeypatch, env)
    off, pad = layout
    data, rec = _encoded(oracle, k, m, nbytes, stripes, k * 1000 + m * 10 + nbytes)
    gd = Guarded(data.reshape(stripes, k * nbytes), off, pad, C_BLOCKS)
    go = Guarded(np.full((stripes, m * nbytes), C_ROWS, dtype=np.uint8), off, pad, C_ROWS)
    before = gd.buf.cpu().numpy()
    rc = lh.lib().cauchy_256_encode_batch(k, m, nbytes, stripes, ctypes.c_void_p(gd.ptr), ctypes.c_longlong(gd.stride),
                                          ctypes.c_void_p(go.ptr), ctypes.c_longlong(go.stride),
                                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, (rc, lh.lib().cauchy_256_last_error())
    trace = lh.last_launch()
    torch.cuda.synchronize()
    assert trace == enc_k, (name, trace)
    got = go.check((name, layout, "recovery")).reshape(stripes, m, nbytes)
    for s in range(stripes):
        wrong = [r for r in range(m) if got[s, r].tobytes() != rec[s, r].tobytes()]
        assert not wrong, (name, layout, "stripe", s, "recovery blocks", wrong)
    assert np.array_equal(gd.buf.cpu().numpy(), before), (name, layout, "the data buffer was written")
