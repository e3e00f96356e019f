"""CPU-only checks of the C-ABI boundary (no compute without a GPU)."""
import ctypes
import os
import re

import pytest

import lhutil

REPO = lhutil.REPO


def _declared_functions(headers=("cauchy_256.h", "cauchy_256_batch.h", "cauchy_256_dispatch.h")):
    names = set()
    for h in headers:
        text = open(os.path.join(REPO, "include", h)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        for m in re.finditer(r"^\s*(?:extern\s+)?(?:const\s+)?\w+\s*\*?\s*(\w+)\s*\(", text, flags=re.M):
            names.add(m.group(1))
    return names


def test_headers_declare_reference_entry_points():
    names = _declared_functions()
    for ref_name in ("_cauchy_256_init", "cauchy_256_encode", "cauchy_256_decode"):
        assert ref_name in names
    assert {"cauchy_256_encode_batch", "cauchy_256_decode_batch"} <= names


def test_library_exports_every_declared_symbol():
    import longhair_amd
    from longhair_amd import _native
    lib = ctypes.CDLL(_native.library_path)
    for name in _declared_functions():
        assert hasattr(lib, name), name
    assert set(_native.EXPORTS) == _declared_functions()
    assert longhair_amd.lib() is not None
    # the test-only header's hooks: in the checked build, not in the product
    hooks = _declared_functions(("cauchy_256_test.h",))
    assert set(_native.OPTIONAL_EXPORTS) == hooks
    check = ctypes.CDLL(os.path.join(os.path.dirname(_native.library_path), "liblonghair_amd_check.so"))
    for name in hooks:
        assert hasattr(check, name) and not hasattr(lib, name), name


def test_jit_knobs_match_integration_doc():
    """The `#ifndef LH_*` tunables of jit_codec.hip are exactly the knobs INTEGRATION.md section 6
    lists for it: a knob added to, or deleted from, one of the two shows up here."""
    csrc = os.path.join(REPO, "longhair_amd", "csrc")
    source = open(os.path.join(csrc, "jit_codec.hip")).read()
    in_file = set(re.findall(r"^\s*#\s*ifndef\s+(LH_\w+)", source, flags=re.M))
    # not tunables: the guards of what jit.cpp defines for every module (the shape, the role)
    shape = {"LH_K", "LH_ROLE"}
    host = open(os.path.join(csrc, "jit.cpp")).read()
    assert all("#define %s " % name in host for name in shape)
    assert shape <= in_file
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    section = doc[doc.index("## 6. Environment knobs"):]
    para = section[section.index("knobs of `jit_codec.hip`:"):]
    para = para[:para.index("\n\n")]
    in_doc = set(re.findall(r"`(LH_\w+)(?:=\w+)?`", para))
    assert in_doc, "INTEGRATION.md section 6: the jit_codec.hip knob paragraph was not found"
    assert in_file - shape == in_doc, (sorted(in_file - shape - in_doc), sorted(in_doc - in_file))


def test_block_layout_matches_reference():
    import longhair_amd
    assert ctypes.sizeof(longhair_amd.Block) == 16
    assert longhair_amd.Block.row.offset == 8


def test_version_mismatch_rejected_without_gpu():
    import longhair_amd
    assert longhair_amd._cauchy_256_init(1) == -1


def test_specialisation_policy():
    import longhair_amd
    assert longhair_amd.batch_path(29, 4, 1296) == "jit"
    assert longhair_amd.batch_path(29, 4, 1296, decode=True) == "jit-fused"
    assert longhair_amd.batch_path(29, 8, 1296, decode=True) == "jit"
    assert longhair_amd.batch_path(128, 32, 8192) == "jit-win"
    assert longhair_amd.batch_path(128, 32, 8192, decode=True) == "jit-wide"
    assert longhair_amd.batch_path(128, 32, 1000) == "generic"


# (k, m, bytes, what, code): cauchy_256_batch_path on both sides of each boundary of the batch
# routes, recorded from the library before codec.cpp's routes were collapsed into one function
# (what 0 / 1: encode / decode path, 2 / 5: LDS staging, 8 / 9: block-size family; 10 / 11, added
# later: the stripes per workgroup of the specialised encode / decode, test_stripes_per_workgroup).
CLASSIFICATION = [
    (29, 4, 1296, 0, 1), (29, 4, 1296, 1, 2), (29, 8, 1296, 1, 1),
    (64, 4, 1296, 1, 2), (65, 4, 1296, 1, 1),          # fused plan: k <= 64
    (8, 4, 4096, 1, 2), (8, 3, 8128, 1, 1),            # ... one stripe per <= 64 lanes
    (4, 8, 64, 1, 2), (5, 8, 64, 1, 1), (10, 4, 64, 1, 2), (10, 5, 64, 1, 1),  # ... e_max <= 4
    (9, 8, 64, 1, 1), (9, 9, 64, 1, 0),                # specialised decode: e_max * m <= 64
    (40, 12, 2048, 0, 1), (40, 13, 2048, 0, 3),        # register network: m <= 12, else windowed
    (10, 12, 64, 0, 1), (10, 13, 64, 0, 0),            # ... or generic (sub % 256 != 0)
    (20, 64, 2048, 1, 4), (20, 65, 2048, 1, 0), (20, 65, 2048, 0, 3),  # windowed decode: m <= 64
    (40, 20, 4096, 1, 4), (40, 20, 4104, 1, 0), (40, 20, 4096, 0, 3), (40, 20, 4104, 0, 0),
    (128, 4, 1296, 0, 1), (129, 4, 1296, 0, 0),        # register network: k <= 128
    (128, 32, 8192, 0, 3), (128, 32, 8192, 1, 4),
    (200, 56, 2048, 0, 3), (200, 57, 2048, 0, 0),      # k + m <= 256
    (29, 4, 1300, 0, 0),                               # bytes % 8
    (29, 4, 1296, 2, 1), (29, 4, 1304, 2, 0), (29, 4, 1040, 2, 0), (29, 8, 1296, 2, 0),
    (64, 4, 64, 2, 0), (64, 4, 4096, 5, 1),
    (29, 4, 1296, 8, 1), (29, 4, 1304, 8, 0), (29, 4, 4096, 8, 1), (29, 4, 4112, 8, 0),
    (29, 6, 1296, 8, 1), (29, 7, 1296, 8, 0), (3, 4, 1296, 8, 0),
    (29, 4, 1296, 9, 1), (29, 5, 1296, 9, 0), (29, 4, 192, 9, 0), (64, 4, 1296, 9, 1), (65, 4, 1296, 9, 0),
]


def test_classification_table():
    import longhair_amd
    path = longhair_amd.lib().cauchy_256_batch_path
    got = [(k, m, b, what, path(k, m, b, what)) for k, m, b, what, _ in CLASSIFICATION]
    assert got == CLASSIFICATION


def test_stripes_per_workgroup(monkeypatch):
    """cauchy_256_batch_path what = 10 / 11: the stripes one workgroup of the strided specialised
    encode / decode covers (stripes per wave x waves per workgroup, codec.cpp jit_encode_blocks /
    jit_blocks), from the configuration alone -- tests/test_gpu_stripe_counts.py sizes its sweeps
    by it."""
    import longhair_amd
    path = longhair_amd.lib().cauchy_256_batch_path
    spw = longhair_amd.stripes_per_workgroup
    assert [path(10, 4, 64, w) for w in (10, 11)] == [256, 256]        # one lane per stripe: 64 x 4 waves
    assert [path(29, 4, 1296, w) for w in (10, 11)] == [12, 12]        # nch 21: 3 stripes per wave
    assert [path(8, 4, 4096, w) for w in (10, 11)] == [4, 4]           # nch 64: one stripe per wave
    assert path(64, 4, 4096, 11) == 4
    # m = 3 at 8128 bytes: the encode's 16-byte lanes fill one wave (nch 64), the decode's 8-byte
    # lanes (a fourth accumulator row) take two waves per stripe (nch 127)
    assert [path(8, 3, 8128, w) for w in (10, 11)] == [4, 1]
    assert [path(40, 13, 2048, 10), path(40, 12, 2048, 11)] == [1, 1]  # the windowed kernels
    assert path(65, 4, 64, 11) == 256 and path(10, 5, 64, 11) == 256   # lh_jit_decode after the planner
    assert path(65, 4, 1296, 11) == 12
    # no specialised configuration: 0
    assert [path(9, 9, 64, 11), path(10, 13, 64, 10), path(129, 4, 1296, 10), path(29, 4, 1300, 11)] == [0, 0, 0, 0]
    assert path(10, 1, 100, 10) == 0 and path(1, 3, 40, 11) == 0
    assert spw(29, 4, 1296) == 12 and spw(29, 4, 1296, decode=True) == 12 and spw(9, 9, 64, True) == 0
    # the block-size family's kernels under the define the tests force them with
    monkeypatch.setenv("LONGHAIR_AMD_JIT_DEFINES", "LH_FAMILY=1")
    assert [path(29, 4, 1312, w) for w in (10, 11)] == [12, 12]        # 8-byte lanes, nch 21
    assert path(4, 5, 96, 11) == 128                                   # nch 2: 32 stripes per wave
    monkeypatch.delenv("LONGHAIR_AMD_JIT_DEFINES")
    monkeypatch.setenv("LONGHAIR_AMD_PATH", "generic")
    assert [path(10, 4, 64, w) for w in (10, 11)] == [0, 0]


def test_stripes_per_wave(monkeypatch):
    """cauchy_256_batch_path what = 12 / 13: the whole stripes one wave of the strided specialised
    encode / decode covers (jit.cpp cfg.spw), 0 when a stripe spans waves or nothing is specialised
    -- route()'s range test multiplies the stride by it, and tests/test_gpu_far.py computes the
    largest admitted and the first refused stride from it.  For every register-network case of
    the kernel catalogue (tests/test_gpu_stripe_counts.py) the workgroup figure of what = 10 / 11
    is this one times the waves of a workgroup (four for the decode)."""
    import longhair_amd
    import test_gpu_stripe_counts as sc
    from test_gpu_far import _is_register
    path = longhair_amd.lib().cauchy_256_batch_path
    spw = longhair_amd.stripes_per_wave
    assert [path(10, 4, 64, w) for w in (12, 13)] == [64, 64]
    assert [path(29, 4, 1296, w) for w in (12, 13)] == [3, 3]
    assert [path(8, 3, 8128, w) for w in (12, 13)] == [1, 0]           # decode: two waves per stripe
    assert [path(40, 13, 2048, 12), path(40, 12, 2048, 13)] == [0, 0]  # the windowed kernels
    assert [path(9, 9, 64, 13), path(10, 13, 64, 12), path(10, 1, 100, 12), path(1, 3, 40, 13)] == [0, 0, 0, 0]
    assert spw(29, 4, 1296) == 3 and spw(65, 4, 64, decode=True) == 64
    checked = 0
    for decode, cases in ((True, sc.DECODE), (False, sc.ENCODE)):
        for case in cases:
            if not _is_register(case):
                continue
            with monkeypatch.context() as mp:
                for key, v in case.env.items():
                    mp.setenv(key, v)
                k, m, b = (case.k, case.m, case.nbytes) if case.k is not None else sc._sample_shape(longhair_amd, case.id)
                T, w = longhair_amd.stripes_per_workgroup(k, m, b, decode), spw(k, m, b, decode)
                assert T >= 1 and w >= 0, (case.id, T, w)
                if decode:
                    assert T == (w * 4 if w else 1), (case.id, T, w)
                else:
                    assert (T % w == 0 and 1 <= T // w <= 8) if w else T == 1, (case.id, T, w)
                checked += 1
    assert checked == 15
    monkeypatch.setenv("LONGHAIR_AMD_PATH", "generic")
    assert [path(10, 4, 64, w) for w in (12, 13)] == [0, 0]


def test_lds_staging_policy():
    """jit.cpp jit_config_for: the register networks stage their columns by LDS-DMA for 8-byte
    lanes, whole stripes per wave and 16-byte-multiple blocks, unless a stripe's partial last
    lane would open a 16-lane DPP row (its stores funnel the previous lane's word) or the
    encode's ring plus its stripes' block-pointer rows would not fit two workgroups per CU."""
    import longhair_amd
    assert longhair_amd.lds_staged(29, 4, 1296)        # nch 21, spw 3: last lanes 20, 41, 62
    assert longhair_amd.lds_staged(64, 4, 4096)        # nch 64: the last lane is whole
    assert not longhair_amd.lds_staged(29, 4, 1304)    # 1304 % 16 = 8: a chunk would span blocks
    assert not longhair_amd.lds_staged(29, 4, 1040)    # nch 17, spw 3: lane 16 is a last lane
    assert not longhair_amd.lds_staged(29, 8, 1296)    # m = 8: 4-byte lanes
    assert not longhair_amd.lds_staged(100, 12, 800)   # no register network
    assert not longhair_amd.lds_staged(64, 4, 64)      # spw 64: the encode's pointer rows would not fit


def test_no_device_gpu_policy_fails_loudly():
    """Without a GPU: under the GPU dispatch policy every drop-in call fails with -2 and
    writes nothing; batch calls always need a device (test_launch_trace_empty_without_gpu)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import numpy as np
    import longhair_amd
    k, m, nbytes = 4, 2, 16
    data = lhutil.fill(1, k * nbytes)
    ptrs = (ctypes.POINTER(ctypes.c_ubyte) * k)()
    for x in range(k):
        ptrs[x] = ctypes.cast(data.ctypes.data + x * nbytes, ctypes.POINTER(ctypes.c_ubyte))
    rec = np.zeros(m * nbytes, dtype=np.uint8)
    prev = longhair_amd.set_dispatch("gpu")
    try:
        assert longhair_amd.cauchy_256_init() == -2
        assert longhair_amd.cauchy_256_encode(k, m, ptrs, rec, nbytes) == -2
        assert not rec.any()
    finally:
        longhair_amd.set_dispatch(prev)


def _golden(name):
    import json
    return json.load(open(os.path.join(lhutil.GOLDEN, name)))


@pytest.mark.parametrize("policy", ["auto", "host"])
def test_no_device_dropin_on_host_engine(policy):
    """VERDICT r4 missing #3 (cauchy_256.cpp:390-399 initialises on any CPU): in a process
    without a HIP device, init succeeds under the AUTO and HOST policies and the drop-in calls
    run on the library's host SIMD engine -- checked through the C ABI against every fixture
    the reference produced (encode grid digests, full-byte vectors, decode scenarios)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the drop-in calls are tested on the device (tests/test_gpu_parity.py)")
    import numpy as np
    import longhair_amd
    from longhair_amd import _native
    lib = longhair_amd.lib()
    prev = longhair_amd.set_dispatch(policy)
    try:
        assert longhair_amd.cauchy_256_init() == 0
        assert b"host engine" in lib.cauchy_256_last_error()
        codec = lhutil._Codec(ctypes.CDLL(_native.library_path), lib.cauchy_256_encode, lib.cauchy_256_decode)
        for k, m, bytes_, seed, rc, digest in _golden("encode_grid.json")["cases"]:
            got_rc, rec = codec.encode(k, m, lhutil.fill(seed, k * bytes_), bytes_)
            assert got_rc == rc, (k, m, bytes_)
            assert lhutil.h64(rec if rc == 0 else rec[:bytes_]) == digest, (k, m, bytes_)
        for c in _golden("encode_full.json"):
            rc, rec = codec.encode(c["k"], c["m"], np.frombuffer(bytes.fromhex(c["data"]), dtype=np.uint8), c["bytes"])
            assert rc == c["rc"] and rec.tobytes().hex() == c["recovery"]
        for c in _golden("decode_cases.json"):
            k, m, bytes_ = c["k"], c["m"], c["bytes"]
            data = lhutil.fill(c["seed"], k * bytes_).reshape(k, bytes_)
            rc_e, rec = codec.encode(k, m, data, bytes_)
            assert rc_e == c["rc_encode"], c["tag"]
            rec = rec.reshape(m, bytes_)
            bufs = [(data[x] if kind == "d" else rec[x]).copy() for kind, x in c["slots"]]
            rc, rows = codec.decode(k, m, bufs, list(c["rows_in"]), bytes_)
            assert rc == c["rc"] and rows == c["rows_out"], c["tag"]
            assert [lhutil.h64(b) for b in bufs] == c["digests"], c["tag"]
        assert longhair_amd.last_launch() == []   # nothing ran on a device
    finally:
        longhair_amd.set_dispatch(prev)


def test_no_exception_crosses_the_abi():
    """SURVEY 8(b) / VERDICT r4 weak #7: an exception thrown inside any entry point (here
    injected by the test-only hook at the start of the guarded body) comes back as -3 with
    cauchy_256_last_error() naming it, never as std::terminate in the caller."""
    import longhair_amd
    from longhair_amd import _native
    # the hook is built into the checked library only (LH_TEST_HOOKS); the product has none
    assert not hasattr(longhair_amd.lib(), "cauchy_256_debug_throw_next")
    check = os.path.join(os.path.dirname(longhair_amd.library_path), "liblonghair_amd_check.so")
    assert os.path.exists(check), "build the checked library (__graft_entry__.build())"
    lib = _native.bind(ctypes.CDLL(check))
    buf = (ctypes.c_ubyte * 64)()
    tab = (ctypes.c_void_p * 8)()
    blocks = (lhutil.Block * 4)()
    policy = lib.cauchy_256_get_dispatch()
    calls = {
        "_cauchy_256_init": lambda: lib._cauchy_256_init(2),
        "cauchy_256_encode": lambda: lib.cauchy_256_encode(4, 2, tab, buf, 16),
        "cauchy_256_decode": lambda: lib.cauchy_256_decode(4, 2, blocks, 16),
        "cauchy_256_encode_batch": lambda: lib.cauchy_256_encode_batch(4, 2, 16, 1, buf, 64, buf, 32, None),
        "cauchy_256_decode_batch": lambda: lib.cauchy_256_decode_batch(4, 2, 16, 1, buf, 64, buf, None, None),
        "cauchy_256_encode_batch_ptrs": lambda: lib.cauchy_256_encode_batch_ptrs(4, 2, 16, 1, tab, tab, None),
        "cauchy_256_decode_batch_ptrs": lambda: lib.cauchy_256_decode_batch_ptrs(4, 2, 16, 1, tab, buf, None, None),
        "cauchy_256_encode_host_batch": lambda: lib.cauchy_256_encode_host_batch(4, 2, 16, 1, buf, 64, buf, 32, 0),
        "cauchy_256_decode_host_batch": lambda: lib.cauchy_256_decode_host_batch(4, 2, 16, 1, buf, 64, buf, None, 0),
        "cauchy_256_batch_prepare": lambda: lib.cauchy_256_batch_prepare(4, 2, 16, 1),
        "cauchy_256_batch_prepare_ptrs": lambda: lib.cauchy_256_batch_prepare_ptrs(4, 2, 16),
        "cauchy_256_batch_prepare_stream": lambda: lib.cauchy_256_batch_prepare_stream(4, 2, 16, 1, None),
        "cauchy_256_batch_path": lambda: lib.cauchy_256_batch_path(4, 2, 16, 0),
        "cauchy_256_jit_precompile": lambda: lib.cauchy_256_jit_precompile(4, 2, 16),
        "cauchy_256_frame_batch": lambda: lib.cauchy_256_frame_batch(4, 2, 16, 1, buf, 64, buf, 32, buf, 102, None),
        "cauchy_256_unframe_batch": lambda: lib.cauchy_256_unframe_batch(4, 16, 1, buf, 68, buf, 64, buf, None),
        "cauchy_256_set_dispatch": lambda: lib.cauchy_256_set_dispatch(policy, -1),
        "cauchy_256_get_dispatch": lambda: lib.cauchy_256_get_dispatch(),
    }
    for name, call in calls.items():
        lib.cauchy_256_debug_throw_next()
        assert call() == -3, name
        assert b"injected" in lib.cauchy_256_last_error(), name
    # every int-returning entry point the headers declare is covered
    ints = {n for n, (res, _) in __import__("longhair_amd._native", fromlist=["EXPORTS"]).EXPORTS.items()
            if res is ctypes.c_int}
    assert ints == set(calls)


def test_dispatch_policy_api():
    import longhair_amd
    if "LONGHAIR_AMD_DISPATCH" not in os.environ:
        assert longhair_amd.dispatch_policy() == "auto"  # default: small host calls stay on the host
    prev = longhair_amd.set_dispatch("gpu")
    assert longhair_amd.dispatch_policy() == "gpu"
    assert longhair_amd.set_dispatch("auto") == "gpu"
    assert longhair_amd.set_dispatch(prev) == "auto"
    assert longhair_amd.lib().cauchy_256_set_dispatch(7, -1) == -1
    assert longhair_amd.host_isa() in ("avx512bw", "avx2", "scalar")


def test_launch_trace_empty_without_gpu():
    """cauchy_256_last_launch names the kernels of the last call; a call that fails before
    any launch (no device here) leaves it empty."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import longhair_amd
    rc = longhair_amd.lib().cauchy_256_encode_batch(4, 2, 16, 1, None, 64, None, 32, None)
    assert rc == -2
    assert longhair_amd.last_launch() == []


def test_pointer_table_calls_validate_before_the_device():
    """cauchy_256_{encode,decode}_batch_ptrs: parameter checks as the strided calls, before any
    device work (so they hold without a GPU); a call with work and no device fails loudly."""
    import torch
    import longhair_amd
    lib = longhair_amd.lib()
    tab = (ctypes.c_void_p * 8)()
    rows = (ctypes.c_ubyte * 8)()
    assert lib.cauchy_256_encode_batch_ptrs(4, 2, 16, 0, tab, tab, None) == 0      # no stripes: nothing to do
    assert lib.cauchy_256_encode_batch_ptrs(0, 2, 16, 1, tab, tab, None) == -1     # k < 1
    assert lib.cauchy_256_encode_batch_ptrs(4, 257, 16, 1, tab, tab, None) == -1   # m > 256
    assert lib.cauchy_256_encode_batch_ptrs(4, 2, 16, 1, None, tab, None) == -1    # no table
    assert lib.cauchy_256_decode_batch_ptrs(4, 2, 16, 0, tab, rows, None, None) == 0
    assert lib.cauchy_256_decode_batch_ptrs(4, 2, 12, 1, tab, rows, None, None) == -1  # bytes % 8, m > 1
    assert lib.cauchy_256_decode_batch_ptrs(250, 7, 16, 1, tab, rows, None, None) == -1  # k + m > 256
    assert lib.cauchy_256_decode_batch_ptrs(4, 2, 16, 1, None, rows, None, None) == -1
    assert lib.cauchy_256_decode_batch_ptrs(4, 2, 16, 1, tab, None, None, None) == -1
    if not torch.cuda.is_available():
        assert lib.cauchy_256_encode_batch_ptrs(4, 2, 16, 1, tab, tab, None) == -2
        assert lib.cauchy_256_decode_batch_ptrs(4, 2, 16, 1, tab, rows, None, None) == -2
        assert longhair_amd.last_launch() == []


def test_inv_jump_table_is_generated():
    """inv_jump.inc (the computed-jump bodies of lh_inverse_gt_kernel) is exactly what
    tools/gen_inv_jump.py renders: no hand edits, no stale generator."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_inv_jump", os.path.join(REPO, "tools", "gen_inv_jump.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    committed = open(os.path.join(REPO, "longhair_amd", "csrc", "inv_jump.inc")).read()
    assert committed == gen.render()
    # two one-dword tables (in-asm indexed for 8 outputs; once per code object) of 256 bodies
    # of 8 v_bitop3_b32 + a return (the fixed 68-byte stride the jump assumes) and the
    # two-dword table of 256 bodies of 16 (132 bytes)
    assert committed.count("v_bitop3_b32") == 2 * 256 * 8 + 256 * 16
    assert committed.count("s_setpc_b64 s[94:95]") == 3 * 256
    # every call statement (1..8 outputs, two-dword 1..4) turns GPR indexing on once and off
    # once, and restores M0 (no path leaves the statement with indexing on)
    assert committed.count("lh_inv_gtab:") == 1 and committed.count("lh_inv_gtab2:") == 1
    assert committed.count("s_set_gpr_idx_on 0, gpr_idx(SRC2,DST)") == 8 + 4
    assert committed.count("s_set_gpr_idx_off") == 8 + 4 + 1 and committed.count("s_mov_b32 m0, s97") == 8 + 4 + 1
