"""The decode of the C oracle, and of the host engine, over the deterministic erasure patterns
of tests/test_gpu_patterns.py (every pattern x placement of each of its codes, 8-byte blocks).

Every GPU decode test takes the oracle's decode as truth.  It is pinned to the reference here:
directly where the reference build is present, and through tests/golden/decode_patterns.json
(one digest per code, recorded from the reference by tools/make_golden.py) everywhere.  For
k, m > 1 the result is also checked for what a decode means: rows out is a permutation of
0..k-1 and the slot whose row is now r holds original r.  (m = 1 with nothing erased is the
reference's known quirk -- a block is overwritten -- so there its bytes are the only rule.)
No GPU needed."""
import ctypes
import json
import os

import numpy as np
import pytest

import lhutil
import test_gpu_patterns as tp

IDS = [f"{kind}-k{k}m{m}" for k, m, kind, _ in tp.CODES]
RECORDS = {(r["k"], r["m"], r["set"]): r
           for r in json.load(open(os.path.join(lhutil.GOLDEN, "decode_patterns.json")))["codes"]}


def first_difference(cases, a, b):
    """The first case at which two (return codes, rows out, blocks out) differ, named."""
    bad = (a[0] != b[0]) | (a[1] != b[1]).any(axis=1) | (a[2] != b[2]).any(axis=(1, 2))
    if not bad.any():
        return None
    s = int(np.argmax(bad))
    E, R, label, _, rows = cases[s]
    return {"differing": int(bad.sum()), "case": s, "E": list(E), "R": list(R), "placement": label, "rows in": rows,
            "rc": (int(a[0][s]), int(b[0][s])), "rows out": (a[1][s].tolist(), b[1][s].tolist())}


def test_golden_records_are_the_codes_table():
    assert sorted(RECORDS) == sorted((k, m, kind) for k, m, kind, _ in tp.CODES)
    assert os.path.getsize(os.path.join(lhutil.GOLDEN, "decode_patterns.json")) < 16 << 10


@pytest.mark.parametrize("k,m,kind,keep", tp.CODES, ids=IDS)
def test_oracle_reproduces_reference_digest(oracle, k, m, kind, keep):
    """The oracle's return codes, rows out and bytes over all cases hash to what the reference
    produced; and for k, m > 1 every stripe holds its originals."""
    rec = RECORDS[(k, m, kind)]
    cases, rcs, rows_out, blocks_out = tp.cpu_decode(oracle, k, m, kind)
    assert (rec["bytes"], rec["seed"], rec["placements"]) == (tp.CPU_BYTES, tp.seed_of(k, m), keep)
    assert rec["patterns"] == len(tp.patterns_of(k, m, kind)) == len({(c[0], c[1]) for c in cases})
    assert rec["stripes"] == len(cases)
    assert (rcs == 0).all()
    assert lhutil.pattern_digest(rcs, rows_out, blocks_out) == rec["h64"], (k, m, kind)
    if k > 1 and m > 1:
        assert (np.sort(rows_out, axis=1) == np.arange(k)).all()
        data = lhutil.pattern_data(k, tp.CPU_BYTES, len(cases), tp.seed_of(k, m))
        want = data[(np.arange(len(cases)) % data.shape[0])[:, None], rows_out.astype(np.intp)]
        bad = (blocks_out != want).any(axis=(1, 2))
        assert not bad.any(), (k, m, "first case not holding its originals", cases[int(np.argmax(bad))][:3])


@pytest.mark.skipif(not os.path.exists(lhutil.REF_SO), reason="reference build absent")
@pytest.mark.parametrize("k,m,kind,keep", tp.CODES, ids=IDS)
def test_oracle_vs_reference_decode(oracle, k, m, kind, keep):
    """Return code, rewritten rows and bytes of every case, the oracle against the reference
    itself; the committed digest is what the reference gives now."""
    ref = lhutil.RefLib()
    cases, *got = tp.cpu_decode(oracle, k, m, kind)
    _, *want = tp.cpu_decode(ref, k, m, kind)
    assert first_difference(cases, got, want) is None, (k, m, first_difference(cases, got, want))
    assert lhutil.pattern_digest(*want) == RECORDS[(k, m, kind)]["h64"]


HOST_CODES = [(4, 4, "x"), (6, 4, "x"), (5, 5, "x"), (8, 1, "x"), (29, 4, "d"), (65, 4, "d"), (40, 20, "d"),
              (128, 32, "d")]


def test_no_device_decode_patterns_on_host_engine(oracle, monkeypatch):
    """In a process without a HIP device (as test_abi.test_no_device_dropin_on_host_engine):
    cauchy_256_decode under the HOST policy, at every instruction-set level the CPU has, gives
    the oracle's return code, rows and bytes on every case of HOST_CODES."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the drop-in calls are tested on the device (tests/test_gpu_patterns.py)")
    import longhair_amd
    from longhair_amd import _native
    lib = longhair_amd.lib()
    monkeypatch.delenv("LONGHAIR_AMD_HOST_ISA", raising=False)
    best = longhair_amd.host_isa()
    levels = ["avx512bw", "avx2", "scalar"]
    levels = levels[levels.index(best):]
    prev = longhair_amd.set_dispatch("host")
    try:
        assert longhair_amd.cauchy_256_init() == 0
        codec = lhutil._Codec(ctypes.CDLL(_native.library_path), lib.cauchy_256_encode, lib.cauchy_256_decode)
        for k, m, kind in HOST_CODES:
            if (k, m, kind) in tp.KEEP:
                cases_of = tp.cases_of
            else:   # a code of this test alone: every placement
                def cases_of(k, m, kind):
                    return lhutil.pattern_cases(k, m, tp.patterns_of(k, m, kind), tp.seed_of(k, m))
            cases = cases_of(k, m, kind)
            blocks, rows = lhutil.pattern_batch(oracle, k, m, tp.CPU_BYTES, cases, tp.seed_of(k, m))
            want = lhutil.decode_all(oracle, k, m, blocks, rows, tp.CPU_BYTES)
            for isa in levels:
                monkeypatch.setenv("LONGHAIR_AMD_HOST_ISA", isa)
                assert longhair_amd.host_isa() == isa
                got = lhutil.decode_all(codec, k, m, blocks, rows, tp.CPU_BYTES)
                diff = first_difference(cases, got, want)
                assert diff is None, (k, m, isa, diff)
        assert longhair_amd.last_launch() == []   # nothing ran on a device
    finally:
        longhair_amd.set_dispatch(prev)
