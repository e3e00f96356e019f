"""CPU-only checks of the locate boundary (include/cauchy_256_locate.h): the exports, every
parameter rule (they come before any device work, so they hold without a GPU), the exception
barrier of the checked library and the argument checks of the Python wrappers."""
import ctypes
import os

import pytest

import lhutil
from test_abi import _declared_functions
from test_update_abi import _check_lib, _device_like

HEADER = ("cauchy_256_locate.h",)
NAMES = {"cauchy_256_locate_batch", "cauchy_256_locate_batch_ptrs"}


def test_locate_header_symbols_are_exported():
    import longhair_amd
    from longhair_amd import _native
    names = _declared_functions(HEADER)
    assert names == NAMES
    assert set(_native.LOCATE_EXPORTS) == names
    for older in (_native.EXPORTS, _native.OPTIONAL_EXPORTS, _native.UPDATE_EXPORTS, _native.VERIFY_EXPORTS,
                  _native.RECONSTRUCT_EXPORTS):
        assert not names & set(older)
    for path in (_native.library_path, _check_lib()):
        lib = ctypes.CDLL(path)
        for name in names:
            assert hasattr(lib, name), (path, name)
    bound = longhair_amd.lib()
    for name, (res, args) in _native.LOCATE_EXPORTS.items():
        assert getattr(bound, name).restype is res and getattr(bound, name).argtypes == args, name


def test_older_export_tables_are_unchanged():
    from longhair_amd import _native
    assert set(_native.EXPORTS) == _declared_functions()
    assert set(_native.OPTIONAL_EXPORTS) == {"cauchy_256_debug_throw_next"}
    assert set(_native.UPDATE_EXPORTS) == _declared_functions(("cauchy_256_update.h",))
    assert set(_native.VERIFY_EXPORTS) == _declared_functions(("cauchy_256_verify.h",))
    assert set(_native.RECONSTRUCT_EXPORTS) == _declared_functions(("cauchy_256_reconstruct.h",))
    assert os.path.exists(os.path.join(lhutil.REPO, "include", HEADER[0]))


def test_header_states_the_contract():
    text = open(os.path.join(lhutil.REPO, "include", HEADER[0])).read()
    for phrase in ("0xFF", "replacing block x ALONE", "m + 1", "lh_locate_kernel", "lh_locate_finish_kernel", "k + m > 255"):
        assert phrase in text, phrase


def _strided(lib, k=4, m=2, nbytes=16, stripes=1, data=True, rec=True, status=True, rows=True,
             data_stride=None, rec_stride=None):
    buf = (ctypes.c_ubyte * 64)()
    on = lambda flag: buf if flag else None   # noqa: E731
    return lib.cauchy_256_locate_batch(k, m, nbytes, stripes, on(data),
                                       max(k, 0) * max(nbytes, 0) if data_stride is None else data_stride, on(rec),
                                       max(m, 0) * max(nbytes, 0) if rec_stride is None else rec_stride,
                                       on(status), on(rows), None)


def _table(lib, k=4, m=2, nbytes=16, stripes=1, data=True, rec=True, status=True, rows=True):
    buf = (ctypes.c_ubyte * 64)()
    tab = (ctypes.c_void_p * 8)()
    return lib.cauchy_256_locate_batch_ptrs(k, m, nbytes, stripes, tab if data else None, tab if rec else None,
                                            buf if status else None, buf if rows else None, None)


INVALID = [
    dict(k=0), dict(m=0), dict(k=-1), dict(m=-3), dict(k=257, m=1), dict(k=1, m=257),
    dict(nbytes=0), dict(nbytes=-8), dict(stripes=-1),
    dict(k=250, m=7), dict(k=255, m=2), dict(nbytes=12), dict(k=2, m=2, nbytes=13),
    dict(k=254, m=2), dict(k=200, m=56), dict(k=128, m=128), dict(k=1, m=255), dict(k=1, m=256),   # k + m == 256 and past it, m >= 2
    dict(k=254, m=2, stripes=0), dict(k=1, m=255, stripes=0),
    dict(status=False), dict(rows=False), dict(status=False, rows=False),
    dict(status=False, stripes=0), dict(rows=False, stripes=0),
    dict(data=False), dict(rec=False),
]
INVALID_STRIDED = [dict(data_stride=63), dict(rec_stride=31), dict(stripes=0, data_stride=0), dict(stripes=0, rec_stride=31)]
NOTHING = [dict(stripes=0), dict(stripes=0, data=False, rec=False),
           dict(m=1, nbytes=13, stripes=0), dict(k=256, m=1, stripes=0), dict(k=1, m=254, stripes=0),
           dict(k=253, m=2, stripes=0), dict(k=200, m=55, stripes=0), dict(k=1, m=3, nbytes=13, stripes=0)]
WORK = [dict(), dict(m=1, nbytes=13), dict(k=1, m=3, nbytes=16), dict(k=1, m=3, nbytes=13),
        dict(k=255, m=1, nbytes=8), dict(k=256, m=1, nbytes=8), dict(k=200, m=55, nbytes=40), dict(k=253, m=2)]


@pytest.mark.parametrize("call", [_strided, _table], ids=["strided", "table"])
def test_locate_parameter_rules(call):
    import torch
    import longhair_amd
    lib = longhair_amd.lib()
    for kw in INVALID + (INVALID_STRIDED if call is _strided else []):
        assert call(lib, **kw) == -1, kw
        assert lib.cauchy_256_last_error(), kw
        assert longhair_amd.last_launch() == [], kw
    for kw in NOTHING:
        assert call(lib, **kw) == 0, kw
        assert longhair_amd.last_launch() == [], kw
    if not torch.cuda.is_available():   # work and no device (with one these would run on host pointers)
        for kw in WORK:
            assert call(lib, **kw) == -2, kw
            assert longhair_amd.last_launch() == [], kw


def test_no_exception_crosses_the_locate_calls():
    """The checked library's injected exception comes back from both new calls as -3."""
    from longhair_amd import _native
    lib = _native.bind(ctypes.CDLL(_check_lib()))
    for call in (_strided, _table):
        lib.cauchy_256_debug_throw_next()
        assert call(lib) == -3, call.__name__
        assert b"injected" in lib.cauchy_256_last_error(), call.__name__
    assert {n for n, (res, _) in _native.LOCATE_EXPORTS.items() if res is ctypes.c_int} == NAMES


def test_locate_wrappers_check_their_tensors():
    import torch
    import longhair_amd as lh
    make, real = _device_like()
    S, k, m, B = 3, 4, 2, 16
    data, rec = make(S, k, B), make(S, m, B)
    cpu = lambda *shape, dtype=torch.uint8: torch.zeros(shape, dtype=dtype)   # noqa: E731
    bad = [
        (TypeError, dict(data=make(S, k, B, dtype=torch.int8))),
        (TypeError, dict(recovery=make(S, m, B, dtype=torch.float32))),
        (TypeError, dict(status=make(S, dtype=torch.uint8))),
        (TypeError, dict(rows=make(S, dtype=torch.int8))),
        (TypeError, dict(data=[[0] * B] * k)),
        (ValueError, dict(data=make(S, k * B))),                      # rank
        (ValueError, dict(recovery=make(S * m, B))),
        (ValueError, dict(recovery=make(S + 1, m, B))),
        (ValueError, dict(recovery=make(S, m, B + 8))),
        (ValueError, dict(data=make(S, k, 2 * B)[:, :, ::2])),        # blocks not contiguous
        (ValueError, dict(recovery=make(S, 2 * m, B)[:, ::2])),
        (ValueError, dict(status=make(S + 1, dtype=torch.int8))),
        (ValueError, dict(rows=make(S + 1))),
        (ValueError, dict(rows=make(S, 1))),
        (ValueError, dict(rows=make(2 * S)[::2])),                    # non-contiguous rows
        (ValueError, dict(status=make(2 * S, dtype=torch.int8)[::2])),
        (ValueError, dict(data=cpu(S, k, B))),                        # not on a device
        (ValueError, dict(recovery=cpu(S, m, B))),
        (ValueError, dict(status=cpu(S, dtype=torch.int8))),
        (ValueError, dict(rows=cpu(S))),
    ]
    for exc, kw in bad:
        args = dict(data=data, recovery=rec, status=make(S, dtype=torch.int8), rows=make(S))   # (allocated here: see _device_like)
        args.update(kw)
        with pytest.raises(exc):
            lh.locate_batch(**args)
    tab = lambda n: make(S, n, dtype=torch.int64)   # noqa: E731
    bad = [
        (TypeError, dict(data_ptrs=make(S, k, dtype=torch.int32))),
        (TypeError, dict(recovery_ptrs=make(S, m))),
        (TypeError, dict(status=make(S, dtype=torch.int16))),
        (TypeError, dict(rows=make(S, dtype=torch.int64))),
        (ValueError, dict(data_ptrs=tab(k + 1))),
        (ValueError, dict(data_ptrs=make(S * k, dtype=torch.int64))),
        (ValueError, dict(recovery_ptrs=tab(m + 1))),
        (ValueError, dict(recovery_ptrs=make(S, 2 * m, dtype=torch.int64)[:, ::2])),
        (ValueError, dict(data_ptrs=cpu(S, k, dtype=torch.int64))),
        (ValueError, dict(status=make(S - 1, dtype=torch.int8))),
        (ValueError, dict(rows=make(S - 1))),
    ]
    for exc, kw in bad:
        args = dict(data_ptrs=tab(k), recovery_ptrs=tab(m), status=make(S, dtype=torch.int8), rows=make(S))
        args.update(kw)
        with pytest.raises(exc):
            lh.locate_batch_ptrs(k, m, B, **args)
    if real and torch.cuda.device_count() > 1:
        with pytest.raises(ValueError):
            lh.locate_batch(data, rec.to("cuda:1"))
    # a non-zero code from the library is a LonghairError (k + m == 256, m >= 2: rejected before any device work)
    with pytest.raises(lh.LonghairError) as err:
        lh.locate_batch(make(S, 250, B), make(S, 6, B), status=make(S, dtype=torch.int8), rows=make(S), stream=0)
    assert err.value.code == -1
    with pytest.raises(lh.LonghairError) as err:
        lh.locate_batch_ptrs(0, m, B, make(S, 0, dtype=torch.int64), tab(m), status=make(S, dtype=torch.int8),
                             rows=make(S), stream=0)
    assert err.value.code == -1
