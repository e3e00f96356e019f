"""CPU-only checks of the repair boundary (include/cauchy_256_reconstruct.h): the exports, every
parameter rule (they come before any device work, so they hold without a GPU), the exception
barrier of the checked library and the argument checks of the Python wrappers."""
import ctypes
import os

import pytest

import lhutil
from test_abi import _declared_functions
from test_update_abi import _check_lib, _device_like

HEADER = ("cauchy_256_reconstruct.h",)
NAMES = {"cauchy_256_reconstruct_batch", "cauchy_256_reconstruct_batch_ptrs"}


def test_reconstruct_header_symbols_are_exported():
    import longhair_amd
    from longhair_amd import _native
    names = _declared_functions(HEADER)
    assert names == NAMES
    assert set(_native.RECONSTRUCT_EXPORTS) == names
    for older in (_native.EXPORTS, _native.OPTIONAL_EXPORTS, _native.UPDATE_EXPORTS, _native.VERIFY_EXPORTS):
        assert not names & set(older)
    for path in (_native.library_path, _check_lib()):
        lib = ctypes.CDLL(path)
        for name in names:
            assert hasattr(lib, name), (path, name)
    bound = longhair_amd.lib()
    for name, (res, args) in _native.RECONSTRUCT_EXPORTS.items():
        assert getattr(bound, name).restype is res and getattr(bound, name).argtypes == args, name


def test_older_export_tables_are_unchanged():
    from longhair_amd import _native
    assert set(_native.EXPORTS) == _declared_functions()
    assert set(_native.OPTIONAL_EXPORTS) == {"cauchy_256_debug_throw_next"}
    assert set(_native.UPDATE_EXPORTS) == _declared_functions(("cauchy_256_update.h",))
    assert set(_native.VERIFY_EXPORTS) == _declared_functions(("cauchy_256_verify.h",))
    assert os.path.exists(os.path.join(lhutil.REPO, "include", HEADER[0]))


def _strided(lib, k=4, m=2, nbytes=16, stripes=1, want=1, blocks=True, rows=True, want_rows=True, out=True,
             status=True, blocks_stride=None, out_stride=None):
    buf = (ctypes.c_ubyte * 64)()
    on = lambda flag: buf if flag else None   # noqa: E731
    return lib.cauchy_256_reconstruct_batch(k, m, nbytes, stripes, on(blocks),
                                            max(k, 0) * max(nbytes, 0) if blocks_stride is None else blocks_stride,
                                            on(rows), want, on(want_rows), on(out),
                                            max(want, 0) * max(nbytes, 0) if out_stride is None else out_stride,
                                            on(status), None)


def _table(lib, k=4, m=2, nbytes=16, stripes=1, want=1, blocks=True, rows=True, want_rows=True, out=True, status=True):
    buf = (ctypes.c_ubyte * 64)()
    tab = (ctypes.c_void_p * 8)()
    return lib.cauchy_256_reconstruct_batch_ptrs(k, m, nbytes, stripes, tab if blocks else None, buf if rows else None,
                                                 want, buf if want_rows else None, tab if out else None,
                                                 buf if status else None, None)


INVALID = [
    dict(k=0), dict(m=0), dict(k=-1), dict(m=-3), dict(k=257, m=1), dict(k=1, m=257),
    dict(nbytes=0), dict(nbytes=-8), dict(stripes=-1), dict(want=0), dict(want=-1),
    dict(k=250, m=6), dict(k=255, m=1), dict(k=1, m=255), dict(k=128, m=128), dict(k=256, m=1),
    dict(nbytes=12), dict(k=2, m=2, nbytes=13),
    dict(blocks=False), dict(rows=False), dict(want_rows=False), dict(out=False),
    dict(stripes=0, want=0), dict(stripes=0, k=255, m=1),
    dict(want=2 ** 29), dict(k=254, m=1, nbytes=8, want=8454661), dict(stripes=0, want=2 ** 31 - 1),   # want * k > 2^31 - 1
]
INVALID_STRIDED = [dict(blocks_stride=63), dict(out_stride=15), dict(want=3, out_stride=47),
                   dict(stripes=0, blocks_stride=0), dict(stripes=0, out_stride=15)]
NOTHING = [dict(stripes=0), dict(stripes=0, blocks=False, rows=False, want_rows=False, out=False),
           dict(stripes=0, status=False), dict(m=1, nbytes=13, stripes=0), dict(k=254, m=1, stripes=0),
           dict(k=1, m=254, nbytes=7, stripes=0), dict(k=254, m=1, nbytes=8, want=8454660, stripes=0)]
WORK = [dict(), dict(status=False), dict(want=3), dict(m=1, nbytes=13), dict(k=1, m=3, nbytes=7),
        dict(k=254, m=1, nbytes=8), dict(k=200, m=55, nbytes=40), dict(k=128, m=32, nbytes=64, want=32)]


@pytest.mark.parametrize("call", [_strided, _table], ids=["strided", "table"])
def test_reconstruct_parameter_rules(call):
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


def test_no_exception_crosses_the_reconstruct_calls():
    """The checked library's injected exception comes back from both new calls as -3."""
    from longhair_amd import _native
    lib = _native.bind(ctypes.CDLL(_check_lib()))
    for call in (_strided, _table):
        lib.cauchy_256_debug_throw_next()
        assert call(lib) == -3, call.__name__
        assert b"injected" in lib.cauchy_256_last_error(), call.__name__
    assert {n for n, (res, _) in _native.RECONSTRUCT_EXPORTS.items() if res is ctypes.c_int} == NAMES


def test_reconstruct_wrappers_check_their_tensors():
    import torch
    import longhair_amd as lh
    make, real = _device_like()
    S, k, m, B, W = 3, 4, 2, 16, 2
    cpu = lambda *shape, dtype=torch.uint8: torch.zeros(shape, dtype=dtype)   # noqa: E731
    bad = [
        (TypeError, dict(blocks=make(S, k, B, dtype=torch.int8))),
        (TypeError, dict(rows=make(S, k, dtype=torch.int32))),
        (TypeError, dict(want_rows=make(S, W, dtype=torch.int8))),
        (TypeError, dict(out=make(S, W, B, dtype=torch.float32))),
        (TypeError, dict(status=make(S, dtype=torch.uint8))),
        (TypeError, dict(want_rows=[[4, 5]] * S)),
        (ValueError, dict(blocks=make(S, k * B))),                      # rank
        (ValueError, dict(rows=make(S, k + 1))),
        (ValueError, dict(rows=make(S * k))),
        (ValueError, dict(rows=make(S, 2 * k)[:, ::2])),                # non-contiguous rows
        (ValueError, dict(want_rows=make(S))),
        (ValueError, dict(want_rows=make(S + 1, W))),
        (ValueError, dict(want_rows=make(S, 2 * W)[:, ::2])),
        (ValueError, dict(out=make(S, W + 1, B))),
        (ValueError, dict(out=make(S, W, B + 8))),
        (ValueError, dict(out=make(S + 1, W, B))),
        (ValueError, dict(out=make(S, W, 2 * B)[:, :, ::2])),           # blocks not contiguous
        (ValueError, dict(blocks=make(S, k, 2 * B)[:, :, ::2])),
        (ValueError, dict(status=make(S + 1, dtype=torch.int8))),
        (ValueError, dict(blocks=cpu(S, k, B))),                        # not on a device
        (ValueError, dict(rows=cpu(S, k))),
        (ValueError, dict(want_rows=cpu(S, W))),
        (ValueError, dict(out=cpu(S, W, B))),
        (ValueError, dict(status=cpu(S, dtype=torch.int8))),
    ]
    for exc, kw in bad:
        args = dict(blocks=make(S, k, B), rows=make(S, k), want_rows=make(S, W), out=make(S, W, B),
                    status=make(S, dtype=torch.int8))   # (allocated here: see _device_like)
        args.update(kw)
        with pytest.raises(exc):
            lh.reconstruct_batch(m=m, **args)
    tab = lambda n: make(S, n, dtype=torch.int64)   # noqa: E731
    bad = [
        (TypeError, dict(block_ptrs=make(S, k, dtype=torch.int32))),
        (TypeError, dict(out_ptrs=make(S, W))),
        (TypeError, dict(rows=make(S, k, dtype=torch.int8))),
        (TypeError, dict(status=make(S, dtype=torch.int16))),
        (ValueError, dict(block_ptrs=tab(k + 1))),
        (ValueError, dict(block_ptrs=make(S * k, dtype=torch.int64))),
        (ValueError, dict(out_ptrs=tab(W + 1))),
        (ValueError, dict(out_ptrs=make(S, 2 * W, dtype=torch.int64)[:, ::2])),
        (ValueError, dict(rows=make(S, k - 1))),
        (ValueError, dict(want_rows=make(S - 1, W))),
        (ValueError, dict(block_ptrs=cpu(S, k, dtype=torch.int64))),
        (ValueError, dict(status=make(S - 1, dtype=torch.int8))),
    ]
    for exc, kw in bad:
        args = dict(block_ptrs=tab(k), rows=make(S, k), want_rows=make(S, W), out_ptrs=tab(W),
                    status=make(S, dtype=torch.int8))
        args.update(kw)
        with pytest.raises(exc):
            lh.reconstruct_batch_ptrs(k, m, B, **args)
    if real and torch.cuda.device_count() > 1:
        with pytest.raises(ValueError):
            lh.reconstruct_batch(make(S, k, B), make(S, k).to("cuda:1"), m, make(S, W))
    # a non-zero code from the library is a LonghairError (k + m > 255: rejected before any device work)
    with pytest.raises(lh.LonghairError) as err:
        lh.reconstruct_batch(make(S, 250, B), make(S, 250), 6, make(S, W), out=make(S, W, B),
                             status=make(S, dtype=torch.int8), stream=0)
    assert err.value.code == -1
    with pytest.raises(lh.LonghairError) as err:
        lh.reconstruct_batch_ptrs(0, m, B, make(S, 0, dtype=torch.int64), make(S, 0), make(S, W), tab(W),
                                  status=make(S, dtype=torch.int8), stream=0)
    assert err.value.code == -1
