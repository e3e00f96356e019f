"""CPU-only checks of the recovery-patch boundary (include/cauchy_256_update.h): the exports,
every parameter rule (they come before any device work, so they hold without a GPU), the
exception barrier of the checked library and the argument checks of the Python wrappers."""
import ctypes
import os

import pytest

import lhutil
from test_abi import _declared_functions

HEADER = ("cauchy_256_update.h",)


def _check_lib():
    from longhair_amd import _native
    path = os.path.join(os.path.dirname(_native.library_path), "liblonghair_amd_check.so")
    assert os.path.exists(path), "build the checked library (__graft_entry__.build())"
    return path


def test_update_header_symbols_are_exported():
    import longhair_amd
    from longhair_amd import _native
    names = _declared_functions(HEADER)
    assert names == {"cauchy_256_update_batch", "cauchy_256_update_batch_ptrs"}
    assert set(_native.UPDATE_EXPORTS) == names
    assert not names & set(_native.EXPORTS) and not names & set(_native.OPTIONAL_EXPORTS)
    for path in (_native.library_path, _check_lib()):
        lib = ctypes.CDLL(path)
        for name in names:
            assert hasattr(lib, name), (path, name)
    bound = longhair_amd.lib()
    for name, (res, args) in _native.UPDATE_EXPORTS.items():
        assert getattr(bound, name).restype is res and getattr(bound, name).argtypes == args, name


def _strided(lib, k=4, m=2, nbytes=16, stripes=1, changes=1, cols=True, old=True, new=True, rec=True,
             old_stride=None, new_stride=None, rec_stride=None):
    buf = (ctypes.c_ubyte * 64)()
    on = lambda flag: buf if flag else None   # noqa: E731
    cb = max(changes, 0) * max(nbytes, 0)
    return lib.cauchy_256_update_batch(k, m, nbytes, stripes, changes, on(cols), on(old),
                                       cb if old_stride is None else old_stride, on(new),
                                       cb if new_stride is None else new_stride, on(rec),
                                       max(m, 0) * max(nbytes, 0) if rec_stride is None else rec_stride, None, None)


def _table(lib, k=4, m=2, nbytes=16, stripes=1, changes=1, cols=True, old=True, new=True, rec=True):
    buf = (ctypes.c_ubyte * 64)()
    tab = (ctypes.c_void_p * 8)()
    return lib.cauchy_256_update_batch_ptrs(k, m, nbytes, stripes, changes, buf if cols else None, tab if old else None,
                                            tab if new else None, tab if rec else None, None, None)


INVALID = [
    dict(k=0), dict(k=256), dict(m=0), dict(k=-1), dict(m=-3),
    dict(nbytes=0), dict(nbytes=-8), dict(stripes=-1), dict(changes=-1), dict(changes=256),
    dict(cols=False), dict(old=False), dict(rec=False),
    dict(k=250, m=7), dict(k=255, m=2), dict(nbytes=12), dict(k=1, m=3, nbytes=13),
]
INVALID_STRIDED = [dict(old_stride=15), dict(new_stride=15), dict(changes=3, old_stride=47), dict(rec_stride=31),
                   dict(stripes=0, rec_stride=31), dict(stripes=0, old_stride=0)]
NOTHING = [dict(stripes=0), dict(changes=0), dict(stripes=0, changes=0), dict(stripes=0, cols=False, old=False, rec=False),
           dict(changes=0, cols=False, old=False, rec=False), dict(m=1, nbytes=13, stripes=0)]
WORK = [dict(), dict(new=False), dict(m=1, nbytes=13), dict(k=1, m=3, nbytes=16), dict(k=255, m=1, nbytes=8),
        dict(k=200, m=56, nbytes=40, rec_stride=56 * 40), dict(changes=4, new=False)]


@pytest.mark.parametrize("call", [_strided, _table], ids=["strided", "table"])
def test_update_parameter_rules(call):
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
            if call is _table:
                kw = {key: v for key, v in kw.items() if not key.endswith("_stride")}
            assert call(lib, **kw) == -2, kw
            assert longhair_amd.last_launch() == [], kw


def test_delta_form_ignores_new_stride():
    """d_new == NULL: d_old holds the deltas and new_stride means nothing."""
    import torch
    import longhair_amd
    lib = longhair_amd.lib()
    assert _strided(lib, new=False, new_stride=0, stripes=0) == 0
    assert _strided(lib, new=True, new_stride=0, stripes=0) == -1
    if not torch.cuda.is_available():
        assert _strided(lib, new=False, new_stride=0) == -2


def test_no_exception_crosses_the_update_calls():
    """The checked library's injected exception comes back from both new calls as -3."""
    from longhair_amd import _native
    lib = _native.bind(ctypes.CDLL(_check_lib()))
    for call in (_strided, _table):
        lib.cauchy_256_debug_throw_next()
        assert call(lib) == -3, call.__name__
        assert b"injected" in lib.cauchy_256_last_error(), call.__name__
    ints = {n for n, (res, _) in _native.UPDATE_EXPORTS.items() if res is ctypes.c_int}
    assert ints == {"cauchy_256_update_batch", "cauchy_256_update_batch_ptrs"}


def _device_like():
    """(make, real): uint8/any-dtype tensors the wrappers accept as device tensors.  With a GPU they
    are CUDA tensors; without one, CPU tensors of a subclass that answers is_cuda, so that the
    checks behind the device check (shape, contiguity) are reached -- every case below raises
    before the library is called."""
    import torch
    if torch.cuda.is_available():
        return (lambda *shape, dtype=torch.uint8: torch.zeros(shape, dtype=dtype, device="cuda")), True

    class OnDevice(torch.Tensor):
        is_cuda = property(lambda self: True)

    return (lambda *shape, dtype=torch.uint8: torch.zeros(shape, dtype=dtype).as_subclass(OnDevice)), False


def test_update_wrappers_check_their_tensors():
    import torch
    import longhair_amd as lh
    make, real = _device_like()
    S, m, c, B, k = 3, 2, 2, 16, 4
    rec, cols, old, new = make(S, m, B), make(S, c), make(S, c, B), make(S, c, B)
    cpu = lambda *shape, dtype=torch.uint8: torch.zeros(shape, dtype=dtype)   # noqa: E731
    bad = [
        (TypeError, dict(recovery=make(S, m, B, dtype=torch.int8))),
        (TypeError, dict(cols=make(S, c, dtype=torch.int32))),
        (TypeError, dict(old=make(S, c, B, dtype=torch.float32))),
        (TypeError, dict(new=make(S, c, B, dtype=torch.int16))),
        (TypeError, dict(status=make(S, dtype=torch.uint8))),
        (TypeError, dict(cols=[[0, 1]] * S)),
        (ValueError, dict(recovery=make(S, m * B))),
        (ValueError, dict(cols=make(S))),
        (ValueError, dict(cols=make(S + 1, c))),
        (ValueError, dict(cols=make(S, 2 * c)[:, ::2])),            # non-contiguous cols
        (ValueError, dict(old=make(S, c + 1, B))),
        (ValueError, dict(old=make(S, c, B + 8))),
        (ValueError, dict(new=make(S, c, B + 8))),
        (ValueError, dict(new=make(S, c, 2 * B)[:, :, ::2])),       # blocks not contiguous
        (ValueError, dict(status=make(S + 1, dtype=torch.int8))),
        (ValueError, dict(recovery=cpu(S, m, B))),                  # not on a device
        (ValueError, dict(cols=cpu(S, c))),
        (ValueError, dict(old=cpu(S, c, B))),
        (ValueError, dict(new=cpu(S, c, B))),
    ]
    for exc, kw in bad:
        args = dict(recovery=rec, cols=cols, old=old, new=new)
        args.update(kw)
        with pytest.raises(exc):
            lh.update_batch(k, **args)
    tab = lambda n: make(S, n, dtype=torch.int64)   # noqa: E731
    bad = [
        (TypeError, dict(cols=make(S, c, dtype=torch.int8))),
        (TypeError, dict(old_ptrs=make(S, c, dtype=torch.int32))),
        (TypeError, dict(recovery_ptrs=make(S, m))),
        (ValueError, dict(cols=make(S, 2 * c)[:, ::2])),
        (ValueError, dict(old_ptrs=tab(c + 1))),
        (ValueError, dict(new_ptrs=tab(c + 1))),
        (ValueError, dict(recovery_ptrs=tab(m + 1))),
        (ValueError, dict(cols=cpu(S, c))),
        (ValueError, dict(old_ptrs=cpu(S, c, dtype=torch.int64))),
        (ValueError, dict(status=make(S - 1, dtype=torch.int8))),
    ]
    for exc, kw in bad:
        args = dict(cols=cols, old_ptrs=tab(c), new_ptrs=tab(c), recovery_ptrs=tab(m))
        args.update(kw)
        with pytest.raises(exc):
            lh.update_batch_ptrs(k, m, B, **args)
    if real and torch.cuda.device_count() > 1:
        with pytest.raises(ValueError):
            lh.update_batch(k, rec, cols.to("cuda:1"), old, new)
    # a non-zero code from the library is a LonghairError (k = 0: rejected before any device work)
    with pytest.raises(lh.LonghairError) as err:
        lh.update_batch(0, rec, cols, old, new, status=make(S, dtype=torch.int8), stream=0)
    assert err.value.code == -1
    with pytest.raises(lh.LonghairError):
        lh.update_batch_ptrs(0, m, B, cols, tab(c), None, tab(m), status=make(S, dtype=torch.int8), stream=0)


def test_existing_export_tables_are_unchanged():
    """The update calls live in their own table: EXPORTS still equals the three older headers
    (tests/test_abi.py pins it) and the test hook is the only optional symbol."""
    from longhair_amd import _native
    assert set(_native.EXPORTS) == _declared_functions()
    assert set(_native.OPTIONAL_EXPORTS) == {"cauchy_256_debug_throw_next"}
    assert lhutil.REPO and os.path.exists(os.path.join(lhutil.REPO, "include", HEADER[0]))
