"""Shared helpers for tests, golden generation and bench (test infrastructure).

- `fill(seed, n)`: the fixed input-data spec.  Bytes are the little-endian words of
  splitmix64(seed * 2**32 + i), i = 0, 1, ...  Reproducible in numpy, C and HIP.
- `Oracle`: ctypes handle to oracle/liblh_oracle.so (the C restatement).
- `RefLib`: ctypes handle to oracle/_ref/liblonghair_ref.so (the reference itself,
  compiled from /root/reference by `make -C oracle ref`).  Only used to generate golden
  fixtures and as the CPU baseline; never by the product.
"""
import ctypes
import hashlib
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = os.path.join(REPO, "longhair_amd", "data", "cauchy_tables_256.bin")
ORACLE_SO = os.path.join(REPO, "oracle", "liblh_oracle.so")
REF_SO = os.path.join(REPO, "oracle", "_ref", "liblonghair_ref.so")
GOLDEN = os.path.join(REPO, "tests", "golden")

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def splitmix64(x):
    """Vectorised splitmix64 finaliser over a uint64 array (wrapping arithmetic)."""
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def fill(seed, n):
    """n pseudo-random bytes for `seed` (see module docstring)."""
    words = (n + 7) // 8
    ctr = np.arange(words, dtype=np.uint64) + np.uint64((seed & 0xFFFFFFFF) << 32)
    return splitmix64(ctr).view(np.uint8)[:n].copy()


def h64(buf):
    """16-hex-digit SHA-256 prefix of a byte buffer (fixture digest)."""
    return hashlib.sha256(np.ascontiguousarray(buf).tobytes()).hexdigest()[:16]


class Block(ctypes.Structure):
    """Reference Block layout (cauchy_256.h:52-55)."""
    _fields_ = [("data", ctypes.POINTER(ctypes.c_ubyte)), ("row", ctypes.c_ubyte)]


def _ptr(arr):
    return arr.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte))


class _Codec:
    """encode/decode over numpy buffers for a C library with the reference ABI."""

    def __init__(self, lib, enc, dec):
        self.lib = lib
        self._enc = enc
        self._dec = dec
        enc.restype = ctypes.c_int
        dec.restype = ctypes.c_int

    def encode(self, k, m, data, bytes_):
        """data: uint8 [k, bytes] (or [k*bytes]).  Returns (rc, recovery uint8 [m*bytes])."""
        data = np.ascontiguousarray(data).reshape(-1)
        rec = np.zeros(max(m, 1) * bytes_ + 64, dtype=np.uint8)
        ptrs = (ctypes.POINTER(ctypes.c_ubyte) * max(k, 1))()
        for x in range(k):
            ptrs[x] = ctypes.cast(data.ctypes.data + x * bytes_, ctypes.POINTER(ctypes.c_ubyte))
        rc = self._enc(ctypes.c_int(k), ctypes.c_int(m), ptrs, _ptr(rec), ctypes.c_int(bytes_))
        return rc, rec[: m * bytes_]

    def decode(self, k, m, bufs, rows, bytes_):
        """bufs: list of k uint8 arrays (modified in place), rows: list of k ints.
        Returns (rc, new_rows)."""
        blocks = (Block * k)()
        for i in range(k):
            blocks[i].data = _ptr(bufs[i])
            blocks[i].row = rows[i]
        rc = self._dec(ctypes.c_int(k), ctypes.c_int(m), blocks, ctypes.c_int(bytes_))
        return rc, [blocks[i].row for i in range(k)]


class Oracle(_Codec):
    def __init__(self, path=ORACLE_SO):
        lib = ctypes.CDLL(path)
        blob = open(TABLES, "rb").read()
        lib.lho_init.restype = ctypes.c_int
        assert lib.lho_init(ctypes.c_char_p(blob), ctypes.c_size_t(len(blob))) == 0
        super().__init__(lib, lib.lho_encode, lib.lho_decode)

    def cauchy_rows(self, k, m):
        out = np.zeros((m - 1) * k, dtype=np.uint8)
        self.lib.lho_cauchy_rows(ctypes.c_int(k), ctypes.c_int(m), _ptr(out))
        return out.reshape(m - 1, k)


class RefLib(_Codec):
    def __init__(self, path=REF_SO):
        lib = ctypes.CDLL(path)
        lib._cauchy_256_init.restype = ctypes.c_int
        assert lib._cauchy_256_init(ctypes.c_int(2)) == 0
        super().__init__(lib, lib.cauchy_256_encode, lib.cauchy_256_decode)


def erasure_case(seed, k, m, e, shuffle=True):
    """A decode scenario: erase `e` random originals, supply `e` random recovery rows,
    optionally shuffle the block order.  Returns (slots, rows) where slots[i] is
    ('d', x) for original x or ('r', j) for recovery block j, and rows[i] its row."""
    rng = np.random.Generator(np.random.PCG64(seed))
    erased = sorted(rng.choice(k, size=e, replace=False).tolist()) if e else []
    rec = sorted(rng.choice(m, size=e, replace=False).tolist()) if e else []
    slots = [("d", x) for x in range(k) if x not in erased] + [("r", j) for j in rec]
    if shuffle:
        order = rng.permutation(len(slots)).tolist()
        slots = [slots[i] for i in order]
    rows = [x if kind == "d" else k + x for kind, x in slots]
    return slots, rows


# ------------------------------------------------------------------ invalid stripes
# include/cauchy_256_batch.h: a stripe whose rows hold a duplicate or a row >= k + m is
# invalid (status -1, left untouched).  `invalidate_rows` breaks a valid stripe in one named
# way, `rows_valid` is that rule in plain Python (tests/test_lhutil_rows.py keeps the two in
# step, so a GPU test never passes because its generator stopped producing invalid stripes).
INVALID_KINDS = ("dup-orig", "dup-rec", "range", "range255")
INVALID_WHERE = ("first", "last", "wave", "wave+1", "rand")


def rows_valid(rows, k, m):
    """The header's rule: all k rows distinct and every one < k + m."""
    rows = [int(r) for r in rows]
    return len(rows) == k and len(set(rows)) == k and all(0 <= r < k + m for r in rows)


def invalid_kinds(k, m):
    """The kinds of `invalidate_rows` that apply to a (k, m) code."""
    kinds = []
    if k >= 2:
        kinds += ["dup-orig", "dup-rec"]
    if k + m <= 255:
        kinds += ["range", "range255"]
    return kinds


def invalid_pairs(k, m):
    """Every (kind, where) pair that applies to the shape, ordered by diagonals so that any
    run of len(kinds) consecutive pairs holds every kind once, at different positions."""
    kinds = invalid_kinds(k, m)
    n = len(INVALID_WHERE)
    return [(kind, INVALID_WHERE[(i + d) % n]) for d in range(n) for i, kind in enumerate(kinds)]


def invalidate_rows(rows, k, m, kind, where, rng):
    """A copy of one stripe's valid row list (as `erasure_case` returns it) made invalid.

    kind:  'dup-orig'  the slot takes the row of another slot that holds an original (when no
                       other slot holds one: as 'dup-rec');
           'dup-rec'   the slot takes the row of another slot that holds a recovery row (when
                       there is none: the slot and one other both get row k);
           'range'     the slot gets k + m;   'range255'  the slot gets 255 (both need
                       k + m <= 255).
    where: the slot overwritten: 'first' 0, 'last' k - 1, 'wave' 63 (k > 63, else k - 1),
           'wave+1' 64 (k > 64, else 0), 'rand' a random slot.
    Raises ValueError when the kind does not apply to the shape; never returns a valid stripe."""
    rows = [int(r) for r in rows]
    if not rows_valid(rows, k, m):
        raise ValueError("invalidate_rows needs a valid stripe")
    pos = {"first": 0, "last": k - 1, "wave": 63 if k > 63 else k - 1, "wave+1": 64 if k > 64 else 0,
           "rand": None}
    if where not in pos:
        raise ValueError(f"unknown position {where!r}")
    if kind not in INVALID_KINDS:
        raise ValueError(f"unknown kind {kind!r}")
    if kind not in invalid_kinds(k, m):
        raise ValueError(f"kind {kind!r} does not apply to k = {k}, m = {m}")
    p = pos[where] if pos[where] is not None else int(rng.integers(0, k))
    out = list(rows)
    others = [i for i in range(k) if i != p]
    if kind == "dup-orig":
        cand = [i for i in others if rows[i] < k]
        if not cand:
            kind = "dup-rec"
    if kind == "dup-rec":
        cand = [i for i in others if rows[i] >= k]
    if kind in ("dup-orig", "dup-rec"):
        if cand:
            out[p] = rows[cand[int(rng.integers(0, len(cand)))]]
        else:  # no recovery row anywhere else: two slots claim recovery row k
            out[p] = k
            out[others[int(rng.integers(0, len(others)))]] = k
    elif kind == "range":
        out[p] = k + m
    else:
        out[p] = 255
    if rows_valid(out, k, m):
        raise AssertionError(("invalidate_rows produced a valid stripe", rows, kind, where))
    return out
