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


# ------------------------------------------------------------- deterministic erasure patterns
# A pattern is (E, R): the erased originals and the recovery rows that stand in for them, two
# ascending tuples of the same length e.  `placements` lays one pattern out over the k slots in
# up to five ways; `exhaustive_patterns` is every pattern of a small code, `designed_patterns` a
# net over the edges of a code too large to enumerate.  Nothing here draws an unseeded number
# (tests/test_lhutil_patterns.py).
PLACEMENTS = "abcde"
EDGES = (0, 1, 2, 31, 32, 62, 63, 64, 65, 126, 127, 128, 129)


def edges(n):
    """The positions of [0, n) at which the kernels change lane, wave or pass."""
    return sorted({v for v in EDGES + (n - 3, n - 2, n - 1) if 0 <= v < n})


def placements(k, E, R, seed, keep=PLACEMENTS, labels=False):
    """The distinct slot layouts of one pattern, as `erasure_case` returns them ((slots, rows);
    with `labels` (label, slots, rows)), in this order:
      a  recovery blocks in the erased slots, R ascending;   b  the same, R descending;
      c  survivors in order, then the recovery blocks;       d  recovery blocks, then survivors;
      e  one permutation of c, seeded by `seed`.
    `keep` names the layouts wanted; duplicates of an earlier layout are dropped."""
    E, R = sorted(int(x) for x in E), sorted(int(j) for j in R)
    assert len(E) == len(R) and len(set(E)) == len(E) and len(set(R)) == len(R)
    assert all(0 <= x < k for x in E)
    surv = [("d", x) for x in range(k) if x not in set(E)]
    rec = [("r", j) for j in R]
    at = {x: i for i, x in enumerate(E)}
    c = surv + rec
    perm = np.random.Generator(np.random.PCG64(seed)).permutation(k).tolist()
    forms = {
        "a": [("r", R[at[x]]) if x in at else ("d", x) for x in range(k)],
        "b": [("r", R[len(R) - 1 - at[x]]) if x in at else ("d", x) for x in range(k)],
        "c": c,
        "d": rec + surv,
        "e": [c[i] for i in perm],
    }
    out, seen = [], set()
    for label in PLACEMENTS:
        slots = forms[label]
        if label not in keep or tuple(slots) in seen:
            continue
        seen.add(tuple(slots))
        rows = [x if kind == "d" else k + x for kind, x in slots]
        out.append((label, slots, rows) if labels else (slots, rows))
    return out


def exhaustive_patterns(k, m):
    """Every (E, R) with |E| = |R| = e, e = 0..min(k, m): C(k + m, k) of them (Vandermonde)."""
    import itertools
    return [(E, R) for e in range(min(k, m) + 1)
            for E in itertools.combinations(range(k), e) for R in itertools.combinations(range(m), e)]


def designed_patterns(k, m):
    """Patterns for a code too large to enumerate, duplicates dropped, in this order: the empty
    pattern; every single erasure (x, j) (all x and j when k * m <= 1024, else edges(k) x
    edges(m)); for e = 1..e_max the four ladders (first / last e originals x first / last e
    rows), one evenly strided pattern (E = floor(i k / e), R = floor(i m / e)) and, from e = 2,
    the same originals with the rows spread from row 0 to row m - 1 inclusive
    (R = floor(i (m - 1) / (e - 1))), so that row 0 meets row m - 1 at every e and not only at
    e = m."""
    e_max = min(k, m)
    out = [((), ())]
    xs, js = (range(k), range(m)) if k * m <= 1024 else (edges(k), edges(m))
    out += [((x,), (j,)) for x in xs for j in js]
    for e in range(1, e_max + 1):
        first_x, last_x = tuple(range(e)), tuple(range(k - e, k))
        first_j, last_j = tuple(range(e)), tuple(range(m - e, m))
        out += [(first_x, first_j), (last_x, last_j), (first_x, last_j), (last_x, first_j)]
        E = tuple(i * k // e for i in range(e))
        if len(set(E)) == e:
            R = tuple(i * m // e for i in range(e))
            out.append((E, R if len(set(R)) == e else first_j))
            if e >= 2:
                R = tuple(i * (m - 1) // (e - 1) for i in range(e))
                if len(set(R)) == e:
                    out.append((E, R))
    return list(dict.fromkeys(out))


def pattern_cases(k, m, patterns, seed, keep=PLACEMENTS):
    """Every pattern x placement, in generation order: a list of (E, R, label, slots, rows).
    Pattern i's permuted layout is seeded by (seed, i)."""
    return [(E, R, label, slots, rows) for i, (E, R) in enumerate(patterns)
            for label, slots, rows in placements(k, E, R, seed * 1000003 + i, keep, labels=True)]


def pattern_data(k, bytes_, stripes, seed, pool=32):
    """The data stripes of `pattern_batch`, uint8 [min(pool, stripes), k, bytes]: stripe s of
    the batch was encoded from entry s % len."""
    n = max(1, min(pool, stripes))
    return fill(seed, n * k * bytes_).reshape(n, k, bytes_)


def pattern_batch(codec, k, m, bytes_, cases, seed, pool=32):
    """The received stripes of `pattern_cases`: (blocks uint8 [S, k, bytes], rows uint8 [S, k]).
    Stripe s takes data stripe s % pool of `fill(seed, ...)` and its recovery blocks from
    codec.encode, so neighbouring stripes hold different bytes."""
    data = pattern_data(k, bytes_, len(cases), seed, pool)
    n = data.shape[0]
    both = np.empty((n, k + m, bytes_), dtype=np.uint8)
    both[:, :k] = data
    for p in range(n):
        rc, rec = codec.encode(k, m, data[p], bytes_)
        assert rc == 0, (k, m, bytes_, rc)
        both[p, k:] = rec.reshape(m, bytes_)
    rows = np.array([c[4] for c in cases], dtype=np.uint8).reshape(len(cases), k)
    blocks = both[(np.arange(len(cases)) % n)[:, None], rows.astype(np.intp)]
    return blocks, rows


_BLOCK_DT = np.dtype({"names": ["data", "row"], "formats": ["<u8", "u1"], "offsets": [0, 8],
                      "itemsize": ctypes.sizeof(Block)})


def decode_all(codec, k, m, blocks, rows, bytes_):
    """codec.decode of every stripe of (blocks [S, k, bytes], rows [S, k]), the inputs left
    alone: (return codes int32 [S], rows out uint8 [S, k], blocks out uint8 [S, k, bytes])."""
    out = np.array(blocks, dtype=np.uint8, order="C")
    stripes = out.shape[0]
    assert out.shape == (stripes, k, bytes_)
    tab = np.zeros((stripes, k), dtype=_BLOCK_DT)
    tab["data"] = out.ctypes.data + (np.arange(stripes * k, dtype=np.uint64) * np.uint64(bytes_)).reshape(stripes, k)
    tab["row"] = rows
    rcs = np.empty(stripes, dtype=np.int32)
    for s in range(stripes):
        rcs[s] = codec._dec(k, m, ctypes.c_void_p(tab.ctypes.data + s * tab.strides[0]), bytes_)
    return rcs, np.ascontiguousarray(tab["row"]), out


def pattern_digest(rcs, rows_out, blocks_out):
    """The fixture digest of a shape's decoded cases: h64 over the return codes (one signed
    byte each), every rows-out and every block, in generation order."""
    return h64(np.concatenate([np.asarray(rcs).astype(np.int8).view(np.uint8).reshape(-1),
                               np.asarray(rows_out, dtype=np.uint8).reshape(-1),
                               np.asarray(blocks_out, dtype=np.uint8).reshape(-1)]))


# ------------------------------------------------------------------ batch sizes
# tests/test_gpu_stripe_counts.py runs every prefix length of one prepared batch that meets an
# edge of a kernel's stripe-to-workgroup mapping (tests/test_lhutil_counts.py holds the set).
COUNT_GRIDS = (7, 8, 9, 15, 16, 17)   # workgroups around the XCD renumbering's 8 and 16


def stripe_counts(tile, extra=(), grids=COUNT_GRIDS):
    """The batch sizes to sweep for a kernel whose workgroup covers `tile` stripes (>= 1),
    ascending and unique: every n in 1 .. 2 tile + 1 (each partial-wave and partial-workgroup
    residue, twice), g tile - 1, g tile, g tile + 1 for g in `grids` (a grid just below, at and
    past 8 and 16 workgroups), and `extra`.  The largest is the batch to prepare."""
    tile = int(tile)
    if tile < 1:
        raise ValueError("a workgroup covers at least one stripe")
    counts = set(range(1, 2 * tile + 2))
    for g in grids:
        counts.update((g * tile - 1, g * tile, g * tile + 1))
    counts.update(int(n) for n in extra)
    if min(counts) < 1:
        raise ValueError("batch sizes start at 1")
    return sorted(counts)


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
