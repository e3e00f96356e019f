"""Shared helpers of the repair tests (cauchy_256_reconstruct_batch, test infrastructure).

The expectation is always first principles: `codeword` is the stripe's data followed by the C
oracle's encode of it, uint8 [k + m, B]; the k survivors are rows dropped from it, and every
wanted row must equal the codeword's row.  `compose` is the coefficient composition of
lh_reconstruct_coef_kernel in numpy (include/cauchy_256_reconstruct.h; a GF(256) inverse of its
own), `apply` the kernel's B(c) arithmetic (lhupdate.ladder); tests/test_reconstruct_model.py pins
both to the oracle.  `case` builds one batch with its expectation."""
import functools
import itertools

import numpy as np

import lhupdate
import lhutil

NONE = 0xFF            # a want_rows entry with nothing wanted
LANE, FLAT_LANE, TILE = 8, 16, 4   # kernels.hip: bytes per lane and sub-block; flat lanes; wanted rows per tile


def is_flat(k, m):
    return m == 1 or k == 1


def lanes_per_stripe(k, m, nbytes):
    return -(-nbytes // FLAT_LANE) if is_flat(k, m) else -(-(nbytes // 8) // LANE)


def stripes_per_workgroup(k, m, nbytes):
    return max(1, 256 // lanes_per_stripe(k, m, nbytes))


# ------------------------------------------------------------------ GF(256), polynomial 0x187
def gmul(a, b):
    r = 0
    a, b = int(a), int(b)
    while b:
        if b & 1:
            r ^= a
        a <<= 1
        if a & 0x100:
            a ^= 0x187
        b >>= 1
    return r


@functools.lru_cache(maxsize=None)
def ginv(a):
    assert a
    r, p = 1, a
    for bit in range(8):   # a^254
        if (254 >> bit) & 1:
            r = gmul(r, p)
        p = gmul(p, p)
    assert gmul(r, a) == 1
    return r


def gf_inverse(A):
    """Inverse of a square GF(256) matrix (list of lists) by Gauss-Jordan."""
    n = len(A)
    M = [list(map(int, A[i])) + [int(i == j) for j in range(n)] for i in range(n)]
    for c in range(n):
        p = next(r for r in range(c, n) if M[r][c])
        M[c], M[p] = M[p], M[c]
        iv = ginv(M[c][c])
        M[c] = [gmul(v, iv) for v in M[c]]
        for r in range(n):
            f = M[r][c]
            if r != c and f:
                M[r] = [v ^ gmul(f, x) for v, x in zip(M[r], M[c])]
    return [row[n:] for row in M]


def generator(oracle, k, m):
    """G uint8 [m, k]: row 0 all ones, rows 1.. the oracle's Cauchy rows."""
    G = np.ones((m, k), dtype=np.uint8)
    if m > 1 and k > 1:
        G[1:] = oracle.cauchy_rows(k, m)
    return G


def compose(k, m, G, rows, want_rows):
    """C [want][k] of one valid stripe, as the header's table has it: a unit vector for a row that
    is present, w[i] for the erased original E_i, and for an absent recovery row r
    [rows[slot] < k] G[r][rows[slot]] ^ sum_i G[r][E_i] w[i][slot]; w = the single-pass matrix of
    the decode (A^-1 over the recovery slots, A^-1 G over the data slots)."""
    rows = [int(r) for r in rows]
    assert len(rows) == k and len(set(rows)) == k and all(r < k + m for r in rows)
    flat = is_flat(k, m)
    E = [x for x in range(k) if x not in rows]
    rcv = [(slot, r - k) for slot, r in enumerate(rows) if r >= k]   # array order
    assert len(E) == len(rcv) or flat
    w = []
    if E and not flat:
        Ainv = gf_inverse([[G[r][x] for x in E] for _, r in rcv])     # A[i][j] = G[r_i][E_j]
        for i in range(len(E)):
            wi = [0] * k
            for slot, row in enumerate(rows):
                if row >= k:
                    wi[slot] = Ainv[i][[s for s, _ in rcv].index(slot)]
                else:
                    for j, (_, r) in enumerate(rcv):
                        wi[slot] ^= gmul(Ainv[i][j], G[r][row])
            w.append(wi)
    C = []
    for wr in want_rows:
        wr = int(wr)
        if wr == NONE:
            C.append([0] * k)
        elif wr in rows:
            C.append([int(slot == rows.index(wr)) for slot in range(k)])
        elif flat:
            C.append([1] * k)
        elif wr < k:
            C.append(list(w[E.index(wr)]))
        else:
            r = wr - k
            c = [int(G[r][row]) if row < k else 0 for row in rows]
            for i, x in enumerate(E):
                for slot in range(k):
                    c[slot] ^= gmul(G[r][x], w[i][slot])
            C.append(c)
    return C


def apply(k, m, nbytes, blocks, C):
    """out_j = sum_slot B(C[j][slot]) block_slot, uint8 [len(C), nbytes]."""
    out = np.zeros((len(C), nbytes), dtype=np.uint8)
    for j, c in enumerate(C):
        for slot in range(k):
            e = int(c[slot])
            if not e:
                continue
            if is_flat(k, m):
                assert e == 1
                out[j] ^= blocks[slot]
                continue
            sub = nbytes // 8
            v = lhupdate.ladder(np.asarray(blocks[slot]).reshape(8, sub))
            o = out[j].reshape(8, sub)
            for q in range(8):
                if (e >> q) & 1:
                    for y in range(8):
                        o[y] ^= v[q + y]
    return out


# ------------------------------------------------------------------ codewords and batches
@functools.lru_cache(maxsize=None)
def codewords(oracle, k, m, nbytes, stripes, seed):
    """uint8 [stripes, k + m, nbytes], read-only: lhutil.fill data and the oracle's recovery."""
    cw = np.empty((stripes, k + m, nbytes), dtype=np.uint8)
    cw[:, :k] = lhutil.fill(seed, stripes * k * nbytes).reshape(stripes, k, nbytes)
    for s in range(stripes):
        rc, r = oracle.encode(k, m, cw[s, :k], nbytes)
        assert rc == 0, (k, m, nbytes, rc)
        cw[s, k:] = r.reshape(m, nbytes)
    cw.setflags(write=False)
    return cw


def stripe_valid(k, m, rows, want_rows):
    rows = [int(r) for r in rows]
    return (len(set(rows)) == k and all(r < k + m for r in rows)
            and all(int(w) == NONE or int(w) < k + m for w in want_rows))


def case(cw, k, m, rows, want_rows, canary):
    """blocks [S, k, B] = the codeword's rows `rows` [S, k] (an invalid row takes row 0's bytes),
    the expected out [S, want, B] (the codeword's wanted rows; `canary` where nothing is written:
    0xFF entries and every entry of an invalid stripe) and the expected status int8 [S]."""
    S, n, nbytes = cw.shape
    rows, want_rows = np.asarray(rows, dtype=np.uint8), np.asarray(want_rows, dtype=np.uint8)
    assert rows.shape == (S, k) and want_rows.shape[0] == S and n == k + m
    blocks = np.empty((S, k, nbytes), dtype=np.uint8)
    exp = np.full((S, want_rows.shape[1], nbytes), canary, dtype=np.uint8)
    status = np.zeros(S, dtype=np.int8)
    for s in range(S):
        for i, r in enumerate(rows[s]):
            blocks[s, i] = cw[s, r if r < n else 0]
        if not stripe_valid(k, m, rows[s], want_rows[s]):
            status[s] = -1
            continue
        for j, w in enumerate(want_rows[s]):
            if w != NONE:
                exp[s, j] = cw[s, w]
    return blocks, exp, status


STYLES = ("absent", "mixed", "hole", "repeat")


def pick_want(rng, k, m, rows, want, style):
    """One stripe's wanted rows: 'absent' the rows that are not among the survivors (walked from a
    random start, so both data and recovery rows come up), 'mixed' any rows, 'hole' mixed with one
    0xFF entry, 'repeat' absent rows with the last entry repeating the first."""
    absent = [r for r in range(k + m) if r not in rows]
    if style in ("absent", "repeat") and absent:
        o = int(rng.integers(0, len(absent)))
        out = [absent[(o + j) % len(absent)] for j in range(want)]
    else:
        out = [int(r) for r in rng.integers(0, k + m, size=want)]
    if style == "repeat" and want >= 2:
        out[-1] = out[0]
    if style == "hole":
        out[int(rng.integers(0, want))] = NONE
    return out


def random_batch(k, m, stripes, want, seed):
    """rows uint8 [S, k] (0 .. min(k, m) erasures cycling, slots shuffled) and want_rows uint8
    [S, want] (STYLES cycling), all valid."""
    rng = np.random.Generator(np.random.PCG64(seed))
    e_max = min(k, m)
    rows = np.empty((stripes, k), dtype=np.uint8)
    wr = np.empty((stripes, want), dtype=np.uint8)
    for s in range(stripes):
        rows[s] = pick_rows(rng, k, m, (e_max - s) % (e_max + 1))
        wr[s] = pick_want(rng, k, m, rows[s].tolist(), want, STYLES[s % len(STYLES)])
    return rows, wr


def survivor_sets(k, m):
    """Every k-subset of the k + m rows, ascending."""
    return [list(c) for c in itertools.combinations(range(k + m), k)]


def pick_rows(rng, k, m, erasures):
    """One stripe's survivor rows: `erasures` originals lost, as many recovery rows in their
    place, the slots shuffled."""
    lost = set(rng.choice(k, size=erasures, replace=False).tolist())
    rec = (k + rng.choice(m, size=erasures, replace=False)).tolist()
    rows = [x for x in range(k) if x not in lost] + rec
    return [int(r) for r in rng.permutation(rows)]
