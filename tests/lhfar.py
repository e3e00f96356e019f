"""Far addresses: one multi-GiB device arena and the planner that places sparse batches in it
(tests/test_gpu_far.py; the planner's properties are proved on the CPU in tests/test_lhfar.py).

The arena is FRONT + 2^32 + 2^31 + SLACK bytes filled with one canary byte.  Every batch base
lies at or after offset FRONT = 2^31, so the two images of wrong 32-bit arithmetic -- an offset
truncated to uint32 lands in [base, base + 2^32), one truncated to int32 and sign-extended in
[base - 2^31, base + 2^31) -- fall inside the arena: a wrong address shows as wrong bytes or a
written canary, not as a fault.  A plan holds, per buffer of a call, the arena offset of every
block it touches:

  far(...)       layouts A, B0 and B: strided buffers with one huge stride, interleaved 1 MiB apart;
  table(...)     layout T: every block somewhere in one of three zones of the arena, so that
                 neighbouring table entries differ in the high word of their address;
  boundary(...)  layout V: dense buffers, an address = 0 (mod 2^32) at a chosen byte of one of them.

The small arrays of a call (rows, status, ...) sit dense in the arena's tail, the pointer tables
more than 2^32 bytes from the arena's start.  Everything here but `Arena` is plain numpy."""
import numpy as np

FRONT = 1 << 31
M32 = 1 << 32
SLACK = 16 << 20
BODY_END = FRONT + M32 + (1 << 31)       # far blocks start before this offset
ARENA_BYTES = BODY_END + SLACK
TAIL = BODY_END + (8 << 20)              # the small arrays of a call
GAP = 1 << 20                            # between the bases of a call's strided buffers
ZONE = 64 << 20                          # a zone of the table layout
CANARY = 0xA7
FAR = (1 << 31) + 16 * 5                 # layout B: offsets 0, 2^31 + 80, 2^32 + 160
FAR_ODD = (1 << 31) + 3
PLACES = ("aligned16", "lane5", "between-blocks", "between-stripes")


class Buf:
    """One buffer of a call: `offs` int64 [S, n], the arena offset of block j of stripe s, each
    `nbytes` long; `base` the offset its wrap images are taken from (the pointer passed, or the
    lowest block of a table); `stride` the stripe stride of a strided buffer (0: a table's)."""

    def __init__(self, name, offs, nbytes, base, stride=0, stripe=None):
        self.name, self.offs, self.nbytes, self.base, self.stride = name, np.asarray(offs, dtype=np.int64), int(nbytes), int(base), int(stride)
        # (the stripe a block belongs to: its row, or -1 for a pointer table, which belongs to none)
        self.stripe = np.broadcast_to(np.arange(self.offs.shape[0])[:, None] if stripe is None else stripe, self.offs.shape)

    @property
    def shape(self):
        return self.offs.shape + (self.nbytes,)

    def rel(self):
        return self.offs - self.base

    def wraps(self):
        """The two wrap images of every block's offset: (base + rel mod 2^32, base + rel
        truncated to 32 bits and sign-extended)."""
        r = self.rel()
        return self.base + r % M32, self.base + (r + (1 << 31)) % M32 - (1 << 31)


class Plan:
    def __init__(self, label, bufs, tables=(), zero=None):
        self.label, self.bufs, self.tables, self.zero = label, {b.name: b for b in bufs}, {t.name: t for t in tables}, zero

    def all(self):
        return list(self.bufs.values()) + list(self.tables.values())

    def __getitem__(self, name):
        return self.bufs[name]


def spec(name, n, nbytes, side=False):
    """A buffer of a call: n blocks of nbytes per stripe; `side`: a small dense array (rows,
    status, ...), one row of nbytes per stripe."""
    return (name, int(n), int(nbytes), bool(side))


def guard_strides(spw):
    """(layout A's stride, layout B0's stride, their stripe count is stripes_for(stride)) for a
    register-network kernel with `spw` stripes per wave (0: a stripe spans waves, counted as 1):
    the largest multiple of 16 with stride * spw < 2^31 and the smallest with stride * spw >= 2^31."""
    spw = max(1, int(spw))
    b0 = -(-(1 << 31) // spw)
    b0 = -(-b0 // 16) * 16
    a = b0 - 16
    assert a * spw < (1 << 31) <= b0 * spw and a % 16 == 0
    return a, b0


def stripes_for(stride):
    """ceil(2^32 / stride) + 1: the last stripe's base lies at or beyond 2^32."""
    return -(-M32 // int(stride)) + 1


def _sides(specs, S, at=TAIL):
    out = []
    for name, n, nbytes, side in specs:
        if side:
            at = -(-at // 64) * 64
            out.append(Buf(name, at + nbytes * np.arange(S, dtype=np.int64)[:, None], nbytes, at, nbytes))
            at += S * nbytes
    assert at <= ARENA_BYTES, "the small arrays outgrow the arena's tail"
    return out


def _dense(name, base, S, n, nbytes):
    offs = base + (np.arange(S, dtype=np.int64)[:, None] * n + np.arange(n, dtype=np.int64)[None, :]) * nbytes
    return Buf(name, offs, nbytes, base, n * nbytes)


def far(label, specs, S, stride, far_names=None):
    """Layouts A, B0, B: block buffer i starts at FRONT + i * GAP; those in `far_names` (default:
    all) take `stride`, the others their dense stride."""
    bufs, i = [], 0
    for name, n, nbytes, side in specs:
        if side:
            continue
        base = FRONT + i * GAP
        i += 1
        assert n * nbytes <= GAP and stride >= 8 * GAP, "a stripe outgrows its share of the stride gap"
        if far_names is None or name in far_names:
            offs = base + np.arange(S, dtype=np.int64)[:, None] * stride + np.arange(n, dtype=np.int64)[None, :] * nbytes
            bufs.append(Buf(name, offs, nbytes, base, stride))
        else:
            assert S * n * nbytes <= GAP
            bufs.append(_dense(name, base, S, n, nbytes))
        assert bufs[-1].offs.max() + nbytes <= TAIL
    return Plan(label, bufs + _sides(specs, S))


def zero_offset(arena_base, at_least=FRONT + (64 << 20)):
    """The first arena offset >= at_least whose virtual address is a multiple of 2^32."""
    return at_least + (-(arena_base + at_least)) % M32


def _table_spot(busy, size):
    """An 8-aligned arena offset beyond 2^32 at least 128 MiB from every busy interval."""
    for c in range(M32 + (1 << 28), BODY_END - (1 << 28), 1 << 27):
        if all(c + size + (1 << 27) <= lo or hi + (1 << 27) <= c for lo, hi in busy):
            return c
    raise AssertionError("no room for the pointer tables")


def _tables(bufs, busy):
    """One table per block buffer, int64 [S, n], 64 KiB-aligned one after the other."""
    sizes = [-(-b.offs.size * 8 // 65536) * 65536 for b in bufs]
    at = _table_spot(busy, sum(sizes))
    out = []
    for b, sz in zip(bufs, sizes):
        out.append(Buf(b.name + " table", [[at]], b.offs.size * 8, at, 0, stripe=-1))
        at += sz
    return out


def block_points(n, nbytes):
    """The byte of a stripe of n blocks at which each of PLACES puts the 2^32 boundary (block
    n // 2), or None where the shape has no such byte."""
    j = n // 2
    x16 = 16 * max(1, nbytes // 32) if nbytes > 16 else None
    x5 = 8 * ((nbytes // 8) // 2) + 5
    return {"aligned16": None if x16 is None else j * nbytes + x16,
            "lane5": j * nbytes + x5 if x5 < nbytes else None,
            "between-blocks": j * nbytes if j >= 1 else None,
            "between-stripes": 0}


def boundary(label, specs, S, arena_base, subject, place, tables=False):
    """Layout V: every buffer dense; the address = 0 (mod 2^32) lies at byte block_points()[place]
    of stripe S // 2 of `subject` (between-stripes: where that stripe starts).  None when the
    shape has no such byte."""
    zero = zero_offset(arena_base)
    bufs, i = [], 0
    for name, n, nbytes, side in specs:
        if side:
            continue
        if name == subject:
            point = block_points(n, nbytes)[place]
            if point is None:
                return None
            base = zero - ((S // 2) * n * nbytes + point)
        else:
            base = zero + (256 << 20) + i * (64 << 20)
            i += 1
        assert S * n * nbytes <= (32 << 20)
        bufs.append(_dense(name, base, S, n, nbytes))
    busy = [(zero - (64 << 20), zero + (256 << 20) + (i + 1) * (64 << 20))]
    return Plan(label, bufs + _sides(specs, S), _tables(bufs, busy) if tables else (), zero)


def table(label, specs, S, arena_base, seed=0):
    """Layout T: three zones, P at FRONT, R at FRONT + 2^30 and Q at the end of the arena's body,
    Q more than 2^32 bytes from both others, so its addresses differ from theirs in the high
    word wherever the arena lies.  Entry j of stripe s lies in Q when s + j is odd, else in P or R
    by turns; inside a zone the blocks take random slots at random byte offsets 0 .. 15."""
    zones = (FRONT, FRONT + (1 << 30), BODY_END - ZONE)
    blocks = [(name, n, nbytes) for name, n, nbytes, side in specs if not side]
    pitch = max(b[2] for b in blocks) + 16
    total = sum(S * b[1] for b in blocks)
    assert total * pitch <= ZONE, "the blocks outgrow a zone"
    for attempt in range(32):
        rng = np.random.Generator(np.random.PCG64(seed * 64 + attempt))
        slots = rng.permutation(ZONE // pitch)[:total]
        odd = rng.integers(0, 16, size=total)
        bufs, at = [], 0
        for name, n, nbytes in blocks:
            s, j = np.meshgrid(np.arange(S), np.arange(n), indexing="ij")
            zone = np.where((s + j) % 2 == 1, zones[2], np.where((s + j // 2) % 2 == 0, zones[0], zones[1]))
            offs = zone + (slots[at:at + S * n] * pitch + odd[at:at + S * n]).reshape(S, n)
            at += S * n
            bufs.append(Buf(name, offs, nbytes, int(offs.min())))
        busy = [(z - (1 << 20), z + ZONE + (1 << 20)) for z in zones]
        plan = Plan(label, bufs + _sides(specs, S), _tables(bufs, busy))
        if not problems(plan, arena_base, far=True):
            return plan
    raise AssertionError(("no table layout without a clashing wrap image", label, problems(plan, arena_base, far=True)[:3]))


# ------------------------------------------------------------------ the planner's properties
def _intervals(plan):
    rows = []
    for bi, b in enumerate(plan.all()):
        rows.append(np.stack([b.offs.reshape(-1), b.offs.reshape(-1) + b.nbytes, b.stripe.reshape(-1),
                              np.full(b.offs.size, bi)], axis=1))
    iv = np.concatenate(rows)
    return iv[np.argsort(iv[:, 0], kind="stable")]


def problems(plan, arena_base, far):
    """What breaks the planner's properties 1, 2, 3 and 5 (tests/test_lhfar.py), as a list of
    strings; empty when the plan is good.  `far`: the layout promises offsets beyond 2^31 and
    2^32 from a batch base (A, B0, B, T); V promises its boundary instead."""
    out = []
    iv = _intervals(plan)
    if (iv[:, 0] < FRONT).any() or (iv[:, 1] > ARENA_BYTES).any():
        out.append("a block lies before FRONT or beyond the arena")
    if (iv[1:, 0] < iv[:-1, 1]).any():
        out.append("two touched blocks overlap")
    if far:   # 1
        rel = np.concatenate([b.rel().reshape(-1) for b in plan.bufs.values()])
        if not ((rel >= (1 << 31)).any() and (rel >= M32).any()):
            out.append("no touched offset beyond 2^31 and 2^32 from its batch base")
    starts, ends = iv[:, 0], iv[:, 1]
    for b in plan.all():
        for kind, img in zip(("uint32", "int32"), b.wraps()):
            img, own = img.reshape(-1), b.offs.reshape(-1)
            moved = img != own
            if (img < 0).any() or (img + b.nbytes > ARENA_BYTES).any():   # 2
                out.append(f"{b.name}: a {kind} wrap image leaves the arena")
                continue
            # 3: every touched block an image [img, img + nbytes) overlaps
            lo = np.searchsorted(ends, img, side="right")
            hi = np.searchsorted(starts, img + b.nbytes, side="left")
            st = b.stripe.reshape(-1)
            for i in np.nonzero(moved & (hi > lo))[0]:
                hit = iv[lo[i]:hi[i]]
                if (hit[:, 2] < 0).any() or st[i] < 0 or (hit[:, 2] == st[i]).any():
                    out.append(f"{b.name}: the {kind} image of a block of stripe {int(st[i])} at offset {int(own[i])} "
                               f"overlaps a block of the same stripe or a pointer table at {int(hit[0, 0])}")
                    break
    if plan.zero is not None and (arena_base + plan.zero) % M32 != 0:   # 5
        out.append("the 2^32 boundary is not where the plan says")
    return out


def table_properties(plan, arena_base):
    """Layout T's own promises, as problems(): neighbouring entries of a row differ in the high
    word of their address, some entries lie more than 2^32 apart, some addresses are odd, the
    tables lie beyond 2^32 from the arena's start."""
    out = []
    for t in plan.tables.values():
        if t.base < M32 or (arena_base + t.base) % 8:
            out.append(f"{t.name} lies within 2^32 of the arena's start or is misaligned")
    for b in plan.bufs.values():
        if b.name + " table" not in plan.tables:
            continue
        addr = arena_base + b.offs
        if b.offs.shape[1] > 1 and ((addr[:, 1:] >> 32) == (addr[:, :-1] >> 32)).any():
            out.append(f"{b.name}: neighbouring entries share a high word")
        if b.offs.size > 1 and addr.max() - addr.min() <= M32:
            out.append(f"{b.name}: no two entries more than 2^32 apart")
        if not (addr % 2 == 1).any():
            out.append(f"{b.name}: no odd address")
    return out


def boundary_at(plan, arena_base, subject):
    """Where layout V's 2^32 boundary falls in `subject`: (stripe, block, byte), byte 0 meaning
    exactly before that block (block 0: exactly before that stripe)."""
    b = plan[subject]
    assert (arena_base + plan.zero) % M32 == 0
    o = plan.zero - b.base
    S, n = b.offs.shape
    assert 0 <= o < S * n * b.nbytes
    return int(o // (n * b.nbytes)), int(o % (n * b.nbytes) // b.nbytes), int(o % b.nbytes)


# ------------------------------------------------------------------ the arena on the device
class Arena:
    """The device allocation.  put / take move a buffer's blocks by their offsets; `sweep` is the
    check after a call: the touched blocks copied out, overwritten with the canary, then the
    whole arena compared with the canary (one reduction per GiB on an int64 view, the flags read
    once), which leaves it clean for the next case."""
    PIECE = 1 << 27   # int64 elements: 1 GiB

    def __init__(self):
        import torch
        self.t = torch.full((ARENA_BYTES,), CANARY, dtype=torch.uint8, device="cuda")
        self.base = self.t.data_ptr()
        self.words = self.t.view(torch.int64)
        self.canary64 = int(np.full(8, CANARY, dtype=np.uint8).view(np.int64)[0])

    def free(self):
        import torch
        self.t = self.words = None
        torch.cuda.empty_cache()

    def index(self, buf):
        import torch
        offs = torch.from_numpy(np.ascontiguousarray(buf.offs.reshape(-1))).cuda()
        return (offs[:, None] + torch.arange(buf.nbytes, dtype=torch.int64, device="cuda")[None, :]).reshape(-1)

    def put(self, buf, values):
        import torch
        v = values if isinstance(values, torch.Tensor) else torch.from_numpy(np.array(values)).cuda()
        assert v.dtype == torch.uint8 and v.numel() == buf.offs.size * buf.nbytes, (buf.name, tuple(v.shape), buf.shape)
        self.t[self.index(buf)] = v.reshape(-1)

    def take(self, buf):
        return self.t[self.index(buf)].reshape(buf.shape)

    def ptr(self, buf):
        return self.base + buf.base

    def sweep(self, plan):
        """Returns ({name: the buffer's bytes after the call}, None or where the first byte
        outside every touched block was overwritten)."""
        import torch
        got = {}
        for b in plan.all():
            idx = self.index(b)
            got[b.name] = self.t[idx].reshape(b.shape)
            self.t[idx] = CANARY
        n = self.words.numel()
        flags = torch.stack([(self.words[a:min(n, a + self.PIECE)] != self.canary64).any() for a in range(0, n, self.PIECE)])
        dirty = flags.cpu().numpy()            # (the one read)
        if not dirty.any():
            return got, None
        a = int(np.nonzero(dirty)[0][0]) * self.PIECE
        piece = self.t[a * 8:min(n, a + self.PIECE) * 8]
        at = a * 8 + int(torch.nonzero(piece != CANARY)[0, 0])
        count = sum(int((self.t[p * 8:min(n, p + self.PIECE) * 8] != CANARY).sum()) for p in range(0, n, self.PIECE))
        self.t.fill_(CANARY)
        return got, f"{count} bytes outside every touched block were written, the first at arena offset {at} ({_near(plan, at)})"


def _near(plan, at):
    best = None
    for b in plan.all():
        d = at - b.offs
        d = np.where(d >= 0, d, 1 << 62)
        i = np.unravel_index(np.argmin(d), d.shape)
        if best is None or d[i] < best[0]:
            best = (int(d[i]), b.name, int(i[0]), int(i[1]))
    if best[0] >= 1 << 62:
        return f"before every touched block; FRONT - {FRONT - at}" if at < FRONT else f"FRONT + {at - FRONT}"
    return f"{best[0]} bytes after the start of {best[1]} stripe {best[2]} block {best[3]}; FRONT + {at - FRONT}"
