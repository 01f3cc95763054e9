"""G32 views whose bytes lie beyond 2^31 and 2^32 from the view's pointer, inside ONE device allocation (the arena) laid
out so that a kernel with a missing 64-bit cast reads or writes the wrong place INSIDE the arena instead of faulting.

The arena is a uint8 tensor of at most ARENA_MAX bytes filled with FILL (0x3C: every fp16 is 1.0586, every fp32 0.0115
— finite).  A view's pointer sits PTR_OFF = 2 GiB + 64 MiB past the arena's start, so for a byte at true offset o from
the pointer all three of ptr + o, ptr + (int32)o and ptr + (uint32)o lie in the arena as long as o < arena - PTR_OFF:
(int32)o >= -2^31 > -PTR_OFF, and (uint32)o <= o.  fits() proves it per case from this arithmetic alone.

A "window" is the Hp x Wp rectangle of one (image, group) of a compact buffer (engine.G32: Hp, Wp from esr_g32_dims).
Families (the strides of the far view; maps stay small):
  batch   batch_stride = FAR = 2^31 + 2^20, group stride and pitch as the compact buffer's.  B <= 3: image 1 starts past
          2^31, image 2 past 2^32.
  group   group_stride = FAR, at most 4 groups: group 1 starts past 2^31, groups 2 and 3 past 2^32.  The images of all
          buffers lie side by side below 2^20 (batch_stride = one window): legal wherever the kernel only ADDS the strides.
  plane   pitch wp = the largest with Hp * wp * 32 < 2^31 (the plane limit engine.G32 enforces), group_stride = that
          plane, at most 2 groups; the images of all buffers are column slots of the long rows (batch_stride = Wp * 32).
          The last rows of group 0 sit just under 2^31, group 1 beyond it.
relocate() rewrites every esr_g32 of a ctypes op struct (and of a host copy of its device block table) from compact
engine.G32 buffers to far views of one family and copies the windows; gather() reads them back — the tests compare
them whole, sentinels included, with the compact buffers — and scan() checks on the device that no byte outside the
windows changed."""
import ctypes as C

FILL = 0x3C
ARENA_MAX = 9 << 30
PTR_OFF = (2 << 30) + (64 << 20)
FAR = (1 << 31) + (1 << 20)
TAIL = 64 << 20                 # slack behind the last window (tile overhang / wrap-around reads stay inside)
CHUNK = 256 << 20               # scan granularity
SPAN = 512 << 20                # most that the windows of one case may take below one far stride
FAMILIES = ('batch', 'group', 'plane')
MAX_GROUPS = {'batch': 64, 'group': 4, 'plane': 2}
MAX_BATCH = {'batch': 3, 'group': 1 << 16, 'plane': 1 << 16}


class Unfit(Exception):
    """the case cannot satisfy the arena property in this family: it is not launched"""


def g32_dims(H, W):
    """esr_g32_dims restated (the host tests pin it against the library)"""
    return (H + 31) // 32 * 32 + 6, (W + 31) // 32 * 32 + 2


def i32(o):
    o &= 0xFFFFFFFF
    return o - (1 << 32) if o >= 1 << 31 else o


def u32(o):
    return o & 0xFFFFFFFF


def plane_wp(Hp):
    """the largest pitch (pixels) whose Hp-row plane stays below 2^31 bytes"""
    return ((1 << 31) - 1) // (Hp * 32)


class FarBuf:
    """one compact buffer's place in the arena: byte offsets are from the view pointer base (arena start + PTR_OFF)"""

    def __init__(self, family, base, B, ng, Hp, Wp, bs, gs, wp):
        self.family, self.base, self.B, self.ng, self.Hp, self.Wp = family, base, B, ng, Hp, Wp
        self.bs, self.gs, self.wp = bs, gs, wp

    def windows(self):
        """(b, g, first byte, last byte + 1) of every window, offsets from base 0 = the family's common pointer base"""
        span = (self.Hp - 1) * self.wp * 32 + self.Wp * 32
        for b in range(self.B):
            for g in range(self.ng):
                lo = self.base + b * self.bs + g * self.gs
                yield b, g, lo, lo + span

    def strided(self, arena):
        """the windows as a [B][ng][Hp][Wp * 32] byte view of the arena tensor"""
        return arena.as_strided((self.B, self.ng, self.Hp, self.Wp * 32), (self.bs, self.gs, self.wp * 32, 1),
                                PTR_OFF + self.base)


def plan(family, shapes):
    """shapes: (B, groups, Hp, Wp) of every compact buffer of a case -> its FarBufs.  Raises Unfit."""
    out, at = [], 0
    for B, ng, Hp, Wp in shapes:
        if ng > MAX_GROUPS[family] or B > MAX_BATCH[family] or ng < 1:
            raise Unfit('%s family: B %d, %d groups' % (family, B, ng))
        win = Hp * Wp * 32
        if family == 'batch':
            fb = FarBuf(family, at, B, ng, Hp, Wp, FAR, win, Wp)
            at += (ng * win + 4095) // 4096 * 4096
        elif family == 'group':
            fb = FarBuf(family, at, B, ng, Hp, Wp, win, FAR, Wp)
            at += B * win
        else:
            wp = plane_wp(Hp)
            fb = FarBuf(family, at, B, ng, Hp, Wp, Wp * 32, Hp * wp * 32, wp)
            at += B * Wp * 32
            if at > min(plane_wp(s[2]) for s in shapes) * 32:
                raise Unfit('plane family: the column slots do not fit one row')
        out.append(fb)
    if family != 'plane' and at > SPAN:
        # what lies side by side below one far stride: far less than the stride, so images / groups never overlap and
        # the arena stays below ARENA_MAX
        raise Unfit('%s family: %d bytes of windows per stride' % (family, at))
    return out


def extent(fbs):
    """one past the last window byte (offset from the pointer base)"""
    return max(hi for fb in fbs for *_, hi in fb.windows())


def arena_bytes(fbs):
    return PTR_OFF + extent(fbs) + TAIL


def fits(fbs, arena=ARENA_MAX):
    """the arena property, from arithmetic alone: for every window byte o (offset from the buffer's own view pointer,
    which is PTR_OFF + base into the arena) ptr + o, ptr + (int32)o and ptr + (uint32)o are inside [0, arena).  The
    truncations are monotone between multiples of 2^31, so the ends of every window and the multiples inside it
    decide."""
    if arena_bytes(fbs) > arena:
        return False
    for fb in fbs:
        ptr = PTR_OFF + fb.base
        for b, g, lo, hi in fb.windows():
            lo, hi = lo - fb.base, hi - fb.base
            pts = {lo, hi - 1}
            k = (lo >> 31) + 1
            while k << 31 < hi:
                pts |= {(k << 31) - 1, k << 31}
                k += 1
            for o in pts:
                for a in (ptr + o, ptr + i32(o), ptr + u32(o)):
                    if not 0 <= a < arena - 32:
                        return False
    return True


def crossings(fbs):
    """(# windows wholly in [2^31, 2^32), # windows wholly past 2^32, largest window end below 2^31), offsets from
    each buffer's own pointer: what a family claims to cross"""
    mid = far = 0
    near = 0
    for fb in fbs:
        for b, g, lo, hi in fb.windows():
            lo, hi = lo - fb.base, hi - fb.base
            if lo >= 1 << 32:
                far += 1
            elif lo >= 1 << 31 and hi <= 1 << 32:
                mid += 1
            elif hi <= 1 << 31:
                near = max(near, hi)
    return mid, far, near


# ----------------------------------------------------------------------------------------------------------------
# device side
# ----------------------------------------------------------------------------------------------------------------

class Arena:
    """the one device allocation; place() / gather() / scan() / clear() work on a list of FarBufs"""

    def __init__(self, dev, nbytes=ARENA_MAX):
        import torch
        assert nbytes <= ARENA_MAX and nbytes % 8 == 0
        self.t = torch.full((nbytes,), FILL, dtype=torch.uint8, device=dev)
        self.n = nbytes

    def ptr(self, fb):
        return self.t.data_ptr() + PTR_OFF + fb.base

    @staticmethod
    def _bytes(t, ng):
        """a compact [B][groups][Hp][Wp][cpg] tensor's first ng groups as [B][ng][Hp][Wp * 32] bytes"""
        import torch
        B, G, Hp, Wp, _ = t.shape
        return t.view(torch.uint8).reshape(B, G, Hp, Wp * 32)[:, :ng]

    def place(self, fb, t):
        assert fits([fb], self.n)
        fb.strided(self.t).copy_(self._bytes(t, fb.ng))

    def gather(self, fb):
        return fb.strided(self.t).clone()

    def clear(self, fbs):
        for fb in fbs:
            fb.strided(self.t).fill_(FILL)

    def scan(self, fbs):
        """True when every byte outside the windows of fbs holds FILL (the windows are blanked for the pass and put
        back); device work in chunks of CHUNK bytes, one synchronisation"""
        import torch
        saved = [self.gather(fb) for fb in fbs]
        self.clear(fbs)
        words = self.t.view(torch.int64)
        pat = int.from_bytes(bytes([FILL]) * 8, 'little')
        bad = torch.zeros((), dtype=torch.bool, device=self.t.device)
        step = CHUNK // 8
        for i in range(0, words.numel(), step):
            bad |= (words[i:i + step] != pat).any()
        for fb, s in zip(fbs, saved):
            fb.strided(self.t).copy_(s)
        return not bool(bad.item())


def _g32_fields(st):
    return [n for n, tp in st._fields_ if getattr(tp, '__name__', '') == 'esr_g32']


class Relocated:
    """what relocate() returns: the rewritten struct(s), the FarBufs in the order of `bufs`, and those a view used"""

    def __init__(self, op, fbs, used, table=None):
        self.op, self.fbs, self.used, self.table = op, fbs, used, table


def _find(v, bufs):
    for i, b in enumerate(bufs):
        p0 = b.t.data_ptr()
        if p0 <= v.ptr < p0 + b.t.numel() * b.t.element_size():
            return i
    raise KeyError('a view points into none of the buffers given')


def view_groups(structs, bufs, keep=()):
    """groups of every buffer that some view of the structs can address: max over the views of g0 + ngroups"""
    ng = [0] * len(bufs)
    for st in structs:
        for name in _g32_fields(st):
            v = getattr(st, name)
            if not v.ptr:
                continue
            i = _find(v, bufs)
            if any(bufs[i] is k for k in keep):
                continue
            b = bufs[i]
            g0 = ((v.ptr - b.t.data_ptr()) % b.bs) // b.gs
            ng[i] = max(ng[i], g0 + v.ngroups)
    return ng


def relocate(op, bufs, family, arena, contents=None, table=None, extra_groups=None, keep=()):
    """op: a ctypes op struct over views of the compact engine.G32 buffers `bufs`; table: a host ctypes array (the
    esr_rdb_block / esr_rdb_wgrad_block table the op's `blocks` pointer names on the device), rewritten too — the caller
    uploads it.  contents: the tensors to copy into the windows (default: the buffers' own, as they are now).  keep: buffers
    whose views stay where they are (views with strides of their own, such as the band views of the banded chain).
    Returns a Relocated; raises Unfit (nothing is copied) when the case does not fit the family."""
    structs = [op] + (list(table) if table is not None else [])
    ng = view_groups(structs, bufs, keep)
    if extra_groups:
        ng = [max(a, b) for a, b in zip(ng, extra_groups)]
    used = [i for i, n in enumerate(ng) if n]
    fbs_used = plan(family, [(bufs[i].B, min(ng[i], bufs[i].ng), bufs[i].Hp, bufs[i].Wp) for i in used])
    if not fits(fbs_used, arena.n if arena is not None else ARENA_MAX):
        raise Unfit('%s family: outside the arena' % family)
    fbs = [None] * len(bufs)
    for i, fb in zip(used, fbs_used):
        fbs[i] = fb
        if arena is not None:
            arena.place(fb, (contents[i] if contents is not None else bufs[i].t))
    base = arena.t.data_ptr() if arena is not None else 0

    def rewrite(st):
        new = type(st).from_buffer_copy(st)
        for name in _g32_fields(st):
            v = getattr(new, name)
            if not v.ptr:
                continue
            i = _find(v, bufs)
            b, fb = bufs[i], fbs[i]
            if any(b is k for k in keep):
                continue
            if (v.batch_stride, v.group_stride, v.wp) != (b.bs, b.gs, b.Wp):
                raise Unfit('a view with strides of its own')
            off = v.ptr - b.t.data_ptr()
            b0, rem = divmod(off, b.bs)
            g0, inpl = divmod(rem, b.gs)
            row, col = divmod(inpl, b.Wp * 32)
            v.ptr = base + PTR_OFF + fb.base + b0 * fb.bs + g0 * fb.gs + row * fb.wp * 32 + col
            v.batch_stride, v.group_stride, v.wp = fb.bs, fb.gs, fb.wp
        return new
    new_table = None
    if table is not None:
        new_table = (type(table[0]) * len(table))(*[rewrite(e) for e in table])
    return Relocated(rewrite(op), fbs, fbs_used, new_table)
