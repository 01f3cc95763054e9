"""Host-side launch planner for the HIP hot path.

Turns one pass of a drop-in module (``RRDBNet.forward`` — reference
codes/models/modules/architecture.py:76-78 — or a single ``ResidualDenseBlock_5C`` / ``RRDB``,
block.py:260-268 / 287-291) into a recorded list of fused-conv launches over G32 buffers
(include/esrgan_hip.h) that ONE C call replays on torch's current HIP stream.

torch is used here for device memory (buffers are torch tensors) and the stream handle only.
"""
import collections
import contextlib
import ctypes as C
import os

import torch

from . import _lib as L
from .packs import ConvW, DgradPack, RdbBwdStreams, RdbStreams, WeightPack, _dt, require_cuda  # noqa: F401 (re-exported)

SIGMA = 0.1   # GaussianNoise sigma (block.py:111)

_STORE_FLAVOUR = int(os.environ.get('ESR_STORE_FLAVOUR', '0'))   # experiment knob: 1 = nt epilogue stores


# ESR_SIDE=0: weight-gradient runs on the launch stream instead of the side stream (A/B)
_SIDE = L.OPF_SIDE if os.environ.get('ESR_SIDE', '1') != '0' else 0
_SIDE_FREE = L.OPF_SIDE_FREE if os.environ.get('ESR_TAIL_WGRAD_FREE', '1') != '0' else 0     # (A/B knob, round 5)

OFFSET_LIMIT = 2 ** 31    # bytes a 32-bit offset inside one image / one channel-group plane can span (G32.__init__)


class G32:
    """[B][ngroups][Hp][Wp][cpg] activation buffer with a physical zero halo."""

    def __init__(self, B, C_, H, W, dtype, device, image_limit=False):
        self.esr_dtype, self.tdtype, self.cpg = _dt(dtype)
        self.B, self.C, self.H, self.W = B, C_, H, W
        self.ng = (C_ + self.cpg - 1) // self.cpg
        self.Hp, self.Wp = L.g32_dims(H, W)
        # The kernels add the image's byte offset (b * batch_stride) in 64 bits, but inside an image some offsets are
        # 32-bit: the conv kernels' staging map inside one channel-group plane (conv_mfma.hip: goff), the fp16
        # weight-gradient kernel's across the groups of one image (wgrad.hip: soff / poff = group * group_stride + ...),
        # the fused chains' likewise (rdb_chain_kernel.h: one buffer descriptor per image).  DESIGN.md 2a has the table.
        # Refused here, before anything is allocated: a plane (every plan) or — image_limit: the training plans, whose
        # buffers the weight-gradient kernels read, and the banded trunk's tall buffers (band_buffers) — one image's
        # extent of OFFSET_LIMIT bytes or more.
        extent = (self.ng if image_limit else 1) * self.Hp * self.Wp * 32
        if extent >= OFFSET_LIMIT:
            raise ValueError('a %d-channel %s buffer of %d x %d pixels spans %d bytes per %s: the kernels address %s with '
                             '32-bit offsets (limit 2^31 bytes) — use a smaller image, or forward_tiled for x4 inference'
                             % (C_, dtype, H, W, extent, 'image' if image_limit else 'channel-group plane',
                                'one image' if image_limit else 'a plane'))
        self.t = torch.zeros(B, self.ng, self.Hp, self.Wp, self.cpg, dtype=self.tdtype, device=device)
        self.gs = self.Hp * self.Wp * 32
        self.bs = self.ng * self.gs

    def view(self, c0=0, nch=None, row0=0):
        """esr_g32 view starting at channel c0 (must be group aligned) and, for the taller buffers of the banded
        chain, at row row0 (the rows above / below the view's image are zero padding that nothing writes)."""
        assert c0 % self.cpg == 0, (c0, self.cpg)
        g0 = c0 // self.cpg
        ng = self.ng - g0 if nch is None else (nch + self.cpg - 1) // self.cpg
        v = L.esr_g32()
        v.ptr = self.t.data_ptr() + g0 * self.gs + row0 * self.Wp * 32
        v.batch_stride = self.bs
        v.group_stride = self.gs
        v.wp = self.Wp
        v.ngroups = ng
        return v

    def groups(self, nch):
        return (nch + self.cpg - 1) // self.cpg


def use_train_chain(dtype_e, B, H, W, explicit_z):
    """fp16 training passes run the dense blocks as fused chains — training forward (esr_rdb_chain.mode 1) and
    backward (esr_rdb_backward) — when the image fits the chain (all tiles co-resident) and z is the fused Philox
    stream (explicit z: per-conv launches).  ESR_RDB_TRAIN_CHAIN=0 restores the per-conv training plan."""
    if dtype_e != L.ESR_F16 or explicit_z or os.environ.get('ESR_RDB_TRAIN_CHAIN', '1') == '0':
        return False
    return rdb_chain_ok(B, H, W, False, False)


def rdb_chain_ok(B, H, W, noise, explicit_z):
    """The fused dense-block chain handles eval / fused-Philox passes whose images have at most
    esr_rdb_max_tiles_per_image() 16x32 tiles (all tiles of an image are co-resident, one per CU)."""
    if os.environ.get('ESR_RDB_FUSED', '1') == '0' or (noise and explicit_z):
        return False
    tpi = ((H + 15) // 16) * ((W + 31) // 32)
    return tpi <= L.lib().esr_rdb_max_tiles_per_image()


def use_rdb_bands(dtype_e, H, W):
    """Images with more tiles than CUs: the fused trunk in row bands for fp16 (339x510, nb=23: 9.2 ms against 10.3 ms
    of per-conv launches); fp32 keeps the per-conv launches, which are 6 % faster there (73.5 / 68.9 ms,
    tools/big_image_probe.py).  ESR_RDB_BANDS=1 forces bands for both, =0 turns them off."""
    mode = os.environ.get('ESR_RDB_BANDS', 'auto')
    if mode == '0' or os.environ.get('ESR_RDB_FUSED', '1') == '0' or rdb_band_geometry(H, W) is None:
        return False
    return mode == '1' or dtype_e == L.ESR_F16


def rdb_band_geometry(H, W):
    """Row bands for an image with more 16x32 tiles than CUs (include/esrgan_hip.h: esr_rdb_chain.band_rows):
    (band_rows, band_margin, n_bands), or None when not even a one-tile-row band fits (W > 32 * CUs / 3).
    One launch runs the three dense blocks of an RRDB, so a band recomputes 15 rows of each neighbour: margin 16
    (a whole tile row), bands as tall as the CU count allows and evened out over the image."""
    margin = 16
    tiles_x = (W + 31) // 32
    t = L.lib().esr_rdb_max_tiles_per_image() // tiles_x - 2 * (margin // 16)
    if t < 1:
        return None
    n = (H + 16 * t - 1) // (16 * t)
    rows = ((H + n - 1) // n + 15) // 16 * 16
    return rows, margin, n


def band_buffers(B, geom, W, dtype, device):
    """The buffers of the banded trunk (Builder.rdb_chain_banded): two `tall` 64-channel images with band_margin rows of
    padding above and below, and the band-local block output and dense scratch.  A band's views keep the tall buffer's
    group stride, and the chain kernels reach the groups of a band through one buffer descriptor with 32-bit offsets
    (include/esrgan_hip.h, esr_g32): the tall buffers take the per-image limit, so a tall, narrow image whose four
    planes pass 2^31 bytes is refused here instead of losing the stores of its last groups."""
    S, m, nbands = geom
    hb = S + 2 * m
    tall = [G32(B, 64, nbands * S + 2 * m, W, dtype, device, image_limit=True) for _ in range(2)]
    return tall, G32(nbands, 64, hb, W, dtype, device), G32(nbands, 128, hb, W, dtype, device)


def _conv(dtype_e, B, H, W, src, src_ch, dst, cw, act=L.ACT_NONE, ks=None, stride=1, upsample=0):
    c = L.esr_conv()
    c.dtype = dtype_e
    c.ks = cw.ks if ks is None else ks
    c.stride = stride
    c.upsample = upsample
    if upsample == 1 and getattr(cw, 'subpix', False):    # same function, 4-phase 2x2 form
        c.ks, c.upsample = 2, 3
    c.B, c.H, c.W = B, H, W
    cpg = 16 if dtype_e == L.ESR_F16 else 8
    c.cin_groups = (src_ch + cpg - 1) // cpg
    c.cout_blocks = (cw.cout + 31) // 32
    c.in_ = src
    if dst is not None:
        c.out = dst
    c.w = cw.w_ptr
    c.bias = cw.bias_ptr
    c.act = act
    c.alpha = 1.0
    c.beta = 1.0
    c.sigma = SIGMA
    c.noise_mode = L.NOISE_OFF
    c.layer1 = L.NO_LAYER
    c.layer2 = L.NO_LAYER
    c.layer3 = L.NO_LAYER
    c.gamma = 1.0
    c.mask_act = L.ACT_LRELU
    c.debug_flags = (_STORE_FLAVOUR << 3) | (int(os.environ.get('ESR_DBG', '0')) & ~7)
    return c


def upload_table(table, device):
    """A ctypes array as a device tensor (the caller keeps it alive as long as an op points at it)."""
    return torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(device)


class PinnedRing:
    """Small per-call tables on their way to the device without a synchronisation: a table is written into a pinned host
    buffer and copied to a FRESH device tensor on the current stream (the caching allocator does not hand that tensor out
    again before the launches that read it have run).  What the next call must not overwrite is the pinned buffer while
    its copy is in flight: a ring of `n` pinned buffers, each guarded by an event recorded behind its copy.  A slot is
    waited for only when the ring has gone round, n calls later — a wait for one small copy, not a device
    synchronisation.  (data.TrainSet's item tables, the slot tables of the tiled forward over an image set.)"""

    def __init__(self, n=4):
        self.n, self.slots, self.calls = n, [], 0

    def slot(self, nbytes):
        """The next [pinned uint8 buffer of at least nbytes, event behind its last copy or None]."""
        k = self.calls % self.n
        self.calls += 1
        if k == len(self.slots):
            self.slots.append([None, None])
        slot = self.slots[k]
        if slot[1] is not None:
            slot[1].synchronize()                     # the copy that read this slot n calls ago
        if slot[0] is None or slot[0].numel() < nbytes:
            slot[0] = torch.empty(max(nbytes, 4096), dtype=torch.uint8).pin_memory()
        return slot

    def upload(self, rec, device, out=None):
        """The 1-D numpy array `rec` as a fresh uint8 device tensor: one non-blocking copy on the current stream.  `out`:
        that tensor, allocated by a caller whose table holds addresses inside itself."""
        nbytes = rec.nbytes
        slot = self.slot(nbytes)
        slot[0].numpy()[:nbytes].view(rec.dtype)[:] = rec
        table = torch.empty(nbytes, dtype=torch.uint8, device=device) if out is None else out
        assert table.numel() == nbytes and table.dtype == torch.uint8 and table.is_contiguous()
        table.copy_(slot[0][:nbytes], non_blocking=True)
        if slot[1] is None:
            slot[1] = torch.cuda.Event()
        slot[1].record()
        return table


class NoiseLayers:
    """Ids of the GaussianNoise layers in execution order (the Philox stream and explicit z tensors are indexed by
    them): per RRDB its three dense blocks, then — test_image/block.py:250,256 — the RRDB's own stage.  kind 'net':
    nb RRDBs; 'rrdb': one; 'rdb': a single dense block.  on=False (eval mode): no layers, every id is None."""

    def __init__(self, variant, kind, nb, on=True):
        self.on = bool(on)
        self.extra = variant == 'test_image' and kind != 'rdb'
        self.per = 4 if variant == 'test_image' else 3
        self.total = 0 if not on else (1 if kind == 'rdb' else self.per * (nb if kind == 'net' else 1))

    def rdb(self, i, j):
        """Dense block j of RRDB i."""
        return self.per * i + j if self.on else None

    def rrdb(self, i):
        """The extra stage behind RRDB i's residual (test_image only)."""
        return self.per * i + 3 if self.on and self.extra else None


def _layer(lid):
    return L.NO_LAYER if lid is None else lid


class Plan:
    """A recorded forward pass for one (module, input shape, dtype, mode)."""

    def __init__(self):
        self.ops = L.OpList()
        self.bufs = []
        self.in_op = None        # index of the NCHW->G32 layout op of the input
        self.out_op = None       # index of the op producing the NCHW output
        self.out_shape = None
        self.ends = None         # the Ends behind in_op / out_op of an RRDBNet plan (bind)
        self.noise_ops = []      # (op index, which) of convs carrying a noise epilogue
        self.chain_ops = []      # indices of OP_RDB_CHAIN ops (noise mode / seed set per run)
        self.chain_ws = None     # workspace of the chain ops (word 1: a bounded spin of the chain kernel timed out)
        self.streams = None      # RdbStreams feeding the chain ops
        self.z_ops = []          # layout ops that import explicit z tensors, in noise-layer order
        self.wgen = None
        self.chain_noise = False
        self.graph_bound = False   # TrainPlan.enable_graph: the chain ops read their seed from the device

    def bind(self, **values):
        """Per-run values of the two end ops, by the names of the plan's Ends.per_run."""
        self.ends.bind(self, **values)

    def run(self, x, out, stream, seed=0, zs=None):
        arr = self.ops.array()
        set_nchw(arr[self.in_op], x.data_ptr())
        set_nchw(arr[self.out_op], out.data_ptr())
        mode = L.NOISE_OFF
        if not self.graph_bound:
            for i in self.chain_ops:
                ch = arr[i].u.rdb_chain
                ch.noise_mode = L.NOISE_PHILOX if self.chain_noise else L.NOISE_OFF
                ch.seed = seed
        if self.noise_ops:
            if zs is not None:
                assert len(zs) == len(self.z_ops), (len(zs), len(self.z_ops))
                for zi, z in zip(self.z_ops, zs):
                    arr[zi].u.layout.nchw = z.data_ptr()
                mode = L.NOISE_EXPLICIT
            else:
                mode = L.NOISE_PHILOX
            for i in self.noise_ops:
                arr[i].u.conv.noise_mode = mode
                arr[i].u.conv.seed = seed
        if self.streams is not None:
            self.streams.ensure(stream)
        if mode != L.NOISE_EXPLICIT and self.z_ops:
            # explicit-z import ops are recorded first; skip them when z is not supplied
            first = max(self.z_ops) + 1
            L.check(L.lib().esr_run_ops(C.cast(C.byref(arr, first * C.sizeof(L.esr_op)), C.c_void_p),
                                        len(self.ops.ops) - first, C.c_void_p(stream)), 'esr_run_ops')
        else:
            self.ops.run(stream)


def new_buf(bufs, B, C_, H, W, dtype, device, image_limit=False):
    """A zeroed G32 buffer that the list `bufs` (a plan's or a backward pass's) keeps alive."""
    b = G32(B, C_, H, W, dtype, device, image_limit)
    bufs.append(b)
    return b


def layout_op(ops, dt_e, B, g, C_, to_g32, nchw=None, affine=None):
    """NCHW -> G32 (to_g32 = 1) or G32 -> NCHW layout op over channels [0, C_) of the first B images of buffer g,
    appended to `ops`; returns its index.  nchw: the fp32 NCHW side, when it is known at build time.  affine: per-channel
    (mean, 1/std) of an input normalisation folded into the conversion (and into its adjoint on the way back)."""
    lo = L.esr_layout()
    lo.dtype, lo.to_g32 = dt_e, to_g32
    lo.B, lo.C, lo.H, lo.W = B, C_, g.H, g.W
    lo.g32 = g.view(0, C_)
    if nchw is not None:
        lo.nchw = nchw
    if affine is not None:
        lo.use_affine = 1
        for i in range(len(affine[0])):
            lo.mean_c[i] = affine[0][i]
            lo.inv_std_c[i] = affine[1][i]
    return ops.add(L.OP_LAYOUT, 'layout', lo)


def _both(*names):
    return {n: (n, n) for n in names}


class Ends:
    """The two ends of an RRDBNet inference plan: how the caller's pixels get into the first G32 buffer and how HR_conv1's
    result reaches the caller.  Everything between them is the same recorded middle (Builder.rrdbnet, Builder.tail), so an
    inference form is one Ends class, one per kind of op, plus its entry function in functional.py.
    kind, field: the op kind of the two ends and its member of the esr_op union; ptr: the field that takes the caller's
    pointer (set_nchw); per_run: the values bind() writes per run, each with the field it goes to on the input op and
    on the output op (None: not there).
    This base class is the plain pair: the NCHW -> G32 layout import, and HR_conv1 itself — through its NCHW epilogue —
    as the output op."""

    kind, field, ptr = L.OP_LAYOUT, 'layout', 'nchw'
    per_run = {}

    def input_op(self, b, xin, in_nc):
        """Records the op that fills the in_nc channels of buffer xin of Builder b; returns its index."""
        return b.import_nchw(xin, in_nc)

    def output(self, b, hr1, out_nc):
        """Records HR_conv1 (the esr_conv hr1, its output still unset) and what follows it; returns the index of the op
        that writes the caller's tensor."""
        return b.plan.ops.add_conv(hr1)

    def end_ops(self, plan):
        """The structs of the plan's input op and output op, in the array the next run launches."""
        arr = plan.ops.array()
        return getattr(arr[plan.in_op].u, self.field), getattr(arr[plan.out_op].u, self.field)

    def bind(self, plan, **values):
        """Writes the per-run values (names of per_run) into the two end ops of the plan."""
        g, s = self.end_ops(plan)
        for name, v in values.items():
            gf, sf = self.per_run[name]
            if gf is not None:
                setattr(g, gf, v)
            if sf is not None:
                setattr(s, sf, v)


class SlotEnds(Ends):
    """Ends with an op on either side (fill(): the struct of the input op, to_g32 = 1 into buffer g, or of the output op,
    to_g32 = 0).  HR_conv1 leaves its fp32 NCHW result (unrounded in either precision, as the ordinary plan's) in a
    buffer of the plan, slot-major, and the output op moves it from there into the caller's tensor."""

    def input_op(self, b, xin, in_nc):
        return b.plan.ops.add(self.kind, self.field, self.fill(b, in_nc, 1, g=xin))

    def output(self, b, hr1, out_nc):
        P = b.plan
        slots = torch.empty(P.out_shape, dtype=torch.float32, device=b.device)
        b.bufs.append(slots)
        hr1.nchw_out = slots.data_ptr()
        P.ops.add_conv(hr1)
        return P.ops.add(self.kind, self.field, self.fill(b, out_nc, 0, slots=slots))

    def ends_of(self, d, C_, to_g32, g, slots):
        """The fields every such struct has: the direction, the channels, and the G32 buffer or the slots tensor."""
        d.to_g32, d.C = to_g32, C_
        if to_g32:
            d.g32 = g.view(0, C_)
        else:
            d.slots_nchw = slots.data_ptr()
        return d


class DihedralEnds(SlotEnds):
    """Self-ensemble ends (esr_dihedral) of a batch of slots x n images: the import of the transformed copies of n NCHW
    images of H x W, and the reduce that undoes the transforms of the slots x n outputs into n NCHW images of sH x sW.
    The range's first k, accumulate and scale are set per pass (x8_passes)."""

    kind, field = L.OP_DIHEDRAL, 'dihedral'
    per_run = dict(_both('k_begin'), accumulate=(None, 'accumulate'), scale=(None, 'scale'))

    def __init__(self, n, H, W):
        self.n, self.H, self.W = n, H, W

    def fill(self, b, C_, to_g32, g=None, slots=None):
        d = self.ends_of(L.esr_dihedral(), C_, to_g32, g, slots)
        s = 1 if to_g32 else b.scale
        d.dtype, d.B, d.H, d.W = b.dt_e, self.n, s * self.H, s * self.W
        d.k_begin, d.k_count, d.accumulate, d.scale = 0, b.B // self.n, 0, 1.0
        return d

    def output(self, b, hr1, out_nc):
        i = super().output(b, hr1, out_nc)
        b.plan.out_shape = (self.n, out_nc, b.scale * self.H, b.scale * self.W)
        return i


class TileEnds(SlotEnds):
    """Tiled-inference ends (esr_tile) of a batch of windows x n images, the builder's H x W the window: the gather of
    t_count windows of each of n NCHW images, and the stitch that copies every tile's owned rectangle out of the
    t_count x n window outputs into n NCHW images.  Everything image-sized (H, W, tile, pad) and the pass's first tile
    are set per run (bind_image, tile_passes): the ops are recorded for the smallest image that has this window."""

    kind, field, struct = L.OP_TILE, 'tile', L.esr_tile
    per_run = dict(_both('tile', 'pad', 't_begin'), H=('H', None), W=('W', None), HR_H=(None, 'H'), HR_W=(None, 'W'))

    def __init__(self, n):
        self.n = n

    def window(self, b):
        """(th, tw, windows per image) of the batch."""
        return b.H, b.W, b.B // self.n

    def fill(self, b, C_, to_g32, g=None, slots=None):
        d = self.ends_of(self.struct(), C_, to_g32, g, slots)
        th, tw, t_count = self.window(b)
        d.dtype, d.B, d.scale = b.dt_e, self.n, 1 if to_g32 else 4
        d.H, d.W = th * d.scale, tw * d.scale
        d.tile, d.pad, d.t_begin, d.t_count = max(th, tw), 0, 0, t_count
        return d


class TileX8Ends(TileEnds):
    """Tiled self-ensemble ends (esr_tile_x8) of a batch of slots x windows x n images: the gather-import of the
    transforms [k0, k0 + slots) of the th x tw windows (th x tw on the NCHW side: the builder's H x W is tw x th for the
    transposed slots, k0 = 4), and the stitch-reduce that undoes the transforms, sums and copies every tile's owned
    rectangle into the caller's tensor.  TileEnds' per-run values and the pass's k range, accumulate and mean scale."""

    kind, field, struct = L.OP_TILE_X8, 'tile_x8', L.esr_tile_x8
    per_run = dict(TileEnds.per_run, **_both('k_begin'), accumulate=(None, 'accumulate'), scale=(None, 'mean_scale'))

    def __init__(self, n, th, tw, k0, slots):
        self.n, self.th, self.tw, self.k0, self.slots = n, th, tw, k0, slots

    def window(self, b):
        return self.th, self.tw, b.B // (self.slots * self.n)

    def fill(self, b, C_, to_g32, g=None, slots=None):
        d = super().fill(b, C_, to_g32, g, slots)
        d.k_begin, d.k_count, d.accumulate, d.mean_scale = self.k0, self.slots, 0, 1.0
        return d


class TileManyEnds(SlotEnds):
    """Image-set tiled ends (esr_tile_many) of a batch of windows, the builder's H x W each: the gather of every slot's
    window from an image of its own, and the stitch of every slot's owned rectangle into the image its table entry
    names.  The images are named by the pass's slice of the device item table (ptr = items); tile and pad are set per
    run."""

    kind, field, ptr, struct = L.OP_TILE_MANY, 'tile_many', 'items', L.esr_tile_many
    per_run = _both('tile', 'pad')

    def fill(self, b, C_, to_g32, g=None, slots=None):
        d = self.ends_of(self.struct(), C_, to_g32, g, slots)
        d.dtype, d.scale = b.dt_e, 1 if to_g32 else 4
        d.th, d.tw, d.n_slots = b.H, b.W, b.B
        d.tile, d.pad = max(b.H, b.W), 0
        return d


class TileImgEnds(TileManyEnds):
    """TileManyEnds with 8-bit HWC images outside (esr_tile_img: the same fields and bgr, set per run too); the stitch
    quantises the fp32 slots buffer."""

    kind, field, struct = L.OP_TILE_IMG, 'tile_img', L.esr_tile_img
    per_run = _both('tile', 'pad', 'bgr')


class TileHrEnds(TileImgEnds):
    """TileImgEnds whose gather makes the LR window itself, out of the 8-bit HR image through the whole image's bicubic
    tables (esr_tile_hr: the gather's table entries name per-image descriptors); the stitch is esr_tile_img's."""

    kind, field, struct = L.OP_TILE_HR, 'tile_hr', L.esr_tile_hr


class TileSetX8Ends(TileManyEnds):
    """Image-set self-ensemble ends (esr_tile_set_x8) of a batch of slots x P windows: the gather-import of the transforms
    [k0, k0 + slots) of the P upright th x tw windows the pass's table names (the builder's H x W is tw x th for the
    transposed slots, k0 = 4), and the stitch-reduce that undoes the transforms, sums and copies every live window's
    owned rectangle into ITS image's result.  img: 8-bit HWC images outside instead of fp32 NCHW; acc: the fp32 tensor
    [P, C, 4 th, 4 tw] that carries the 8-bit form's partial sums between the passes (the two plans of a non-square
    window share it; None: the float form, or all eight slots in one pass).  tile, pad, bgr and the pass's k range,
    accumulate and mean scale are set per run."""

    kind, field, struct = L.OP_TILE_SET_X8, 'tile_set_x8', L.esr_tile_set_x8
    per_run = dict(_both('tile', 'pad', 'bgr', 'k_begin'), accumulate=(None, 'accumulate'), scale=(None, 'mean_scale'))

    def __init__(self, th, tw, k0, slots, img=False, acc=None):
        self.th, self.tw, self.k0, self.slots, self.img, self.acc = th, tw, k0, slots, img, acc

    def fill(self, b, C_, to_g32, g=None, slots=None):
        d = self.ends_of(self.struct(), C_, to_g32, g, slots)
        d.dtype, d.scale = b.dt_e, 1 if to_g32 else 4
        d.th, d.tw, d.n_windows = self.th, self.tw, b.B // self.slots
        d.tile, d.pad = max(self.th, self.tw), 0
        d.k_begin, d.k_count, d.accumulate, d.mean_scale = self.k0, self.slots, 0, 1.0
        d.img, d.bgr = int(self.img), 0
        if self.acc is not None and not to_g32:
            b.bufs.append(self.acc)
            d.acc = self.acc.data_ptr()
        return d


ENDS_OF_KIND = {e.kind: e for e in (Ends, DihedralEnds, TileEnds, TileX8Ends, TileManyEnds, TileImgEnds, TileSetX8Ends,
                                         TileHrEnds)}


def set_nchw(op, ptr):
    """Bind the caller's tensor to an op that reads or writes one: a conv with an NCHW epilogue, or one of the end ops."""
    if op.kind == L.OP_CONV:
        op.u.conv.nchw_out = ptr
    else:
        e = ENDS_OF_KIND[op.kind]
        setattr(getattr(op.u, e.field), e.ptr, ptr)


class Builder:
    """Emits the fused-conv sequence of RDB / RRDB / RRDBNet into a Plan."""

    image_limit = False           # G32's per-image offset bound (TrainBuilder: the weight-gradient kernels)

    def __init__(self, wp, B, H, W, dtype, device, noise, variant, kind='net', nb=1, scale=4, ends=None):
        self.wp = wp
        self.scale = scale            # upscale of the generator: 1, 2, 4, 8 = 0..3 nearest-x2 up-convs, 3 = one folded x3
        self.B, self.H, self.W = B, H, W
        self.dt_e, self.tdtype, self.cpg = _dt(dtype)
        self.dtype = dtype
        self.device = device
        self.noise = noise            # bool: emit noise epilogues (training mode)
        self.variant = variant        # 'codes' | 'test_image'
        self.kind = kind              # 'net' | 'rrdb' | 'rdb'
        self.nb = nb                  # RRDBs
        self.layers = NoiseLayers(variant, kind, nb, noise)
        self.plan = Plan()
        self.bufs = self.plan.bufs    # everything the ops point at stays alive with the plan
        self.zbufs = []
        self.ends = ends or Ends()    # the two ends of rrdbnet(); B x H x W is the batch between them

    def buf(self, C_, H=None, W=None):
        return new_buf(self.bufs, self.B, C_, H or self.H, W or self.W, self.dtype, self.device, self.image_limit)

    def upload(self, table):
        t = upload_table(table, self.device)
        t.host_table = table          # what the launchers cannot read: chain() checks the views' address limits on it
        self.bufs.append(t)
        return t

    def layout(self, ops, g, C_, to_g32):
        return layout_op(ops, self.dt_e, self.B, g, C_, to_g32)

    def import_nchw(self, dst, C_):
        return self.layout(self.plan.ops, dst, C_, 1)

    def export_nchw(self, src, C_):
        return self.layout(self.plan.ops, src, C_, 0)

    def alloc_z(self, explicit_z):
        """Explicit-z staging: one 64-channel G32 buffer + import op per noise layer."""
        self.zbufs = []
        for _ in range(self.layers.total if explicit_z else 0):
            zb = self.buf(64)
            self.plan.z_ops.append(self.import_nchw(zb, 64))
            self.zbufs.append(zb)

    def set_noise(self, c, slot, lid):
        """Stage `slot` (1 / 2 / 3) of conv c multiplies by (1 + sigma * z[lid]); lid None: no noise there."""
        if lid is None:
            return
        setattr(c, 'layer%d' % slot, lid)
        if self.zbufs:
            setattr(c, 'z%d' % slot, self.zbufs[lid].view(0, 64))

    def rdb(self, prefix, bf, bn, layer1=None, rrdb_x=None, layer2=None, aux=None):
        """ResidualDenseBlock_5C (block.py:260-268) over concat buffer ``bf`` (x in ch 0..63);
        result -> ``bn`` channels 0..63, through noise layer ``layer1``.  ``rrdb_x``: fuse the RRDB tail
        (block.py:291) and its noise layer ``layer2``.  ``aux`` (training): 64-channel buffer that keeps the
        pre-residual activations of conv2 / conv4, whose signs are the LeakyReLU masks of the backward."""
        e = self.wp.entries
        B, H, W, d = self.B, self.H, self.W, self.dt_e
        add = self.plan.ops.add_conv
        # x1 = lrelu(conv1(x))
        add(_conv(d, B, H, W, bf.view(0), 64, bf.view(64, 32), e[prefix + '.conv1.0'], L.ACT_LRELU))
        # x2 = lrelu(conv2([x,x1])) + conv1x1(x)            (block.py:262-263)
        c = _conv(d, B, H, W, bf.view(0), 96, bf.view(96, 32), e[prefix + '.conv2.0'], L.ACT_LRELU)
        c.w1x1 = e[prefix + '.conv1x1'].w_ptr
        c.n1x1_groups = 64 // self.cpg
        if aux is not None:
            c.aux_out = aux.view(0, 32)
        add(c)
        # x3 = lrelu(conv3([x,x1,x2]))
        add(_conv(d, B, H, W, bf.view(0), 128, bf.view(128, 32), e[prefix + '.conv3.0'], L.ACT_LRELU))
        # x4 = lrelu(conv4([x..x3])) + x2                     (block.py:265-266)
        c = _conv(d, B, H, W, bf.view(0), 160, bf.view(160, 32), e[prefix + '.conv4.0'], L.ACT_LRELU)
        c.res1, c.alpha = bf.view(96, 32), 1.0
        if aux is not None:
            c.aux_out = aux.view(32, 32)
        add(c)
        # out = noise(conv5([x..x4]) * 0.2 + x)               (block.py:267-268)
        c = _conv(d, B, H, W, bf.view(0), 192, bn.view(0, 64), e[prefix + '.conv5.0'], L.ACT_NONE)
        c.res1, c.alpha = bf.view(0, 64), 0.2
        self.set_noise(c, 1, layer1)
        if rrdb_x is not None:                                 # RRDB: out*0.2 + x (block.py:291)
            c.res2, c.beta = rrdb_x.view(0, 64), 0.2
            self.set_noise(c, 2, layer2)                       # test_image/block.py:256
        i = add(c)
        if self.noise:
            self.plan.noise_ops.append(i)

    def rrdb(self, prefix, i, x0, x1, x2):
        """RRDB i (block.py:287-291): x0 -> x1 -> x2 -> back into x0 (in place, pixel-local)."""
        ly = self.layers
        self.rdb(prefix + '.RDB1', x0, x1, ly.rdb(i, 0))
        self.rdb(prefix + '.RDB2', x1, x2, ly.rdb(i, 1))
        self.rdb(prefix + '.RDB3', x2, x0, ly.rdb(i, 2), rrdb_x=x0, layer2=ly.rrdb(i))

    def rrdb_chain_specs(self, prefix, i, xa, xb):
        """RRDB i as three rdb_chain specs over two 64-channel slots: RDB1 xa -> xb, RDB2 xb -> xb (in place), RDB3
        xb -> xa with the RRDB tail reading xa."""
        ly = self.layers
        return [(prefix + '.RDB1', xa, xb, None, ly.rdb(i, 0), None), (prefix + '.RDB2', xb, xb, None, ly.rdb(i, 1), None),
                (prefix + '.RDB3', xb, xa, xa, ly.rdb(i, 2), ly.rrdb(i))]

    def chain_workspace(self, B, H, W):
        """The flag / counter workspace of chain launches over B images of H x W (zeroed once; the kernel leaves it
        clean).  Returns (tensor, bytes)."""
        ws_bytes = L.lib().esr_rdb_workspace_bytes(B, H, W)
        ws = torch.zeros((ws_bytes + 3) // 4, dtype=torch.int32, device=self.device)
        self.bufs.append(ws)
        return ws, ws_bytes

    def chain(self, ws, blk_t, k0, k1, dense, geom=None, mode=0, save_dense=0, bands=None):
        """esr_rdb_chain over blocks [k0, k1) of the uploaded esr_rdb_block table blk_t.  geom: (B, H, W) of the launch
        (default: the plan's); mode 0 / 1 / 2 = inference / training forward / backward; bands: (band_rows,
        band_margin, img_H) of the banded form.  noise_mode and seed are set per run."""
        ch = L.esr_rdb_chain()
        ch.dtype = self.dt_e
        ch.B, ch.H, ch.W = geom or (self.B, self.H, self.W)
        ch.mode, ch.save_dense = mode, save_dense
        ch.n_blocks, ch.noise_mode, ch.sigma = k1 - k0, L.NOISE_OFF, SIGMA
        ch.dense = dense
        ch.blocks = blk_t.data_ptr() + k0 * C.sizeof(L.esr_rdb_block)
        ch.workspace, ch.workspace_bytes = ws[0].data_ptr(), ws[1]
        if bands is not None:
            ch.band_rows, ch.band_margin, ch.img_H = bands
        host = getattr(blk_t, 'host_table', None)
        if host is not None:      # the block table is device memory to the launcher: its views are checked here
            L.check(L.lib().esr_rdb_chain_check(ch, C.addressof(host) + k0 * C.sizeof(L.esr_rdb_block)),
                    'esr_rdb_chain_check')
        return ch

    def rdb_chain(self, specs):
        """ONE fused launch for a chain of dense blocks.  specs: list of (prefix, x_in, x_out, res2 or None, layer1,
        layer2) over 64-channel G32 buffers; the 128-channel dense scratch is shared."""
        P = self.plan
        if P.streams is not None:
            raise NotImplementedError('one chain per plan')
        P.streams = RdbStreams(self.wp, [s[0] for s in specs])
        dense = self.buf(128)
        blocks = (L.esr_rdb_block * len(specs))()
        for i, (prefix, xi, xo, r2, layer1, layer2) in enumerate(specs):
            b = blocks[i]
            b.w, b.bias = P.streams.w_ptr(i), P.streams.bias_ptr(i)
            b.x_in, b.x_out = xi.view(0, 64), xo.view(0, 64)
            if r2 is not None:
                b.res2 = r2.view(0, 64)
            b.layer1, b.layer2 = _layer(layer1), _layer(layer2)
            # the output must be complete in memory when it is the chain's result or a later RRDB input
            later_res2 = any(s[3] is xo for s in specs[i + 1:])
            b.flags = L.RDB_FULL_OUT if (i == len(specs) - 1 or later_res2) else 0
        blk_t = self.upload(blocks)
        ws = self.chain_workspace(self.B, self.H, self.W)
        i = P.ops.add(L.OP_RDB_CHAIN, 'rdb_chain', self.chain(ws, blk_t, 0, len(specs), dense.view(0, 128)))
        P.chain_ops.append(i)
        P.chain_noise = self.noise
        P.chain_ws = ws[0]
        return i

    def rdb_chain_banded(self, geom, head):
        """The trunk of an image too large for one chain launch: per RRDB (and per image of the batch) one launch
        over row bands.  RRDB i reads the 64-channel buffer xs[i % 2] and writes xs[(i + 1) % 2] — out of place: a
        band's margin rows are its neighbours' own rows, so nothing a band reads may change during the launch —
        with the two intermediate block outputs and the dense scratch in band-local buffers.  head(view): emits
        the op(s) that fill xs[0]'s image rows.  Returns the view of the result's image rows."""
        P = self.plan
        S, m, nbands = geom
        hb = S + 2 * m
        B, H, W, nb = self.B, self.H, self.W, self.nb
        tall, mid, dense = band_buffers(B, geom, W, self.dtype, self.device)
        self.bufs.extend(tall + [mid, dense])
        prefixes = ['model.1.sub.%d.RDB%d' % (i, j + 1) for i in range(nb) for j in range(3)]
        P.streams = RdbStreams(self.wp, prefixes)
        ws = self.chain_workspace(nbands, hb, W)
        head(tall[0].view(0, 64, m))

        def band(buf, bi):
            v = buf.view(0, 64)
            v.ptr += bi * buf.bs
            v.batch_stride = S * buf.Wp * 32
            return v
        for i in range(nb):
            src, dst = tall[i % 2], tall[(i + 1) % 2]
            for bi in range(B):
                blocks = (L.esr_rdb_block * 3)()
                for j in range(3):
                    b = blocks[j]
                    b.w, b.bias = P.streams.w_ptr(3 * i + j), P.streams.bias_ptr(3 * i + j)
                    b.x_in = band(src, bi) if j == 0 else mid.view(0, 64)
                    b.x_out = band(dst, bi) if j == 2 else mid.view(0, 64)
                    b.layer1 = b.layer2 = L.NO_LAYER
                    b.flags = 0
                blocks[2].res2 = band(src, bi)
                blocks[2].flags = L.RDB_FULL_OUT | L.RDB_BAND_OWN
                ch = self.chain(ws, self.upload(blocks), 0, 3, dense.view(0, 128), geom=(nbands, hb, W), bands=(S, m, H))
                P.chain_ops.append(P.ops.add(L.OP_RDB_CHAIN, 'rdb_chain', ch))
        P.chain_noise = False
        P.chain_ws = ws[0]
        return tall[nb % 2].view(0, 64, m)

    def head(self, xin, in_nc, dst, fea):
        """fea_conv (model.0) into the view dst, with a copy in fea for the trunk shortcut (block.py:84-86)."""
        c = _conv(self.dt_e, self.B, self.H, self.W, xin.view(0), in_nc, dst, self.wp.entries['model.0'])
        c.aux_out = fea.view(0, 64)
        self.plan.ops.add_conv(c)

    def tail_keys(self):
        """Keys of the convs behind the trunk, from the pack (= the module tree): (up-conv keys, HR_conv0, HR_conv1)."""
        idx = sorted(int(k[6:]) for k in self.wp.entries if k.startswith('model.') and k[6:].isdigit() and int(k[6:]) >= 2)
        keys = ['model.%d' % i for i in idx]
        return keys[:-2], keys[-2], keys[-1]

    def shuffle3(self, ops, z, u, H, W, inverse=False):
        """esr_pool mode 4: u[c][3h+i][3w+j] = z[ch(c,i,j)][h][w] over H x W low-resolution pixels (64 channels of u, 576
        of z), or mode 5, its adjoint z <- u."""
        pl = L.esr_pool()
        pl.dtype, pl.mode = self.dt_e, L.POOL_UNSHUFFLE3 if inverse else L.POOL_SHUFFLE3
        pl.B, pl.C, pl.H, pl.W = self.B, 64, H, W
        if inverse:
            pl.x, pl.g, pl.gx = z.view(0, 576), u.view(0, 64), z.view(0, 576)
        else:
            pl.x, pl.y = z.view(0, 576), u.view(0, 64)
        return ops.add(L.OP_POOL, 'pool', pl)

    def tail(self, x, fea, t, out_nc):
        """LR_conv + trunk shortcut from the view x into t (None: a new buffer), the up-convs — n x (nearest x2 + conv +
        lrelu) for x1 / x2 / x4 / x8, or for x3 the folded 64 -> 576 conv + lrelu on the LR grid and a 3x pixel shuffle —
        HR_conv0 + lrelu, HR_conv1 -> NCHW (architecture.py:66-78).  Returns the buffers the backward reads:
        (T, [outputs of the up-convs], U3 = HR_conv0's output)."""
        e = self.wp.entries
        B, H, W, d, s = self.B, self.H, self.W, self.dt_e, self.scale
        P = self.plan
        ups, hr0, hr1 = self.tail_keys()
        t = self.buf(64) if t is None else t
        c = _conv(d, B, H, W, x, 64, t.view(0, 64), e['model.1.sub.%d' % self.nb])
        c.res1, c.alpha = fea.view(0, 64), 1.0
        P.ops.add_conv(c)
        us, src, h, w = [], t, H, W
        if s == 3:
            self.Z3 = self.buf(576)
            h, w = 3 * H, 3 * W
            us.append(self.buf(64, h, w))
            P.ops.add_conv(_conv(d, B, H, W, t.view(0), 64, self.Z3.view(0, 576), e[ups[0] + '#fold'], L.ACT_LRELU))
            self.shuffle3(P.ops, self.Z3, us[0], H, W)
            src = us[0]
        else:
            assert 2 ** len(ups) == s, (ups, s)
            sizes = [(H << (i + 1), W << (i + 1)) for i in range(len(ups))]
            us = [self.buf(64, hh, ww) for hh, ww in sizes]
            for k, u, (h, w) in zip(ups, us, sizes):
                P.ops.add_conv(_conv(d, B, h, w, src.view(0), 64, u.view(0, 64), e[k], L.ACT_LRELU, upsample=1))
                src = u
        u3 = self.buf(64, h, w)
        P.ops.add_conv(_conv(d, B, h, w, src.view(0), 64, u3.view(0, 64), e[hr0], L.ACT_LRELU))
        c = _conv(d, B, h, w, u3.view(0), 64, None, e[hr1])
        c.nchw_out_c = out_nc
        P.out_shape = (B, out_nc, s * H, s * W)
        P.out_op = self.ends.output(self, c, out_nc)
        return t, us, u3

    def rrdbnet(self, in_nc, out_nc, explicit_z):
        """RRDBNet (architecture.py:47-78): fea_conv, nb x RRDB, LR_conv + trunk shortcut, the up-convs of `scale`,
        HR_conv0 + lrelu, HR_conv1."""
        B, H, W, nb = self.B, self.H, self.W, self.nb
        P = self.plan
        self.alloc_z(explicit_z)
        xin = self.buf(in_nc)
        fea = self.buf(64)
        P.ends = self.ends
        P.in_op = self.ends.input_op(self, xin, in_nc)
        if nb and rdb_chain_ok(B, H, W, self.noise, explicit_z):
            # fused trunk: two 64-channel slots + the chain's 128-channel dense scratch
            xa, xb = self.buf(64), self.buf(64)
            self.head(xin, in_nc, xa.view(0, 64), fea)
            self.rdb_chain([s for i in range(nb) for s in self.rrdb_chain_specs('model.1.sub.%d' % i, i, xa, xb)])
            x, t = xa.view(0), xb
        elif nb and not self.noise and use_rdb_bands(self.dt_e, H, W):
            # more tiles than CUs (a DIV2K-sized LR image): the fused trunk in row bands, one launch per RRDB
            x = self.rdb_chain_banded(rdb_band_geometry(H, W), lambda dst: self.head(xin, in_nc, dst, fea))
            t = None
        else:
            x0, x1, x2 = self.buf(192), self.buf(192), self.buf(192)
            self.head(xin, in_nc, x0.view(0, 64), fea)
            for i in range(nb):
                self.rrdb('model.1.sub.%d' % i, i, x0, x1, x2)
            x, t = x0.view(0), x1
        self.tail(x, fea, t, out_nc)
        return P

    def block_plan(self, explicit_z):
        """Stand-alone ResidualDenseBlock_5C ('rdb') or RRDB ('rrdb') pass: NCHW in -> NCHW out."""
        P = self.plan
        self.alloc_z(explicit_z)
        if rdb_chain_ok(self.B, self.H, self.W, self.noise, explicit_z):
            xa, xb = self.buf(64), self.buf(64)
            P.in_op = self.import_nchw(xa, 64)
            if self.kind == 'rdb':
                self.rdb_chain([('rdb', xa, xb, None, self.layers.rdb(0, 0), None)])
            else:
                self.rdb_chain(self.rrdb_chain_specs('rrdb', 0, xa, xb))
            res = xb if self.kind == 'rdb' else xa
        else:
            x0, x1 = self.buf(192), self.buf(192)
            P.in_op = self.import_nchw(x0, 64)
            if self.kind == 'rdb':
                self.rdb('rdb', x0, x1, self.layers.rdb(0, 0))
            else:
                self.rrdb('rrdb', 0, x0, x1, self.buf(192))
            res = x1 if self.kind == 'rdb' else x0
        P.out_op = self.export_nchw(res, 64)
        P.out_shape = (self.B, 64, self.H, self.W)
        return P


def use_graphs():
    """hipGraph replay of the training plans (ESR_GRAPH=1).  Off by default: on ROCm 7.2 a graph launch
    of ~1 000 kernel nodes costs the host about as much as the individual launches (train step 25.6 ms
    with graphs vs 25.2 ms without, profiles/r01_experiments.md), so it buys nothing yet."""
    return os.environ.get('ESR_GRAPH', '0') == '1'


def deterministic_wgrad():
    """Two-stage weight-gradient reduction (esr_wgrad.partial): bit-identical gradients run to run instead of
    fp32 atomics (ESR_WGRAD_DET=0 restores the atomics)."""
    return os.environ.get('ESR_WGRAD_DET', '1') != '0'


def _own_wgrad_regions(oplist, device, pick):
    """A partial region of its own for every OP_WGRAD op of the list that pick(op) selects.  Returns the tensor that
    holds the regions (or None)."""
    arr = oplist.array()
    needs = []
    for i, o in enumerate(oplist.ops):
        if o.kind == L.OP_WGRAD and pick(o):
            n = L.lib().esr_wgrad_workspace_elems(C.cast(C.byref(arr[i]), C.c_void_p), 1)
            needs.append((o, (int(n) + 63) // 64 * 64))
    total = sum(n for _, n in needs)
    if total <= 0:
        return None
    arena = torch.empty(total, dtype=torch.float32, device=device)
    off = 0
    for o, n in needs:
        o.u.wgrad.partial, o.u.wgrad.partial_elems = (arena.data_ptr() + 4 * off, n) if n else (None, 0)
        off += n
    oplist._arr = None
    return arena


def attach_wgrad_arena(oplist, device, exclusive=False):
    """Give every fp16 weight-gradient op of a backward list the partial arena of the deterministic reduction
    (one arena per list: a slot only lives inside one esr_run_ops launch group, and the list's wgrad runs are
    ordered on one stream).  exclusive: every op gets a region of its own (ESR_OPF_SIDE_FREE runs are in flight
    together).  Returns the arena tensor (keep it alive with the plan) or None."""
    if not deterministic_wgrad():
        return None
    wops = [o for o in oplist.ops if o.kind == L.OP_WGRAD]      # fp16 kernels and the fp32 parity kernel alike
    if not wops:
        return None
    if exclusive:
        return _own_wgrad_regions(oplist, device, lambda o: True)
    need = L.lib().esr_wgrad_workspace_elems(C.cast(oplist.array(), C.c_void_p), len(oplist.ops))
    if need <= 0:
        return None
    arena = torch.empty(need, dtype=torch.float32, device=device)
    for o in wops:
        o.u.wgrad.partial, o.u.wgrad.partial_elems = arena.data_ptr(), need
    oplist._arr = None
    return arena


def attach_free_wgrad_regions(oplist, device):
    """ESR_OPF_SIDE_FREE weight-gradient ops of a list whose other wgrad ops share one arena (attach_wgrad_arena): they
    are in flight together, so each gets a partial region of its own.  Returns the tensor that holds them (or None)."""
    if not deterministic_wgrad():
        return None
    return _own_wgrad_regions(oplist, device, lambda o: o.flags & L.OPF_SIDE_FREE)


def current_stream():
    return torch.cuda.current_stream().cuda_stream


_concurrent_cache = {}


def concurrent_streams(device, n):
    """n torch streams on `device` for work next to the current stream: plain new streams, cached per (device, current
    stream).  HIP maps streams onto a few hardware queues (GPU_MAX_HW_QUEUES, default 4) and two streams on one queue
    serialise; measured on MI355X / ROCm 7.2 (tools/stream_probe.py): the FIRST stream a process creates shares its
    queue with the default stream — the train step's "side" stream of round 3, whose D step therefore never
    overlapped the main stream's work."""
    dev = torch.device(device)
    have = _concurrent_cache.setdefault((dev.index, torch.cuda.current_stream(dev).cuda_stream), [])
    while len(have) < n:
        have.append(torch.cuda.Stream(device=dev))
    return have[:n]


class StreamOrder:
    """A module's launch plans own their activation buffers, packed weights and chain workspaces, so two inference
    calls of ONE module from two streams must not overlap (torch modules are stateless in that respect; a second
    stream is how users overlap independent work).  ``with StreamOrder.of(mod).call():`` makes the calling stream wait —
    on the device — for the module's previous call when that ran on another stream, and marks the end of this call on
    the way out, also when the call raises: part of its launches may be queued by then.  Skipped under graph capture
    (the graph's order applies)."""

    def __init__(self):
        self.last = None
        self.event = None

    @staticmethod
    def of(mod):
        so = mod.__dict__.get('_stream_order')
        if so is None:
            so = mod.__dict__['_stream_order'] = StreamOrder()
        return so

    @contextlib.contextmanager
    def call(self):
        cur = torch.cuda.current_stream()
        if not torch.cuda.is_current_stream_capturing() and self.last is not None and self.last != cur.cuda_stream:
            cur.wait_event(self.event)
        try:
            yield cur
        finally:
            if not torch.cuda.is_current_stream_capturing():
                if self.event is None:
                    self.event = torch.cuda.Event()
                self.event.record(cur)
                self.last = cur.cuda_stream


def env_int(name, default, lo, hi):
    """An integer schedule knob from the environment, validated: a misspelt or out-of-range value is an error that
    names the knob and its range, not an opaque ValueError in the middle of a plan build or a silently ignored
    setting."""
    v = os.environ.get(name)
    if v is None or v == '':
        return default
    try:
        n = int(v)
    except ValueError:
        raise ValueError('%s=%r: expected an integer in [%d, %d]' % (name, v, lo, hi)) from None
    if not lo <= n <= hi:
        raise ValueError('%s=%d: expected an integer in [%d, %d]' % (name, n, lo, hi))
    return n


def spare_cus(B, H, W):
    """CUs that a backward-chain launch over 4-row tiles leaves free."""
    return L.lib().esr_rdb_max_tiles_per_image() - B * ((H + 3) // 4) * ((W + 31) // 32)


def bwd_chain_split(B, H, W, nb):
    """Launches the fused backward chain of a training plan is cut into (runs of whole RRDBs; 1 = one launch).  More
    than one only when the chain's grid leaves at least half of the CUs idle (4-row tiles, at most cus / 2 of them):
    the weight gradients of a run then execute under the next run's chain.  ESR_BWD_SPLIT = n forces n (1: off)."""
    env = env_int('ESR_BWD_SPLIT', None, 1, max(1, nb))
    if env is not None:
        return env
    half_idle = 2 * spare_cus(B, H, W) >= L.lib().esr_rdb_max_tiles_per_image()
    return min(2, nb) if half_idle else 1      # (train step, same box: 1 run 7.09 ms, 2 runs 7.01, 4 runs 7.06)


def bwd_follow():
    """Training crops: the backward chain's weight gradients as a follower pass next to ONE chain launch (ESR_OPF_FOLLOW)
    instead of the two-launch form of bwd_chain_split.  ESR_BWD_FOLLOW=0: the round-5 form (A/B)."""
    if os.environ.get('ESR_BWD_SPLIT'):            # an explicit split asks for the multi-launch form
        return False
    return os.environ.get('ESR_BWD_FOLLOW', '1') != '0'


def use_rdb_wgrad():
    """fp16 training plans: the six weight gradients of a dense block as ONE esr_rdb_wgrad pass over its saved
    concat buffer and gradient concat (csrc/rdb_wgrad.hip) instead of six esr_conv_wgrad problems
    (ESR_RDB_WGRAD=0 restores those, for A/B runs)."""
    return os.environ.get('ESR_RDB_WGRAD', '1') != '0'


def build_block_plan(kind, wp, B, H, W, dtype, device, noise, variant, explicit_z):
    """Stand-alone ResidualDenseBlock_5C ('rdb') or RRDB ('rrdb') pass: NCHW in -> NCHW out."""
    return Builder(wp, B, H, W, dtype, device, noise, variant, kind).block_plan(explicit_z)


def build_rrdbnet_plan(wp, nb, in_nc, out_nc, B, H, W, dtype, device, noise, variant, explicit_z, scale=4, ends=None):
    """The plan of RRDBNet over a batch of B x H x W between `ends` (default: the plain NCHW pair).  Every other form
    below is this plan in eval mode, at the batch its ends make of the caller's images: the ops between the two ends
    are those of the ordinary plan of that batch shape."""
    b = Builder(wp, B, H, W, dtype, device, noise, variant, 'net', nb, scale=scale, ends=ends)
    return b.rrdbnet(in_nc, out_nc, explicit_z)


X8_SLOTS = (8, 4, 2, 1)


def x8_slots(H, W, slots_per_pass=None):
    """Slots (transformed copies per image) one pass of the self-ensemble runs as a batch: the argument, else
    ESR_X8_SLOTS, else 8 for square input and 4 otherwise — a pass cannot mix H x W and W x H slots."""
    n = env_int('ESR_X8_SLOTS', 8, 1, 8) if slots_per_pass is None else int(slots_per_pass)
    if n not in X8_SLOTS:
        raise ValueError('slots per pass of the x8 self-ensemble must be one of %s, got %r' % (X8_SLOTS, n))
    return min(n, 4) if H != W else n


def x8_passes(slots):
    """The 8 / slots passes of a self-ensemble, [(first k, index of the plan, accumulate, scale)]: the first plan runs
    k 0..3 and the last one k 4..7 (the transposed shape where there are two), the passes are chained through the
    output op's accumulate from the second on, and the last applies the 1/8."""
    return [(k0, -1 if k0 >= 4 else 0, int(k0 > 0), 0.125 if k0 + slots == 8 else 1.0) for k0 in range(0, 8, slots)]


def tile_passes(n_tiles, P):
    """First tiles of the passes of P tiles over an image of n_tiles.  A tail pass is as large as the others: the gather
    repeats the last tile, the stitch skips it."""
    return range(0, n_tiles, P)


def bind_image(plans, x, tile, pad, P):
    """What a tiled run of the images x sets once per call on the two ends of its plans — H, W on the gather, 4H, 4W on
    the stitch, tile and pad on both — -> its tile_passes."""
    H, W = x.shape[2], x.shape[3]
    for plan in plans:
        plan.bind(H=H, W=W, HR_H=4 * H, HR_W=4 * W, tile=tile, pad=pad)
    return tile_passes(-(-H // tile) * -(-W // tile), P)


class X8Plan:
    """The x8 self-ensemble of one (batch, shape, precision): x8_passes over one inference plan of batch slots x B (two
    plans for non-square input: H x W for k 0..3, W x H for k 4..7) between DihedralEnds."""

    def __init__(self, plans, slots, out_shape):
        self.plans, self.slots, self.out_shape = plans, slots, out_shape

    def run(self, x, out, stream):
        for k0, i, accumulate, scale in x8_passes(self.slots):
            self.plans[i].bind(k_begin=k0, accumulate=accumulate, scale=scale)
            self.plans[i].run(x, out, stream)


def build_rrdbnet_x8_plan(wp, nb, in_nc, out_nc, B, H, W, dtype, device, variant, slots, scale=4):
    plans = [build_rrdbnet_plan(wp, nb, in_nc, out_nc, slots * B, sh, sw, dtype, device, False, variant, False, scale,
                                DihedralEnds(B, H, W)) for sh, sw in ([(H, W)] if H == W else [(H, W), (W, H)])]
    return X8Plan(plans, slots, (B, out_nc, scale * H, scale * W))


def tiled_geometry(H, W, tile, pad):
    """Tiling of an H x W image (LR pixels; include/esrgan_hip.h: esr_tile) -> (th, tw, ny, nx, tiles): the window
    shape, the tile grid and, row-major, per tile (y0, y1, x0, x1, wy, wx): the owned rows [y0, y1) and columns
    [x0, x1) and the top-left corner of its th x tw window."""
    th, tw = min(tile + 2 * pad, H), min(tile + 2 * pad, W)
    ny, nx = -(-H // tile), -(-W // tile)
    tiles = []
    for i in range(ny):
        for j in range(nx):
            tiles.append((i * tile, min((i + 1) * tile, H), j * tile, min((j + 1) * tile, W),
                          min(max(i * tile - pad, 0), H - th), min(max(j * tile - pad, 0), W - tw)))
    return th, tw, ny, nx, tiles


class TiledPlan:
    """The tiled forward of every image whose windows are th x tw, in passes of P windows per image: one inference plan
    of batch P x B at th x tw between TileEnds.  Nothing in it depends on the image size."""

    def __init__(self, plan, P):
        self.plan, self.P = plan, P

    def run(self, x, out, tile, pad, stream):
        for t0 in bind_image([self.plan], x, tile, pad, self.P):
            self.plan.bind(t_begin=t0)
            self.plan.run(x, out, stream)


def build_rrdbnet_tiled_plan(wp, nb, in_nc, out_nc, B, th, tw, dtype, device, variant, P):
    return TiledPlan(build_rrdbnet_plan(wp, nb, in_nc, out_nc, P * B, th, tw, dtype, device, False, variant, False,
                                        ends=TileEnds(B)), P)


class TiledManyPlan:
    """The tiled forward of S windows of th x tw per pass, whichever images they belong to: one inference plan of batch S
    at th x tw between TileManyEnds — or TileImgEnds, the same plan with 8-bit images outside and one more bound value,
    bgr.  Nothing in it depends on an image or a channel order."""

    def __init__(self, plan, S):
        self.plan, self.S = plan, S

    def bind(self, **bound):
        """tile and pad (and bgr) of the passes that follow."""
        self.plan.bind(**bound)

    def run(self, gather_items, stitch_items, stream):
        """One pass: the two uint8 device tensors hold the pass's S item entries (esr_tile_item / esr_tile_img_item: LR
        images / HR results)."""
        self.plan.run(gather_items, stitch_items, stream)


def build_rrdbnet_tiled_many_plan(wp, nb, in_nc, out_nc, S, th, tw, dtype, device, variant, ends=TileManyEnds):
    return TiledManyPlan(build_rrdbnet_plan(wp, nb, in_nc, out_nc, S, th, tw, dtype, device, False, variant, False,
                                            ends=ends()), S)


class TiledX8Plan:
    """The tiled x8 self-ensemble of every image whose windows are th x tw: per pass of P windows per image, the
    x8_passes of one inference plan of batch slots x P x B (two plans for non-square windows: th x tw for k 0..3, tw x th
    for k 4..7) between TileX8Ends, chained into the caller's tensor.  Nothing in it depends on the image size."""

    def __init__(self, plans, slots, P):
        self.plans, self.slots, self.P = plans, slots, P

    def run(self, x, out, tile, pad, stream):
        for t0 in bind_image(self.plans, x, tile, pad, self.P):
            for k0, i, accumulate, scale in x8_passes(self.slots):
                self.plans[i].bind(t_begin=t0, k_begin=k0, accumulate=accumulate, scale=scale)
                self.plans[i].run(x, out, stream)


def build_rrdbnet_tiled_x8_plan(wp, nb, in_nc, out_nc, B, th, tw, dtype, device, variant, P, slots):
    plans = [build_rrdbnet_plan(wp, nb, in_nc, out_nc, slots * P * B, sh, sw, dtype, device, False, variant, False,
                                ends=TileX8Ends(B, th, tw, k0, slots))
             for k0, sh, sw in ([(0, th, tw)] if th == tw else [(0, th, tw), (4, tw, th)])]
    return TiledX8Plan(plans, slots, P)


class TiledSetX8Plan:
    """The x8 self-ensemble of P windows of th x tw per pass, whichever images they belong to: the x8_passes of one
    inference plan of batch slots x P (two plans for non-square windows: th x tw for k 0..3, tw x th for k 4..7) between
    TileSetX8Ends, chained through the results themselves (fp32 ends) or through `acc` (8-bit ends).  Nothing in it
    depends on an image or a channel order."""

    def __init__(self, plans, slots, P, acc):
        self.plans, self.slots, self.P, self.acc = plans, slots, P, acc

    def bind(self, **bound):
        """tile and pad (and bgr) of the passes that follow."""
        for plan in self.plans:
            plan.bind(**bound)

    def run(self, gather_items, stitch_items, stream):
        """One pass of P windows: the two uint8 device tensors hold its P item entries (LR images / HR results)."""
        for k0, i, accumulate, scale in x8_passes(self.slots):
            self.plans[i].bind(k_begin=k0, accumulate=accumulate, scale=scale)
            self.plans[i].run(gather_items, stitch_items, stream)


def build_rrdbnet_tiled_set_x8_plan(wp, nb, in_nc, out_nc, P, th, tw, dtype, device, variant, slots, img=False):
    acc = (torch.empty((P, out_nc, 4 * th, 4 * tw), dtype=torch.float32, device=device) if img and slots < 8 else None)
    plans = [build_rrdbnet_plan(wp, nb, in_nc, out_nc, slots * P, sh, sw, dtype, device, False, variant, False,
                                ends=TileSetX8Ends(th, tw, k0, slots, img, acc))
             for k0, sh, sw in ([(0, th, tw)] if th == tw else [(0, th, tw), (4, tw, th)])]
    return TiledSetX8Plan(plans, slots, P, acc)


# =================================================================================================
# Training path: forward that keeps every activation + the matching backward launch list
# =================================================================================================
class TapMajorGrads:
    """fp16 wgrad accumulates 3x3 weight gradients tap-major ([tap][cout][cin]: atomics of one wave
    instruction land in 2 cache lines instead of ~36); one esr_grad_unpermute launch at the end of the
    backward pass rewrites all of them into the OIHW slots of the flat gradient buffer."""

    def __init__(self, grad_flat):
        self.flat = grad_flat
        self.tm = torch.zeros_like(grad_flat)
        self.rows = []
        self.total = 0

    def slot(self, off_elems, cout, cin, ntap=9):
        self.rows.append((off_elems, off_elems, self.total, cout, cin, ntap))
        self.total += cout * cin * ntap
        return self.tm.data_ptr() + 4 * off_elems

    def op(self, lo=None, hi=None):
        """The unpermute of every slot (default) or of the slots inside flat elements [lo, hi) — the segmented
        backward rewrites each finished span before its all-reduce starts."""
        rows = [r for r in self.rows if lo is None or lo <= r[0] < hi]
        if not rows:
            return None
        arr = (L.esr_unperm_entry * len(rows))()
        begin = pairs = 0
        for i, r in enumerate(rows):
            arr[i].src_off, arr[i].dst_off, arr[i].elem_begin = r[0], r[1], begin
            arr[i].cout, arr[i].cin, arr[i].ntap, arr[i].pair_begin = r[3], r[4], r[5], pairs
            begin += r[3] * r[4] * r[5]
            pairs += r[3] * r[4]
        table = upload_table(arr, self.flat.device)
        self.tables = getattr(self, 'tables', []) + [table]
        up = L.esr_unpermute()
        up.table, up.n, up.total = table.data_ptr(), len(rows), begin
        up.n_pairs = pairs if pairs < 2 ** 31 else 0
        up.src, up.dst = self.tm.data_ptr(), self.flat.data_ptr()
        return up


class TrainPlan:
    """Forward (all activations kept) + backward launch lists of RRDBNet for one input shape."""

    def __init__(self):
        self.fwd = Plan()
        self.bwd = L.OpList()
        self.bufs = []
        self.packs = None            # (WeightPack, DgradPack) the lists point into: kept alive with the plan (functional._train_plan)
        self.busy = False
        self.gy_op = None            # layout op importing dL/dy (NCHW fp32) in the backward list
        self.bwd_noise_ops = []      # backward conv ops that need (noise_mode, seed)
        self.grad_flat = None        # fp32 flat gradient buffer; views per parameter
        self.grad_views = None
        self.tapmajor = None
        self.gx_op = None            # op exporting dL/dx (NCHW fp32): a layout op (stand-alone blocks) or fea_conv's dgrad
        self.gx_shape = None         # shape of dL/dx
        self.gx_begin = None         # whole generator: ops [gx_begin, end) produce dL/dx and run only when it is wanted
        self.segments = None         # segmented backward: [(op_end, elem_lo, elem_hi)] — after ops [.., op_end) the
                                     # gradients in flat[elem_lo:elem_hi] are final (see TrainBuilder.close_segment)
        self.follow_op = None        # index of the ESR_OPF_FOLLOW weight-gradient op of the backward list (follow_spare: the CUs its
        self.follow_spare = 0        # chain leaves free; follow_wgs: the plan's default grid)
        self.follow_wgs = 0
        self.bwd_chain_ops = []      # indices of OP_RDB_CHAIN_BWD ops in the backward list (noise mode / seed per run)
        self.bwd_chain_ws = None     # their workspace
        self.bwd_streams = None      # RdbBwdStreams feeding them
        self.wgrad_arena = None      # partial sums of the deterministic weight-gradient reduction (attach_wgrad_arena)
        self.wgrad_free_arena = None   # the same for the free-running runs (attach_free_wgrad_regions)
        self.scratch_grads = []      # fp32 gradient buffers outside grad_flat that the backward adds into: zeroed with it
        self.graph = False           # hipGraph replay with I/O bound to the static tensors below
        self.x_static = self.out_static = self.gy_static = self.gx_static = self.seed_t = None

    def enable_graph(self, in_shape, device):
        """Bind every per-step pointer / scalar of both launch lists to fixed device buffers so the
        lists can be captured once and replayed as hipGraphs (the train step is host-launch-bound):
        input / output / upstream-gradient tensors become static staging buffers, the Philox seed is
        read from `seed_t` on the device."""
        P = self.fwd
        assert not P.z_ops, 'graph replay is for the fused-Philox path (explicit z tensors re-bind pointers)'
        f32 = dict(dtype=torch.float32, device=device)
        self.x_static = torch.empty(in_shape, **f32)
        self.out_static = torch.empty(P.out_shape, **f32)
        self.gy_static = torch.empty(P.out_shape, **f32)
        self.gx_static = torch.empty(in_shape, **f32) if self.gx_op is not None else None
        self.seed_t = torch.zeros(1, dtype=torch.int64, device=device)
        chain_mode = L.NOISE_PHILOX if P.chain_noise else L.NOISE_OFF
        arr, barr = P.ops.array(), self.bwd.array()
        arr[P.in_op].u.layout.nchw = self.x_static.data_ptr()
        set_nchw(arr[P.out_op], self.out_static.data_ptr())
        barr[self.gy_op].u.layout.nchw = self.gy_static.data_ptr()
        if self.gx_op is not None:
            set_nchw(barr[self.gx_op], self.gx_static.data_ptr())
        for a, noise_ops, chain_ops in ((arr, P.noise_ops, P.chain_ops), (barr, self.bwd_noise_ops, self.bwd_chain_ops)):
            for i in noise_ops:
                a[i].u.conv.noise_mode = L.NOISE_PHILOX
                a[i].u.conv.seed_dev = self.seed_t.data_ptr()
            for i in chain_ops:
                a[i].u.rdb_chain.noise_mode = chain_mode
                a[i].u.rdb_chain.seed_dev = self.seed_t.data_ptr()
        P.graph_bound = True         # Plan.run keeps its hands off the chain ops from here on
        self.graph = True


# Where the input gradient of a dense block goes (TrainBuilder.block_exit).  dst: the buffer whose channels [0, 64) take
# what runs on — the g_t of the block below it, dL/dx of a stand-alone block, or dL/dfea — through noise layer dst_layer;
# skip_in: the RRDB's skip gradient, added when the block is RDB1; skip_out: the sum becomes the skip gradient of the
# RRDB below it, through noise layer skip_layer — dst then takes 0.2 x that sum (the scaled third output of a conv).
BlockExit = collections.namedtuple('BlockExit', 'dst dst_layer skip_in skip_out skip_layer', defaults=(None,) * 4)


class TrainBuilder(Builder):
    """Emits the training forward of RRDBNet — every RDB concat buffer kept, + the pre-residual activations of conv2 /
    conv4 or the chain's LeakyReLU masks — and the matching backward list into a TrainPlan.  One method per step;
    build_rrdbnet_train_plan calls them in order."""

    image_limit = True

    def __init__(self, wp, dp, nb, B, H, W, dtype, device, noise, variant, explicit_z, kind, segmented, scale=4):
        self.block = kind != 'net'                  # stand-alone RRDB / dense block: no head / tail, dL/dx returned
        super().__init__(wp, B, H, W, dtype, device, noise, variant, kind, 1 if self.block else nb, scale=scale)
        self.tp = TrainPlan()
        self.plan, self.bwd, self.bufs = self.tp.fwd, self.tp.bwd, self.tp.bufs
        self.dp = dp
        self.nj = 1 if kind == 'rdb' else 3         # dense blocks per RRDB
        self.explicit_z = explicit_z
        self.segmented = bool(segmented) and not self.block
        self.chained = self.nb > 0 and use_train_chain(self.dt_e, B, H, W, explicit_z)
        self.fused_wgrad = self.dt_e == L.ESR_F16 and use_rdb_wgrad() and self.nb > 0

    def pkey(self, i, j):
        if self.kind == 'rdb':
            return 'rdb'
        return ('rrdb.RDB%d' % (j + 1)) if self.kind == 'rrdb' else 'model.1.sub.%d.RDB%d' % (i, j + 1)

    def x_out(self, i, j):
        """The buffer whose channels [0, 64) take the output of dense block (i, j): the next block's concat buffer, or
        XF behind the last one.  (-1, nj - 1): what feeds the first block."""
        if j < self.nj - 1:
            return self.S[i][j + 1]
        return self.S[i + 1][0] if i + 1 < self.nb else self.XF

    def rrdb_x(self, i, j):
        """The RRDB input that block (i, j) adds to its output when it closes an RRDB (block.py:291), else None."""
        return self.S[i][0] if j == 2 and self.kind != 'rdb' else None

    # ------------------------------------------------------------------ forward
    def forward_head(self, in_nc):
        P, nb, nj = self.plan, self.nb, self.nj
        self.alloc_z(self.explicit_z)
        self.S = [[self.buf(192) for _ in range(nj)] for _ in range(nb)]
        self.AUX = [[self.buf(64) for _ in range(nj)] for _ in range(nb)] if not self.chained else None
        self.XF = self.buf(64)                              # output of the last RRDB
        if self.block:
            P.in_op = self.import_nchw(self.S[0][0], 64)    # x straight into the concat buffer's first slice
        else:
            self.xin, self.fea = self.buf(in_nc), self.buf(64)
            P.in_op = self.import_nchw(self.xin, in_nc)
            self.head(self.xin, in_nc, self.x_out(-1, nj - 1).view(0, 64), self.fea)

    def forward_blocks_chain(self):
        """ONE esr_rdb_forward launch (mode 1) over all dense blocks; every block keeps its concat buffer S[i][j] =
        [x | x1..x4], its output (the next block's x) and its LeakyReLU masks."""
        P, ly = self.plan, self.layers
        order = [(i, j) for i in range(self.nb) for j in range(self.nj)]
        P.streams = RdbStreams(self.wp, [self.pkey(i, j) for i, j in order])
        mbytes = int(L.lib().esr_rdb_mask_bytes(self.B, self.H, self.W))
        self.masks = {ij: torch.empty(mbytes, dtype=torch.uint8, device=self.device) for ij in order}
        self.bufs.append(self.masks)
        blocks = (L.esr_rdb_block * len(order))()
        for n, (i, j) in enumerate(order):
            bf, b = self.S[i][j], blocks[n]
            b.w, b.bias = P.streams.w_ptr(n), P.streams.bias_ptr(n)
            b.x_in, b.x_out, b.dense = bf.view(0, 64), self.x_out(i, j).view(0, 64), bf.view(64, 128)
            b.mask = self.masks[(i, j)].data_ptr()
            b.layer1, b.layer2 = _layer(ly.rdb(i, j)), L.NO_LAYER
            if self.rrdb_x(i, j) is not None:
                b.res2, b.layer2 = self.rrdb_x(i, j).view(0, 64), _layer(ly.rrdb(i))
            b.flags = L.RDB_FULL_OUT
        blk_t, ws = self.upload(blocks), self.chain_workspace(self.B, self.H, self.W)
        # (dense: the geometry of every view; blocks carry their own)
        ch = self.chain(ws, blk_t, 0, len(order), self.S[0][0].view(64, 128), mode=1)
        P.chain_ops.append(P.ops.add(L.OP_RDB_CHAIN, 'rdb_chain', ch))
        P.chain_noise = bool(self.noise)
        P.chain_ws = ws[0]

    def forward_blocks_convs(self):
        ly = self.layers
        for i in range(self.nb):
            for j in range(self.nj):
                self.rdb(self.pkey(i, j), self.S[i][j], self.x_out(i, j), ly.rdb(i, j), rrdb_x=self.rrdb_x(i, j),
                         layer2=ly.rrdb(i), aux=self.AUX[i][j])

    def forward_exit(self, out_nc):
        if self.block:
            self.plan.out_op = self.export_nchw(self.XF, 64)
            self.plan.out_shape = (self.B, 64, self.H, self.W)
        else:
            self.T, self.Us, self.U3 = self.tail(self.XF.view(0), self.fea, None, out_nc)

    # ------------------------------------------------------------------ gradient storage
    def grad_store(self, net):
        """The flat fp32 gradient buffer with one view per parameter, in net._conv_list() order, and the tap-major
        staging of the fp16 weight gradients."""
        tp = self.tp
        self.plist = list(net._conv_list())
        total = sum(w.numel() + (b_.numel() if b_ is not None else 0) for _, w, b_ in self.plist)
        tp.grad_flat = torch.zeros(total, dtype=torch.float32, device=self.device)
        tp.tapmajor = TapMajorGrads(tp.grad_flat) if self.dt_e == L.ESR_F16 else None
        tp.grad_views, self.gptr, self.goff, self.gend, off = [], {}, {}, {}, 0
        for k, w, b_ in self.plist:
            gw = tp.grad_flat[off:off + w.numel()].view_as(w)
            self.goff[k] = off
            off += w.numel()
            gb = None
            if b_ is not None:
                gb = tp.grad_flat[off:off + b_.numel()].view_as(b_)
                off += b_.numel()
            self.gend[k] = off
            tp.grad_views.append((gw, gb))
            self.gptr[k] = (gw.data_ptr(), gb.data_ptr() if gb is not None else None)
        self.segs = []

    def close_segment(self, prefixes):
        """Segmented backward (data-parallel runs start a slice's all-reduce under the rest of the backward): everything
        the ops so far produce for the parameters whose key starts with one of `prefixes` is final: rewrite the
        tap-major pieces of that span, record the boundary."""
        if not self.segmented:
            return
        goff, gend = self.goff, self.gend
        ks_ = [k for k, _, _ in self.plist if any(k == p_ or k.startswith(p_ + '.') for p_ in prefixes)]
        lo, hi = min(goff[k] for k in ks_), max(gend[k] for k in ks_)
        assert hi - lo == sum(gend[k] - goff[k] for k in ks_), 'segment parameters must tile one span'
        self.unpermute(lo, hi)
        self.segs.append((len(self.bwd.ops), lo, hi))

    def unpermute(self, lo=None, hi=None):
        up = self.tp.tapmajor.op(lo, hi) if self.tp.tapmajor is not None else None
        if up is not None:
            self.bwd.add(L.OP_UNPERMUTE, 'unpermute', up)

    # ------------------------------------------------------------------ backward: pieces
    def dconv(self, Ho, Wo, src, src_ch, dst, key, **kw):
        c = _conv(self.dt_e, self.B, Ho, Wo, src, src_ch, dst, self.dp.entries[key], L.ACT_NONE, **kw)
        c.bias = None
        return c

    def add_b(self, c, noisy=False):
        k = self.bwd.add_conv(c)
        if noisy and self.noise:
            self.tp.bwd_noise_ops.append(k)
        return k

    def wgrad(self, key, g, gin, Hh, Ww, cout, cin, ks=3, ups=0, scale=1.0, dst=None):
        """The esr_wgrad of conv `key`: gradient view g, saved input view gin.  dst: (dw, dbias) pointers of an OIHW
        gradient outside the flat store (the folded x3 up-conv's: backward_tail)."""
        tm = self.tp.tapmajor
        wg = L.esr_wgrad()
        wg.dtype, wg.ks, wg.stride, wg.upsample = self.dt_e, ks, 1, ups
        wg.B, wg.H, wg.W = self.B, Hh, Ww
        wg.cout, wg.cin = cout, cin
        wg.g, wg.in_ = g, gin
        wg.dw, wg.dbias = self.gptr[key] if dst is None else dst
        if tm is not None and ks == 3 and dst is None:
            wg.dw, wg.tap_major = tm.slot(self.goff[key], cout, cin), 1
        wg.scale = scale
        return wg

    def free_wgrad(self, *a, **kw):
        """Weight gradient of a head / tail conv.  Their gradient and input buffers are written once per backward pass
        and their slots of the gradient buffer are read only behind the list's unpermute, so these launches run next
        to the main chain WITHOUT ordering among themselves (ESR_OPF_SIDE_FREE: up to three in flight, each with its
        own partial region — attach_free_wgrad_regions).  Round 5: as ordered side runs the main stream waited for
        run k - 1 before forking run k — at training crops a 70 us weight gradient per 25 us dgrad conv, i.e. the
        tail's backward took 0.4 ms of the step's critical path instead of 0.15."""
        self.bwd.add(L.OP_WGRAD, 'wgrad', self.wgrad(*a, **kw), flags=(_SIDE | _SIDE_FREE) if _SIDE else 0)

    def rdb_wgrad_block(self, i, j, Q):
        """The six weight gradients of dense block (i, j) from its saved concat buffer and its gradient concat Q."""
        p = self.pkey(i, j)
        wb = L.esr_rdb_wgrad_block()
        wb.in_, wb.q = self.S[i][j].view(0, 192), Q.view(0, 224)
        for k in range(5):
            key = p + '.conv%d.0' % (k + 1)
            wb.dw[k] = self.tp.tapmajor.slot(self.goff[key], 64 if k == 4 else 32, 64 + 32 * k)
            wb.db[k] = self.gptr[key][1]
        wb.dw[5] = self.gptr[p + '.conv1x1'][0]
        return wb

    def rdb_wgrad_arena(self, *n_blocks):
        """Per-task partial sums of the deterministic two-stage reduction of esr_rdb_wgrad passes over n_blocks blocks
        (several counts: one arena that fits each; the need is not monotonic in the block count: fewer blocks -> fewer
        images per task -> more slots)."""
        need = max(int(L.lib().esr_rdb_wgrad_workspace_elems(self.B, self.H, self.W, n)) for n in n_blocks)
        arena = torch.empty(need, dtype=torch.float32, device=self.device)
        self.bufs.append(arena)
        return arena

    def add_rdb_wgrad(self, grp, arena, flags=0, max_wg=0):
        """ONE esr_rdb_wgrad pass over the esr_rdb_wgrad_blocks of grp."""
        rw = L.esr_rdb_wgrad()
        rw.dtype, rw.B, rw.H, rw.W = self.dt_e, self.B, self.H, self.W
        rw.n_blocks, rw.tap_major, rw.scale5, rw.scale = len(grp), 1, 0.2, 1.0
        table = (L.esr_rdb_wgrad_block * len(grp))(*grp)
        rw.blocks = self.upload(table).data_ptr()
        rw.partial, rw.partial_elems = arena.data_ptr(), arena.numel()
        rw.max_workgroups = max_wg
        # the block table is device memory to the launcher: its address limits are checked here, on the host copy
        L.check(L.lib().esr_rdb_wgrad_check(rw, C.addressof(table)), 'esr_rdb_wgrad_check')
        return self.bwd.add(L.OP_RDB_WGRAD, 'rdb_wgrad', rw, flags=flags)

    def bwd_index(self, i, j):
        """Position of dense block (i, j) in backward order."""
        return (self.nb - 1 - i) * self.nj + (self.nj - 1 - j)

    def Q(self, n):
        """The gradient concat of the n-th block in backward order (the fused backward keeps one per block, the
        per-conv backward rotates: backward_buffers)."""
        return self.Qs[n % len(self.Qs)]

    def block_exit(self, i, j):
        """Where the input gradient of dense block (i, j) goes.  The RRDB skip gradient A(i) ping-pongs through gA,
        starting with gA[0] for the last RRDB."""
        ly, below = self.layers, self.Q(self.bwd_index(i, j) + 1)
        if j > 0:                       # g_x = g_y of RDB j - 1 -> its g_t = g_y * n
            return BlockExit(below, ly.rdb(i, j - 1))
        if self.kind == 'rdb':
            return BlockExit(self.GX)
        skip_in = self.gA[(self.nb - 1 - i) % 2]
        if self.block:
            return BlockExit(self.GX, skip_in=skip_in)
        if i > 0:                       # through the tail of RRDB i - 1: A(i - 1) = g [n3'], g_t3 = 0.2 A n2
            return BlockExit(below, ly.rdb(i - 1, 2), skip_in, self.gA[(self.nb - i) % 2], ly.rrdb(i - 1))
        return BlockExit(self.GF, skip_in=skip_in)

    def exit_to_block(self, x, b):
        """BlockExit -> esr_rdb_block of the fused backward (its kernel scales x_out when there is an out_a)."""
        b.x_out, b.layer1 = x.dst.view(0, 64), _layer(x.dst_layer)
        b.layer2 = _layer(x.skip_layer)
        if x.skip_in is not None:
            b.res2 = x.skip_in.view(0, 64)
        if x.skip_out is not None:
            b.out_a = x.skip_out.view(0, 64)

    def exit_to_conv(self, x, c):
        """BlockExit -> the slice-x conv that closes a block of the per-conv backward."""
        if x.skip_in is not None:
            c.res2, c.beta = x.skip_in.view(0, 64), 1.0
        if x.skip_out is None:
            c.out = x.dst.view(0, 64)
            self.set_noise(c, 2, x.dst_layer)
        else:
            c.out = x.skip_out.view(0, 64)
            self.set_noise(c, 2, x.skip_layer)
            c.out3, c.gamma = x.dst.view(0, 64), 0.2
            self.set_noise(c, 3, x.dst_layer)

    # ------------------------------------------------------------------ backward: steps
    def backward_buffers(self, out_nc):
        H, W = self.H, self.W
        if self.block:
            self.GY = self.buf(64)
            self.tp.gy_op = self.layout(self.bwd, self.GY, 64, 1)
        else:
            s_ = self.scale
            self.GY = self.buf(out_nc, s_ * H, s_ * W)
            self.tp.gy_op = self.layout(self.bwd, self.GY, out_nc, 1)
            # masked gradients at the outputs of HR_conv0 (x4: "GA8") and of every up-conv (x4: GA3, GA6)
            self.GA_hr = self.buf(64, s_ * H, s_ * W)
            self.GAs = [self.buf(64, u.H, u.W) for u in self.Us]
            if s_ == 3:
                # x3: the gradient of the folded conv's 576 outputs (the unshuffled GAs[0]) and, fp32 OIHW, the folded
                # weight / bias gradient that esr_fold3 (mode 1) sums into the up-conv's slots of the flat store
                self.G3 = self.buf(576)
                self.DW3 = torch.zeros(576 * 64 * 9 + 576, dtype=torch.float32, device=self.device)
                self.tp.scratch_grads.append(self.DW3)
            self.GTt = self.buf(64)                     # dL/dT (trunk output)
        # The six weight gradients of a block run on the side stream, concurrently with the NEXT block's
        # dgrad chain (both are latency-bound, ~64-workgroup launches at training sizes), and are joined
        # before the block after that starts: what they read (g_t, GA, G[96:128]) rotates so that the
        # chain running next to them writes other buffers — g_t through 3, G/GA through 2.
        # Gather-form dgrad (block._rdb_gathers): per block one 224-channel gradient concat
        #   Q = [g_t (64) | g_a4 | g_a3 | g_a2 | g_a1 | g_x2 raw]   (32 each)
        # that the slice convs read as a growing prefix and each fills one slice of — the dense
        # connectivity mirrored, no read-modify-write of an accumulator.  Q rotates through 3 buffers: the
        # block's weight gradients read it on the side stream while the next block runs, and the block
        # after that is the first to overwrite it (its predecessor already writes ITS g_t into slot 0).
        # The side runs are forked once per RRDB (its three blocks' 18 weight gradients in one run: every fork costs the
        # main stream an event record + wait, ~11 us of idle chip at LR sizes) and joined at the next fork, so a block's
        # Q has to survive two groups: 2 * nj + 1 buffers.
        # Fused backward: every block keeps its Q for the weight gradients.
        nj = self.nj
        self.gA = [self.buf(64), self.buf(64)]          # RRDB skip gradient A(i), ping-pong
        self.Qs = [self.buf(224) for _ in range(2 * nj + 1 if not self.chained else self.nb * nj)]
        self.X4 = self.buf(32) if not self.chained else None     # raw g_x4 (identity path x4 = lrelu(a4) + x2)
        self.GF = self.buf(64)                          # dL/dfea

    def backward_entry_block(self):
        """Entry of a stand-alone block: the incoming gradient through the block's own tail.
          rdb : y = (0.2 x5 + x) n            -> g_t = g_y n
          rrdb: y = ((t3 n2) 0.2 + x) [n3']   -> skip gradient A = g_y [n3'],  g_t3 = 0.2 A n2
        = a 1x1 identity "conv" (key '__eye') whose epilogue applies the noise / scale stages."""
        ly = self.layers
        c = self.dconv(self.H, self.W, self.GY.view(0), 64, None, '__eye')
        if self.kind == 'rdb':
            self.exit_to_conv(BlockExit(self.Q(0), ly.rdb(0, 0)), c)
        else:
            self.exit_to_conv(BlockExit(self.Q(0), ly.rdb(0, 2), None, self.gA[0], ly.rrdb(0)), c)
        self.add_b(c, noisy=True)

    def backward_tail(self, out_nc):
        """HR_conv1 .. LR_conv backwards: dL/dy -> the skip gradient and g_t of the last RRDB (nb = 0: dL/dfea)."""
        H, W, nb, ly = self.H, self.W, self.nb, self.layers
        dconv, add_b, wgrad = self.dconv, self.add_b, self.free_wgrad
        s_ = self.scale
        ups, hr0, hr1 = self.tail_keys()
        ins = [self.T] + self.Us                      # input of up-conv i (and, last, of HR_conv0)
        GY, GA_hr, GAs, GTt, U3 = self.GY, self.GA_hr, self.GAs, self.GTt, self.U3
        # HR_conv1: u3 -> y
        wgrad(hr1, GY.view(0, out_nc), U3.view(0, 64), s_ * H, s_ * W, out_nc, 64)
        c = dconv(s_ * H, s_ * W, GY.view(0), out_nc, None, hr1)
        c.mask, c.out2, c.mask_cb_begin = U3.view(0, 64), GA_hr.view(0, 64), 0
        add_b(c)
        # HR_conv0: last up-conv's output (lrelu; x1: T, no activation) -> u3 (lrelu)
        wgrad(hr0, GA_hr.view(0, 64), ins[-1].view(0, 64), s_ * H, s_ * W, 64, 64)
        if self.Us:
            c = dconv(s_ * H, s_ * W, GA_hr.view(0), 64, None, hr0)
            c.mask, c.out2 = self.Us[-1].view(0, 64), GAs[-1].view(0, 64)
            add_b(c)
        else:
            add_b(dconv(H, W, GA_hr.view(0), 64, GTt.view(0, 64), hr0))
        if s_ == 3:
            # folded up-conv: T -> Z3 (576, lrelu) -> shuffle3 -> us[0].  GAs[0] is already masked at 3H x 3W (lrelu
            # commutes with the shuffle), so: its adjoint shuffle, the plain 576 <- 64 weight gradient into DW3, its
            # unfold into the up-conv's own gradient slots, and the plain 576 -> 64 input-gradient conv
            self.shuffle3(self.bwd, self.G3, GAs[0], H, W, inverse=True)
            dw3 = (self.DW3.data_ptr(), self.DW3.data_ptr() + 4 * 576 * 64 * 9)
            self.bwd.add(L.OP_WGRAD, 'wgrad', self.wgrad(ups[0], self.G3.view(0, 576), self.T.view(0, 64), H, W, 576, 64, dst=dw3))
            f = L.esr_fold3()
            f.mode, f.cout, f.cin = L.FOLD3_UNFOLD, 64, 64
            f.wf, f.bf = dw3
            f.w, f.bias = self.gptr[ups[0]]
            self.bwd.add(L.OP_FOLD3, 'fold3', f)
            add_b(dconv(H, W, self.G3.view(0), 576, GTt.view(0, 64), ups[0] + '#fold'))
        for i in range(len(ups) - 1, -1, -1):
            if s_ == 3:
                break
            # up-conv i: up(ins[i]) -> us[i] ; adjoint = 4x4/s2 conv
            u = self.Us[i]
            wgrad(ups[i], GAs[i].view(0, 64), ins[i].view(0, 64), u.H, u.W, 64, 64, ups=1)
            if i > 0:
                c = dconv(u.H // 2, u.W // 2, GAs[i].view(0), 64, None, ups[i], ks=4, stride=2)
                c.mask, c.out2 = ins[i].view(0, 64), GAs[i - 1].view(0, 64)
                add_b(c)
            else:
                add_b(dconv(H, W, GAs[0].view(0), 64, GTt.view(0, 64), ups[0], ks=4, stride=2))
        # LR_conv (model.1.sub.nb): XF -> T - fea
        lrk = 'model.1.sub.%d' % nb
        wgrad(lrk, GTt.view(0, 64), self.XF.view(0, 64), H, W, 64, 64)
        c = dconv(H, W, GTt.view(0), 64, None, lrk)
        if nb:
            self.exit_to_conv(BlockExit(self.Q(0), ly.rdb(nb - 1, 2), None, self.gA[0], ly.rrdb(nb - 1)), c)
        else:
            c.out = self.GF.view(0, 64)
            c.res1 = GTt.view(0, 64)                    # fea feeds both the trunk and the shortcut
        add_b(c, noisy=bool(nb))
        self.close_segment([lrk] + ups + [hr0, hr1])

    def backward_blocks(self):
        if self.fused_wgrad and not self.chained:
            # per-RRDB passes of the per-conv backward: one arena, reused by every pass (the passes are ordered on the
            # side stream; a slot only lives inside one pass)
            self.rdbw_arena = self.rdb_wgrad_arena(self.nj)
        self.GX = self.buf(64) if self.block else None      # dL/dx of a stand-alone block
        if self.chained:
            self.backward_blocks_chain()
        else:
            self.backward_blocks_convs()

    def backward_blocks_chain(self):
        """Fused backward: esr_rdb_backward over the dense blocks in backward order (block n reads its g_t from
        Qs[n][0:64], leaves g_a4..g_a1 and the raw g_x2 in Qs[n][64:224], and writes the next block's g_t), and the
        weight gradients of all blocks in esr_rdb_wgrad passes over (S, Q), in one of three schedules."""
        tp, nb, nj = self.tp, self.nb, self.nj
        border = [(i, j) for i in range(nb - 1, -1, -1) for j in range(nj - 1, -1, -1)]
        tp.bwd_streams = RdbBwdStreams(self.dp, [self.pkey(i, j) for i, j in border])
        blocks = (L.esr_rdb_block * len(border))()
        wblocks = []
        for n, (i, j) in enumerate(border):
            Q, b = self.Q(n), blocks[n]
            b.w = tp.bwd_streams.w_ptr(n)
            b.x_in, b.dense, b.aux = Q.view(0, 64), Q.view(64, 128), Q.view(192, 32)
            b.mask = self.masks[(i, j)].data_ptr()
            b.flags = L.RDB_FULL_OUT
            self.exit_to_block(self.block_exit(i, j), b)
            wblocks.append(self.rdb_wgrad_block(i, j, Q))
        self.bwd_blk_t = self.upload(blocks)
        self.bwd_ws = self.chain_workspace(self.B, self.H, self.W)
        tp.bwd_chain_ws = self.bwd_ws[0]
        nsplit = 1 if self.segmented else bwd_chain_split(self.B, self.H, self.W, nb)
        spare = spare_cus(self.B, self.H, self.W)
        if nsplit > 1 and _SIDE and bwd_follow() and spare >= 32:
            self.chain_with_follower(wblocks, spare)
        elif nsplit > 1:
            self.chain_in_runs(wblocks, nsplit, max(32, spare))
        else:
            self.chain_then_wgrads(wblocks)

    def add_bwd_chain(self, k0, k1):
        """Blocks [k0, k1) (backward order) of the fused backward as one launch."""
        ch = self.chain(self.bwd_ws, self.bwd_blk_t, k0, k1, self.Q(k0).view(64, 128), mode=2, save_dense=1)
        self.tp.bwd_chain_ops.append(self.bwd.add(L.OP_RDB_CHAIN_BWD, 'rdb_chain', ch))

    def chain_with_follower(self, wblocks, spare):
        """Round 6: ONE chain launch and, launched with it on the side stream, the weight gradients of ALL blocks as a
        follower pass on the CUs the chain leaves free — a block's tasks start when the chain has published the block
        (csrc/rdb_wgrad.hip: follow_wait), its partial sums are reduced in slices by the tasks of the block a round of
        the grid later (delayed-slice reduction, rdb_wgrad_follow_kernel).  Behind the chain only the last block's
        tasks are left (the two-launch form, chain_in_runs, left the second run's pass + reduction: 0.4 + 0.08 ms of
        the step's critical path)."""
        tp = self.tp
        arena = self.rdb_wgrad_arena(len(wblocks))
        self.add_bwd_chain(0, len(wblocks))
        # (the follower's workgroups each hold a whole CU's LDS for the length of the chain: what else runs next to
        # the G backward — the D step on the caller's second stream — needs CUs too.  Train step, same box, two runs
        # each: round-5 form 6.52 ms; follower on 40 / 48 / 56 / 64 / 72 / 80 / 88 / 96 / 128 workgroups 7.33 / 6.86 /
        # 6.52 / 6.28 / 6.29 / 6.26 / 6.27 / 6.23* / 6.57* (* another box: 6.42 without).  ESR_BWD_FOLLOW_WGS: A/B knob)
        wgs = env_int('ESR_BWD_FOLLOW_WGS', min(spare, 80), 32, max(32, spare))
        # (functional._train_backward: a caller may size the follower per run — the train step's logging form)
        tp.follow_op = self.add_rdb_wgrad(wblocks, arena, flags=_SIDE | L.OPF_FOLLOW, max_wg=wgs)
        tp.follow_spare, tp.follow_wgs = spare, wgs

    def chain_in_runs(self, wblocks, nsplit, spare):
        """Small grids (the reference's training crops: 16 x 32^2 LR = 128 four-row tiles on 256 CUs): the chain leaves
        half of the chip idle and the weight gradients — 0.7 ms behind a 1.9 ms chain — sit on the step's critical
        path.  The chain runs as `nsplit` launches over runs of whole RRDBs, and the weight gradients of a run go to
        the SIDE stream right behind its chain launch: they execute on the idle CUs under the next run's chain (block n
        reads its g_t from Qs[n], which the previous launch's last block wrote: launch boundaries are free of
        semantics).  Only the last run's weight gradients are left behind the chain."""
        nb, nj = self.nb, self.nj
        per_run = (nb + nsplit - 1) // nsplit
        # run boundaries (RRDB indices).  ESR_BWD_SPLIT_FIRST = n: two runs, the first of n RRDBs (A/B: the LAST run's
        # weight gradients are the ones left behind the chain, the first run's must fit under the second chain)
        first = env_int('ESR_BWD_SPLIT_FIRST', 0, 0, nb)          # 0 / nb: equal runs
        bounds = list(range(0, nb, per_run)) + [nb]
        if nsplit == 2 and 0 < first < nb:
            bounds = [0, first, nb]
        runs = list(zip(bounds[:-1], bounds[1:]))
        arena = self.rdb_wgrad_arena(*[(r1 - r0) * nj for r0, r1 in runs])
        for r0, r1 in runs:
            k0, k1 = r0 * nj, r1 * nj
            self.add_bwd_chain(k0, k1)
            # every run but the last shares the chip with the next run's chain: its pass keeps to the spare CUs
            # (a persistent grid of that many workgroups) so that the chain's workgroups find theirs free
            self.add_rdb_wgrad(wblocks[k0:k1], arena, flags=_SIDE, max_wg=spare if k1 < len(wblocks) else 0)

    def chain_then_wgrads(self, wblocks):
        """One chain launch, then the weight gradients: one pass over all blocks — or, data-parallel, one per RRDB so
        that each RRDB's slice of the flat gradient buffer goes to its all-reduce while the next pass runs."""
        nj = self.nj
        self.add_bwd_chain(0, len(wblocks))
        groups = [wblocks] if not self.segmented else [wblocks[k:k + nj] for k in range(0, len(wblocks), nj)]
        arena = self.rdb_wgrad_arena(max(len(g_) for g_ in groups))
        for gi, grp in enumerate(groups):
            self.add_rdb_wgrad(grp, arena)
            if self.segmented:
                self.close_segment(['model.1.sub.%d' % (self.nb - 1 - gi)])

    def backward_blocks_convs(self):
        """Per-conv backward of the dense blocks: five gather-form slice convs per block over its Q, the weight
        gradients of an RRDB as one side run behind its last dgrad conv."""
        H, W, dconv, add_b = self.H, self.W, self.dconv, self.add_b
        X4 = self.X4
        for i in range(self.nb - 1, -1, -1):
            # a block's six weight gradients read Q and the saved input, intact until the group after next
            # starts -> emitted together with the rest of the RRDB's after its last dgrad chain (one side run)
            deferred = []
            for j in range(self.nj - 1, -1, -1):
                bf, ax, p = self.S[i][j], self.AUX[i][j], self.pkey(i, j)
                Q = self.Q(self.bwd_index(i, j))            # Q[0:64] already holds this block's g_t
                if self.fused_wgrad:
                    # one esr_rdb_wgrad pass per RRDB over (saved concat buffer, Q) of its blocks (rdb_wgrad.hip)
                    deferred.append(self.rdb_wgrad_block(i, j, Q))
                else:
                    deferred += [self.wgrad(p + '.conv5.0', Q.view(0, 64), bf.view(0, 192), H, W, 64, 192, scale=0.2),
                                 self.wgrad(p + '.conv4.0', Q.view(64, 32), bf.view(0, 160), H, W, 32, 160),
                                 self.wgrad(p + '.conv3.0', Q.view(96, 32), bf.view(0, 128), H, W, 32, 128),
                                 self.wgrad(p + '.conv2.0', Q.view(128, 32), bf.view(0, 96), H, W, 32, 96),
                                 self.wgrad(p + '.conv1x1', Q.view(192, 32), bf.view(0, 64), H, W, 32, 64, ks=1),
                                 self.wgrad(p + '.conv1.0', Q.view(160, 32), bf.view(0, 64), H, W, 32, 64)]
                # slice x4: g_x4 = conv5^T[x4](0.2 g_t)  -> raw to X4, masked (lrelu'(a4)) to Q[64:96]
                c = dconv(H, W, Q.view(0), 64, X4.view(0, 32), p + '.g4')
                c.mask, c.out2, c.mask_cb_begin = ax.view(32, 32), Q.view(64, 32), 0
                add_b(c)
                # slice x3 -> g_a3 = masked into Q[96:128]
                c = dconv(H, W, Q.view(0), 96, None, p + '.g3')
                c.mask, c.out2, c.mask_cb_begin = bf.view(128, 32), Q.view(96, 32), 0
                add_b(c)
                # slice x2 (+ g_x4: x4 = lrelu(a4) + x2) -> raw to Q[192:224] (feeds the 1x1), masked to Q[128:160]
                c = dconv(H, W, Q.view(0), 128, Q.view(192, 32), p + '.g2')
                c.res1 = X4.view(0, 32)
                c.mask, c.out2, c.mask_cb_begin = ax.view(0, 32), Q.view(128, 32), 0
                add_b(c)
                # slice x1 -> g_a1 = masked into Q[160:192]
                c = dconv(H, W, Q.view(0), 160, None, p + '.g1')
                c.mask, c.out2, c.mask_cb_begin = bf.view(64, 32), Q.view(160, 32), 0
                add_b(c)
                # slice x closes the block: g_x = sum_k conv_k^T[x](g_ak) + conv1x1^T(g_x2) + g_t
                # (d(0.2 x5 + x)/dx)  (+ RRDB skip for RDB1)
                c = dconv(H, W, Q.view(0), 224, None, p + '.g0')
                c.res1 = Q.view(0, 64)
                self.exit_to_conv(self.block_exit(i, j), c)
                add_b(c, noisy=True)
            if self.fused_wgrad:
                self.add_rdb_wgrad(deferred, self.rdbw_arena, flags=_SIDE)
            else:
                for wg in deferred:
                    self.bwd.add(L.OP_WGRAD, 'wgrad', wg, flags=_SIDE)
            if not self.block:
                self.close_segment(['model.1.sub.%d' % i])

    def backward_exit(self, in_nc):
        """dL/dfea -> fea_conv's weight gradient, the unpermute of the tap-major gradients, and dL/dx."""
        tp, H, W = self.tp, self.H, self.W
        GF = self.GF
        if not self.block:
            if self.nb:
                # trunk shortcut (fea feeds T directly as well): dL/dfea = chain result + dL/dT
                GF = self.buf(64)
                c = self.dconv(H, W, self.GF.view(0), 64, GF.view(0, 64), '__eye')
                c.res1 = self.GTt.view(0, 64)
                self.add_b(c)
            # fea_conv (model.0): weight gradient only (the LR input image needs no gradient)
            self.free_wgrad('model.0', GF.view(0, 64), self.xin.view(0, in_nc), H, W, 64, in_nc)
            self.close_segment(['model.0'])
        if self.segmented:
            segs = self.segs
            assert sorted((lo, hi) for _, lo, hi in segs)[0][0] == 0 and sum(hi - lo for _, lo, hi in segs) == tp.grad_flat.numel()
            tp.segments = segs
        else:
            self.unpermute()
        if self.block:
            tp.gx_op, tp.gx_shape = self.layout(self.bwd, self.GX, 64, 0), (self.B, 64, H, W)
        else:
            # dL/dx of the whole generator (autograd through architecture.py:76-78 when the LR input requires a gradient):
            # fea_conv's input gradient, written straight into the caller's NCHW tensor.  Recorded at the END of the list
            # and only run on request (TrainPlan.gx_begin: functional._train_backward stops there otherwise).
            tp.gx_begin = len(self.bwd.ops)
            c = self.dconv(H, W, GF.view(0), 64, None, 'model.0')
            c.nchw_out_c = in_nc
            tp.gx_op, tp.gx_shape = self.add_b(c), (self.B, in_nc, H, W)
        tp.wgrad_arena = attach_wgrad_arena(self.bwd, self.device)
        tp.wgrad_free_arena = attach_free_wgrad_regions(self.bwd, self.device)


def build_rrdbnet_train_plan(net, wp, dp, nb, in_nc, out_nc, B, H, W, dtype, device, noise, variant,
                             explicit_z, kind='net', segmented=False, scale=4):
    """RRDBNet forward keeping every RDB concat buffer (+ pre-residual activations of conv2/conv4,
    whose signs are the LeakyReLU masks) and the backward pass:
      * input gradients = the same fused conv kernel over transposed/rotated weights, with the
        LeakyReLU-mask / noise / residual-scale backward applied in its epilogue;
      * weight/bias gradients = esr_conv_wgrad.
    kind 'net' = the whole generator; 'rrdb' / 'rdb' = a stand-alone RRDB / ResidualDenseBlock_5C
    (64-channel NCHW in and out, gradient w.r.t. the input returned): same block code, no head/tail.
    segmented ('net' only): the backward list records, per RRDB (and for the tail / the first conv), the op
    index after which that slice of the flat gradient buffer is final — data-parallel runs start its
    all-reduce there, under the rest of the backward (TrainPlan.segments, functional._train_backward)."""
    bld = TrainBuilder(wp, dp, nb, B, H, W, dtype, device, noise, variant, explicit_z, kind, segmented, scale)
    bld.forward_head(in_nc)
    if bld.chained:
        bld.forward_blocks_chain()
    else:
        bld.forward_blocks_convs()
    bld.forward_exit(out_nc)
    bld.grad_store(net)
    bld.backward_buffers(out_nc)
    if bld.block:
        bld.backward_entry_block()
    else:
        bld.backward_tail(out_nc)
    bld.backward_blocks()
    bld.backward_exit(in_nc)
    return bld.tp
