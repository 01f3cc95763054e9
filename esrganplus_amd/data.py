"""Data path on the GPU: what ``LRHRDataset.__getitem__`` does per sample on a CPU
worker (codes/data/LRHR_dataset.py:80-112, codes/data/util.py:94-106,213-343) done per BATCH on the
device, so eight GPUs are not fed by eight Python processes looping over image rows.

* ``imresize`` — MATLAB-compatible bicubic resize with antialiasing (util.py:276-343 /
  ``imresize_np`` 345-412): output size ceil(in*scale), cubic kernel of width 4 (4/scale when
  shrinking), weights normalised per output sample, symmetric border, H pass then W pass, float32.
  The tiny weight / index tables are derived on the host in float64 from the definition of the resize
  (``resample_tables``) and pinned to the reference's outputs by fixtures (<= 2e-6); the two gather passes are
  HIP launches (``esr_resample_axis``).
* ``paired_random_crop`` / ``augment`` — the crop + flip/rot logic on NCHW device tensors, one window / one
  set of coin flips per sample.  ``crop_and_augment`` draws from Python's ``random`` in the reference's
  per-item order (randint, randint, then the three coin flips, sample by sample: LRHR_dataset.py:96-110);
  the two separate helpers draw all windows first, then all flips.
* ``TrainSet`` — the dataset itself on the device: a pool of decoded images of any sizes (uint8 as decoded), and per
  batch ONE launch (``esr_batch_assemble``) that cuts the windows, flips, converts and, without LR images, resamples the
  LR window from the HR image.  ``batch_reference`` restates it in torch on the CPU for the tests."""
import ctypes as C
import math
import random

import torch

from . import _lib as L
from . import engine as E


def _keys_kernel(t):
    """Keys' piecewise-cubic interpolation kernel with a = -1/2 (what MATLAB's bicubic `imresize` and the
    reference's `cubic`, util.py:213-218, evaluate): support [-2, 2], C1, reproduces quadratics.
    Horner form on |t|, float64."""
    import numpy as np
    a = np.abs(np.asarray(t, dtype=np.float64))
    near = (1.5 * a - 2.5) * a * a + 1.0                     # |t| <= 1
    far = ((-0.5 * a + 2.5) * a - 4.0) * a + 2.0             # 1 < |t| <= 2
    return np.where(a <= 1.0, near, np.where(a <= 2.0, far, 0.0))


def resample_tables(in_length, scale, antialiasing=True):
    """Weights and SOURCE indices of one axis of the MATLAB-style resize (the function util.py:221-343
    computes; derived here from its definition, in float64, not from the reference's float32 tensor code):

      * output sample o (0-based) sits at input coordinate  c(o) = (o + 0.5) / scale - 0.5   (pixel centres
        of the two grids coincide at the image borders);
      * the footprint is Keys' kernel stretched by s = 1/scale when shrinking with antialiasing (a low-pass of
        width 4/scale), unstretched otherwise:  w(o, i) = k((c(o) - i) / s) / s, then normalised per o;
      * taps run over the integer positions within half a footprint of c(o); positions outside the image are
        mirrored about the border pixel EDGES (period 2 n: -1 -> 0, n -> n - 1);
      * columns that are zero for every output sample are dropped, so the table is [out, P] with P the
        widest real support.
    -> (weights [out, P] float32, src [out, P] int32, out_len)"""
    import numpy as np
    n = int(in_length)
    out_length = math.ceil(n * scale)
    stretch = 1.0 / scale if (scale < 1 and antialiasing) else 1.0
    half = 2.0 * stretch                                          # half width of the footprint
    o = np.arange(out_length, dtype=np.float64)
    centre = (o + 0.5) / scale - 0.5
    first = np.floor(centre - half).astype(np.int64) + 1          # first integer position that can fall inside
    ntap = int(math.ceil(2.0 * half)) + 1
    pos = first[:, None] + np.arange(ntap, dtype=np.int64)[None, :]
    w = _keys_kernel((centre[:, None] - pos) / stretch) / stretch
    w /= w.sum(axis=1, keepdims=True)
    live = np.nonzero(np.any(w != 0.0, axis=0))[0]                # trim all-zero columns at either end
    pos, w = pos[:, live[0]:live[-1] + 1], w[:, live[0]:live[-1] + 1]
    m = np.mod(pos, 2 * n)                                        # mirror: period 2n
    src = np.where(m < n, m, 2 * n - 1 - m)
    assert src.min() >= 0 and src.max() < n
    return (torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32)),
            torch.from_numpy(np.ascontiguousarray(src, dtype=np.int32)), out_length)


def _axis_pass(x, axis, w, idx, out_len, stream):
    n, c, h, wd = x.shape
    out = torch.empty((n, c, out_len, wd) if axis == 0 else (n, c, h, out_len), dtype=torch.float32, device=x.device)
    a = L.esr_resample()
    a.in_, a.out = x.data_ptr(), out.data_ptr()
    a.planes, a.in_h, a.in_w, a.out_len, a.axis, a.taps = n * c, h, wd, out_len, axis, w.shape[1]
    a.w, a.idx = w.data_ptr(), idx.data_ptr()
    L.check(L.lib().esr_resample_axis(C.byref(a), C.c_void_p(stream)), 'esr_resample_axis')
    return out


_TABLES = {}


def device_tables(length, scale, dev, antialiasing=True):
    """``resample_tables(length, scale)`` on the device ``dev``, cached per (length, scale): (weights, indices, out_len).
    The cache is bounded; whoever hands the tables' addresses to a kernel keeps the tuple referenced until that work is
    queued."""
    key = (int(length), float(scale), bool(antialiasing), str(dev))
    t = _TABLES.get(key)
    if t is None:
        w, idx, ol = resample_tables(length, scale, antialiasing)
        t = (w.to(dev), idx.to(dev), ol)
        if len(_TABLES) >= 64:            # (length, scale) pairs of a dataset are few; stay bounded anyway
            _TABLES.clear()
        _TABLES[key] = t
    return t


def table_resample(x, scale):
    """``imresize(x, 1 / scale)`` of a [3, H, W] float32 tensor restated with torch on x's device: the tables of
    ``resample_tables`` evaluated as sums over the taps, H pass then W pass (``batch_reference``'s generated LR)."""
    wh, ih, _ = resample_tables(x.shape[1], 1.0 / scale)
    ww, iw, _ = resample_tables(x.shape[2], 1.0 / scale)
    wh, ih, ww, iw = wh.to(x.device), ih.to(x.device), ww.to(x.device), iw.to(x.device)
    y = (x[:, ih.long(), :] * wh[None, :, :, None]).sum(2)
    return (y[:, :, iw.long()] * ww[None, None, :, :]).sum(3)


def table_resample_fused(x, scale):
    """``table_resample`` with the kernels' arithmetic, so that the bits are theirs (``imresize`` on the device,
    ``esr_batch_assemble``'s generated LR, esr_tile_hr's gather): per pass the taps in ascending order from acc = 0,
    ``acc = fma(w[o][t], x[idx[o][t]], acc)`` — one rounding per tap.  The fused multiply-add is formed in float64, where
    the product of two float32 values is exact; the sum is then rounded to float64 and to float32, which differs from
    the one rounding of the hardware only where the float64 sum lands on a float32 tie, a 29-bit coincidence."""
    def axis_pass(x, w, idx, dim):
        acc = None
        shape = [1, -1, 1] if dim == 1 else [1, 1, -1]
        for t in range(w.shape[1]):
            term = w[:, t].double().reshape(shape) * x.index_select(dim, idx[:, t].long()).double()
            acc = (term if acc is None else term + acc.double()).float()
        return acc

    wh, ih, _ = resample_tables(x.shape[1], 1.0 / scale)
    ww, iw, _ = resample_tables(x.shape[2], 1.0 / scale)
    y = axis_pass(x.float(), wh.to(x.device), ih.to(x.device), 1)
    return axis_pass(y, ww.to(x.device), iw.to(x.device), 2)


def imresize(img, scale, antialiasing=True):
    """img: [C,H,W] or [N,C,H,W] float32 on the MI355X, range [0,1], not rounded (util.py:276-343)."""
    E.require_cuda(img, 'image')
    squeeze = img.dim() == 3
    x = (img.unsqueeze(0) if squeeze else img).contiguous().float()
    n, c, h, wd = x.shape
    dev, st = x.device, E.current_stream()
    tabs = [device_tables(length, scale, dev, antialiasing) for length in (h, wd)]
    y = _axis_pass(x, 0, tabs[0][0], tabs[0][1], tabs[0][2], st)
    y = _axis_pass(y, 1, tabs[1][0], tabs[1][1], tabs[1][2], st)
    return y[0] if squeeze else y


def paired_random_crop(lr, hr, lr_size, scale):
    """LRHR_dataset.py:96-103 on NCHW batches.  The reference's ``__getitem__`` draws one window PER SAMPLE
    (two ``random.randint`` calls each, in sample order); a batch does the same — B independent windows.  The
    stream of Python's ``random`` is consumed as B consecutive crops would consume it; use ``crop_and_augment``
    for the reference's interleaved crop / flip order.  A 3-D tensor is one sample."""
    single = lr.dim() == 3
    if single:
        lr, hr = lr[None], hr[None]
    h, w = lr.shape[-2:]
    hs = lr_size * scale
    outl, outh = [], []
    for b in range(lr.shape[0]):
        rnd_h = random.randint(0, max(0, h - lr_size))
        rnd_w = random.randint(0, max(0, w - lr_size))
        rh, rw = int(rnd_h * scale), int(rnd_w * scale)
        outl.append(lr[b, :, rnd_h:rnd_h + lr_size, rnd_w:rnd_w + lr_size])
        outh.append(hr[b, :, rh:rh + hs, rw:rw + hs])
    if single:
        return outl[0], outh[0]
    return torch.stack(outl), torch.stack(outh)


def augment(img_list, hflip=True, rot=True):
    """util.py:94-106: horizontal flip, vertical flip, transpose.  For NCHW batches the three coin flips are
    drawn per SAMPLE, applied to the same sample of every tensor in ``img_list`` (``crop_and_augment`` keeps the
    reference's crop-then-flip draw order per item);
    [C,H,W] tensors are one sample.  Batches need square images when ``rot`` is on (a transposed sample must
    stack with an un-transposed one), which the reference's fixed-size crops guarantee."""
    if img_list[0].dim() == 3:
        return [t[0] for t in augment([t[None] for t in img_list], hflip, rot)]
    B = img_list[0].shape[0]
    flags = []
    for _ in range(B):
        hf = hflip and random.random() < 0.5
        vf = rot and random.random() < 0.5
        r9 = rot and random.random() < 0.5
        flags.append((hf, vf, r9))

    def _aug(t, f):
        if f[0]:
            t = t.flip(-1)
        if f[1]:
            t = t.flip(-2)
        if f[2]:
            t = t.transpose(-1, -2)
        return t
    return [torch.stack([_aug(t[b], flags[b]) for b in range(B)]) for t in img_list]


def crop_and_augment(lr, hr, lr_size, scale, hflip=True, rot=True):
    """One training batch exactly as B consecutive ``LRHRDataset.__getitem__`` calls would cut it
    (LRHR_dataset.py:96-110): per sample, in order, the crop window (``randint`` for the row, ``randint`` for the
    column) and then the flip / transpose coins (util.py:94-106; a disabled option draws nothing) — so a seeded
    run picks the reference's windows and flips.  lr / hr: NCHW batches (or one CHW sample)."""
    single = lr.dim() == 3
    if single:
        lr, hr = lr[None], hr[None]
    outl, outh = [], []
    for b in range(lr.shape[0]):
        l, h = paired_random_crop(lr[b], hr[b], lr_size, scale)
        l, h = augment([l, h], hflip, rot)
        outl.append(l)
        outh.append(h)
    if single:
        return outl[0], outh[0]
    return torch.stack(outl), torch.stack(outh)


# ------------------------------------------------------------------------------------------------------------------
# The device-resident training set: the pool of decoded images stays on the device as it was decoded (uint8 HWC, or
# float32 CHW), and a batch is ONE esr_batch_assemble launch driven by a table of B items.
# ------------------------------------------------------------------------------------------------------------------
SCALES = (1, 2, 3, 4, 8)
FLAG_HFLIP, FLAG_VFLIP, FLAG_TRANSPOSE = 1, 2, 4


def modcrop(img, scale):
    """``util.modcrop`` (util.py:191-204): drop the rows / columns beyond the largest multiple of ``scale``.
    img: an H x W or H x W x C array (a copy is returned, as the reference does), or a [..., H, W] tensor (CHW)."""
    if isinstance(img, torch.Tensor):
        if img.dim() < 2:
            raise ValueError('Wrong img ndim: [%d].' % img.dim())
        h, w = img.shape[-2:]
        return img[..., :h - h % scale, :w - w % scale].clone()
    import numpy as np
    img = np.copy(img)
    if img.ndim not in (2, 3):
        raise ValueError('Wrong img ndim: [%d].' % img.ndim)
    h, w = img.shape[:2]
    return img[:h - h % scale, :w - w % scale]


def _item_dtype():
    import numpy as np
    dt = np.dtype([(n, {C.c_void_p: '<u8', C.c_int32: '<i4'}[t]) for n, t in L.esr_batch_item._fields_], align=True)
    assert dt.itemsize == C.sizeof(L.esr_batch_item)
    assert all(dt.fields[n][1] == getattr(L.esr_batch_item, n).offset for n, _ in L.esr_batch_item._fields_)
    return dt


def _as_pool_image(img, what, i):
    """-> ('u8', HWC uint8 array of 3 channels) or ('f32', CHW float32 tensor of 3 channels); ValueError otherwise."""
    import numpy as np
    if isinstance(img, torch.Tensor):
        if img.dim() != 3 or img.dtype != torch.float32 or img.shape[0] < 3:
            raise ValueError('TrainSet: %s image %d must be a float32 CHW tensor of 3 channels, got %s %s'
                             % (what, i, img.dtype, tuple(img.shape)))
        return 'f32', img[:3]                                    # some images have 4 channels (util.py:83-84)
    img = np.asarray(img)
    if img.ndim != 3 or img.shape[2] < 3 or img.dtype != np.uint8:
        raise ValueError('TrainSet: %s image %d must be a uint8 H x W x 3 array (grey images are not converted), got '
                         '%s %s' % (what, i, img.dtype, img.shape))
    return 'u8', img[:, :, :3]


class TrainSet:
    """The training set of ``LRHRDataset`` (codes/data/LRHR_dataset.py, phase 'train') held on the device as the pixels a
    decoder produced, and cut into batches by one HIP launch each.

    hr_images (and lr_images, when the LR side is stored rather than generated): uint8 HWC arrays as ``cv2.imread`` /
    PIL give them, or float32 CHW tensors in [0, 1]; one set holds one kind; the images may all differ in size.  Images
    with 4 channels keep the first three (util.py:83-84).  Without ``lr_images`` the LR window of a sample is
    resampled from its HR image on the fly (LRHR_dataset.py:81-85: ``imresize_np(img_HR, 1 / scale)``) — evaluated on
    the whole image's tables, so it equals the crop of the whole image's ``imresize``.  ``bgr=True``: the pool is in
    cv2's channel order and a batch comes out RGB (LRHR_dataset.py:117-119).

    Out of scope (refused with ``ValueError`` in the constructor, before the device is touched): the reference's
    ``cv2.resize`` branches — HR sizes that are no multiple of ``scale`` (LRHR_dataset.py:74-76 resizes them
    bilinearly; ``modcrop`` the images instead), images smaller than the window (:90-96), random scales — and
    ``color`` conversion.

    All pixels live in ONE device buffer; the resample tables are cached on the device per distinct (length, scale)."""

    RING = 4        # pinned item tables: a call may rewrite a table only once the copy that read it is done

    def __init__(self, hr_images, lr_images=None, scale=4, lr_size=32, use_flip=True, use_rot=True, bgr=False,
                 device=None):
        import numpy as np
        if scale not in SCALES:
            raise ValueError('TrainSet: scale must be one of %s, got %r' % (SCALES, scale))
        if int(lr_size) < 1:
            raise ValueError('TrainSet: lr_size must be >= 1, got %r' % (lr_size,))
        hr_images = list(hr_images)
        if not hr_images:
            raise ValueError('TrainSet: no HR images')
        if lr_images is not None:
            lr_images = list(lr_images)
            if len(lr_images) != len(hr_images):
                raise ValueError('TrainSet: %d LR images for %d HR images' % (len(lr_images), len(hr_images)))
        self.scale, self.lr_size = int(scale), int(lr_size)
        self.use_flip, self.use_rot, self.bgr = bool(use_flip), bool(use_rot), bool(bgr)
        kinds = set()
        hrs, lrs = [], []
        for i, im in enumerate(hr_images):
            k, im = _as_pool_image(im, 'HR', i)
            kinds.add(k)
            hrs.append(im)
        for i, im in enumerate(lr_images or []):
            k, im = _as_pool_image(im, 'LR', i)
            kinds.add(k)
            lrs.append(im)
        if len(kinds) != 1:
            raise ValueError('TrainSet: one set holds one kind of image, uint8 HWC arrays or float32 CHW tensors, not both')
        self.kind = kinds.pop()
        hw = (lambda im: tuple(im.shape[:2])) if self.kind == 'u8' else (lambda im: tuple(im.shape[1:]))
        self.sizes = [hw(im) for im in hrs]                        # (H, W) of every HR image
        lr_sizes = []
        for i, (h, w) in enumerate(self.sizes):
            if lrs:
                lh, lw = hw(lrs[i])
                if (h, w) != (self.scale * lh, self.scale * lw):
                    raise ValueError('TrainSet: HR image %d is %d x %d, not %d times its LR image of %d x %d'
                                     % (i, h, w, self.scale, lh, lw))
            else:
                if h % self.scale or w % self.scale:
                    raise ValueError('TrainSet: HR image %d is %d x %d, not a multiple of scale %d in both directions: '
                                     'cut it with data.modcrop(img, %d) first (the reference resizes it instead, which '
                                     'this project does not restate)' % (i, h, w, self.scale, self.scale))
                lh, lw = h // self.scale, w // self.scale
            if lh < self.lr_size or lw < self.lr_size:
                raise ValueError('TrainSet: the LR side of image %d is %d x %d, smaller than the %d x %d window (the '
                                 'reference resizes such images, which this project does not restate)'
                                 % (i, lh, lw, self.lr_size, self.lr_size))
            lr_sizes.append((lh, lw))
        self.lr_sizes = lr_sizes
        if device is not None and torch.device(device).type != 'cuda':
            raise ValueError('TrainSet: the pool lives on the MI355X, got device %s' % (device,))

        # ---- from here on the device is used ----
        dev = torch.device('cuda') if device is None else torch.device(device)
        self.device = torch.device('cuda', torch.cuda.current_device()) if dev.index is None else dev
        L.lib()
        esz = 1 if self.kind == 'u8' else 4
        flat, offs, pos = [], [], 0
        for im in hrs + lrs:
            a = np.ascontiguousarray(im) if self.kind == 'u8' else im.contiguous().numpy()
            offs.append(pos)
            flat.append(a.reshape(-1))
            pos += a.size
        host = np.concatenate(flat)
        self.pool = torch.from_numpy(host).to(self.device)          # ONE allocation, an offset per image
        self.pool_bytes = host.size * esz
        base = self.pool.data_ptr()
        n = len(hrs)
        self._tables = {}                                             # (length, scale) -> (w, idx, taps) on the device
        rec = np.zeros(n, dtype=_item_dtype())
        for i in range(n):
            rec['hr'][i] = base + offs[i] * esz
            rec['hr_h'][i], rec['hr_w'][i] = self.sizes[i]
            rec['lr_h'][i], rec['lr_w'][i] = lr_sizes[i]
            if lrs:
                rec['lr'][i] = base + offs[n + i] * esz
            else:
                wy, iy, ty = self._table(self.sizes[i][0])
                wx, ix, tx = self._table(self.sizes[i][1])
                rec['wy'][i], rec['iy'][i], rec['taps_y'][i] = wy.data_ptr(), iy.data_ptr(), ty
                rec['wx'][i], rec['ix'][i], rec['taps_x'][i] = wx.data_ptr(), ix.data_ptr(), tx
        self._static = rec
        self._lr_h = np.array([s[0] for s in lr_sizes], dtype=np.int64)
        self._lr_w = np.array([s[1] for s in lr_sizes], dtype=np.int64)
        # The item table of a call goes to the device through a ring of RING pinned tables (engine.PinnedRing): one
        # non-blocking copy, no device synchronisation.
        self._ring = E.PinnedRing(self.RING)

    def _table(self, length):
        key = (int(length), self.scale)
        t = self._tables.get(key)
        if t is None:
            w, idx, out_len = resample_tables(length, 1.0 / self.scale)
            assert out_len == length // self.scale and w.shape == idx.shape, (length, self.scale, out_len)
            t = self._tables[key] = (w.to(self.device), idx.to(self.device), int(w.shape[1]))
        return t

    def __len__(self):
        return len(self.sizes)

    def draw(self, indices):
        """The crop windows and flips of the samples ``indices``, from Python's ``random`` in the reference's per-item
        order (LRHR_dataset.py:102-103 then util.py:96-98): randint, randint, then the coins of the enabled options
        -> [(y0, x0, flags)], flags = hflip | vflip << 1 | transpose << 2.  Host code only."""
        out = []
        for i in indices:
            lh, lw = self.lr_sizes[i]
            y0 = random.randint(0, max(0, lh - self.lr_size))
            x0 = random.randint(0, max(0, lw - self.lr_size))
            hf = self.use_flip and random.random() < 0.5
            vf = self.use_rot and random.random() < 0.5
            r9 = self.use_rot and random.random() < 0.5
            out.append((y0, x0, (FLAG_HFLIP if hf else 0) | (FLAG_VFLIP if vf else 0) | (FLAG_TRANSPOSE if r9 else 0)))
        return out

    def batch(self, indices, draws=None):
        """-> (lr [B, 3, s, s], hr [B, 3, s scale, s scale]): float32 NCHW on the device, fresh tensors every call, one
        launch on the current stream, no device synchronisation.  draws: [(y0, x0, flags)] per sample (``draw``'s
        result; drawn now if None)."""
        import numpy as np
        idx = np.asarray(list(indices), dtype=np.int64).reshape(-1)
        B = idx.size
        if B < 1 or B > 65535:
            raise ValueError('TrainSet.batch: %d samples (1 ... 65535)' % B)
        if idx.min() < 0 or idx.max() >= len(self):
            raise ValueError('TrainSet.batch: indices outside the set of %d images' % len(self))
        if draws is None:
            draws = self.draw(idx.tolist())
        d = np.asarray(draws, dtype=np.int64).reshape(-1, 3)
        if d.shape[0] != B:
            raise ValueError('TrainSet.batch: %d draws for %d samples' % (d.shape[0], B))
        s = self.lr_size
        if ((d[:, 0] < 0) | (d[:, 0] > self._lr_h[idx] - s) | (d[:, 1] < 0) | (d[:, 1] > self._lr_w[idx] - s)
                | (d[:, 2] < 0) | (d[:, 2] > 7)).any():
            raise ValueError('TrainSet.batch: a window outside its image, or flags outside 0 ... 7')
        with torch.cuda.device(self.device):
            lr = torch.empty((B, 3, s, s), dtype=torch.float32, device=self.device)
            hr = torch.empty((B, 3, s * self.scale, s * self.scale), dtype=torch.float32, device=self.device)
            self._assemble(idx, d, lr, hr)
        return lr, hr

    def _assemble(self, idx, d, lr, hr):
        """The launch behind ``batch``: samples idx (int64 array) with draws d (int64 [B, 3], validated by the caller)
        into the contiguous float32 tensors lr / hr, on the current stream of the current device (= self.device)."""
        B, s = idx.size, self.lr_size
        assert lr.is_contiguous() and hr.is_contiguous() and lr.dtype == hr.dtype == torch.float32
        assert lr.numel() == B * 3 * s * s and hr.numel() == lr.numel() * self.scale ** 2
        assert lr.device == hr.device == self.device
        rec = self._static[idx]
        rec['y0'], rec['x0'], rec['flags'] = d[:, 0], d[:, 1], d[:, 2]
        table = self._ring.upload(rec, self.device)
        a = L.esr_batch()
        a.B, a.C, a.lr_size, a.scale = B, 3, s, self.scale
        a.src_format, a.swap_rb = (1 if self.kind == 'u8' else 0), int(self.bgr)
        a.lr_out, a.hr_out, a.items = lr.data_ptr(), hr.data_ptr(), table.data_ptr()
        L.check(L.lib().esr_batch_assemble(C.byref(a), C.c_void_p(E.current_stream())), 'esr_batch_assemble')
        return a, table

    def epoch(self, batch_size, shuffle=True, drop_last=True):
        """Batches over one pass of the set, in a ``torch.randperm`` order when shuffled (not the order of the
        reference's ``DataLoader``, which with workers is not reproducible either)."""
        n = len(self)
        order = torch.randperm(n).tolist() if shuffle else list(range(n))
        for i in range(0, n, batch_size):
            ids = order[i:i + batch_size]
            if len(ids) < batch_size and drop_last:
                return
            yield self.batch(ids)


def batch_reference(hr_images, lr_images, scale, lr_size, draws, bgr=False):
    """What ``TrainSet.batch`` computes, restated with torch on the CPU in float32 — the yardstick of its tests, itself
    pinned to the reference's ``LRHRDataset.__getitem__`` by tests/golden/batch_assemble.npz.  hr_images / lr_images:
    the images of the batch's samples, one per draw (lr_images None: the LR window is cut from the whole image's
    resample — the tables of ``resample_tables`` evaluated as sums over the taps, H pass then W pass).
    -> (lr [B, 3, s, s], hr [B, 3, s scale, s scale])"""
    import numpy as np

    def chw(img):
        if isinstance(img, torch.Tensor):
            return img[:3].float()
        a = np.asarray(img)[:, :, :3]
        return torch.from_numpy(np.ascontiguousarray(np.transpose(a.astype(np.float32) / np.float32(255.), (2, 0, 1))))

    def resample(x):
        return table_resample(x, scale)

    outl, outh = [], []
    whole = {}                                                        # the resample of an image used more than once
    for b, (y0, x0, flags) in enumerate(draws):
        hr = chw(hr_images[b])
        if lr_images is not None:
            lr = chw(lr_images[b])
        else:
            key = id(hr_images[b])
            if key not in whole:
                whole[key] = resample(hr)
            lr = whole[key]
        l = lr[:, y0:y0 + lr_size, x0:x0 + lr_size]
        h = hr[:, scale * y0:scale * (y0 + lr_size), scale * x0:scale * (x0 + lr_size)]
        assert l.shape[1:] == (lr_size, lr_size) and h.shape[1:] == (scale * lr_size, scale * lr_size), (b, y0, x0)
        for bit, fn in ((FLAG_HFLIP, lambda t: t.flip(-1)), (FLAG_VFLIP, lambda t: t.flip(-2)),
                        (FLAG_TRANSPOSE, lambda t: t.transpose(-1, -2))):
            if flags & bit:
                l, h = fn(l), fn(h)
        if bgr:
            l, h = l.flip(0), h.flip(0)
        outl.append(l)
        outh.append(h)
    return torch.stack(outl).contiguous(), torch.stack(outh).contiguous()
