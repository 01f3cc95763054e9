"""Image conversion + PSNR exactly as the reference's validation does it
(codes/utils/util.py:71-95 ``tensor2img``, 107-114 ``calculate_psnr``; codes/train.py:131-148: crop
``scale`` pixels, compare uint8 images).  The numpy functions are the host restatement (pinned by
tests/golden/psnr.npz, metrics.npz); ``device_tensor2img`` / ``device_psnr_ssim`` run the same arithmetic in
csrc/metrics.hip on the tensors' GPU, so that a validation pass over many images reads back four doubles per
image pair instead of two images.  ``device_set_metrics`` (csrc/metrics_set.hip) scores a whole set of uint8 image
pairs — PSNR, SSIM, PSNR_Y, SSIM_Y as codes/test.py:69-110 — in one device pass; ``set_metrics_reference`` restates it."""
import math

import numpy as np


def tensor2img(t, min_max=(0, 1)):
    """3-D (C,H,W) RGB tensor -> uint8 HWC **BGR** image, clamped and rounded like the reference."""
    a = t.detach().squeeze().float().cpu().clamp(*min_max).numpy()
    a = (a - min_max[0]) / (min_max[1] - min_max[0])
    if a.ndim == 3:
        a = np.transpose(a[[2, 1, 0], :, :], (1, 2, 0))
    return (a * 255.0).round().astype(np.uint8)


def calculate_psnr(img1, img2):
    mse = np.mean((img1.astype(np.float64) - img2.astype(np.float64)) ** 2)
    if mse == 0:
        return float('inf')
    return 20 * math.log10(255.0 / math.sqrt(mse))


def validation_psnr(sr, hr, scale=4):
    a, b = tensor2img(sr) / 255., tensor2img(hr) / 255.
    a, b = a[scale:-scale, scale:-scale, :], b[scale:-scale, scale:-scale, :]
    return calculate_psnr(a * 255, b * 255)


# ---- SSIM and Y-channel conversion (codes/utils/util.py:117-158, codes/data/util.py:123-168) -----------
_Y_RGB = np.array([65.481, 128.553, 24.966])
_YCC_RGB = np.array([[65.481, -37.797, 112.0], [128.553, -74.203, -93.786], [24.966, 112.0, -18.214]])


def _ycbcr(img, coeff_y, coeff_full, only_y):
    """MATLAB-style conversion for uint8 [0,255] (rounded) or float [0,1] HWC images.  Unlike the
    reference (data/util.py:132-134) the input array is not scaled in place."""
    is_u8 = img.dtype == np.uint8
    x = img.astype(np.float64) if is_u8 else img.astype(np.float64) * 255.0
    if only_y:
        r = np.dot(x, coeff_y) / 255.0 + 16.0
    else:
        r = np.matmul(x, coeff_full) / 255.0 + np.array([16, 128, 128])
    r = r.round() if is_u8 else r / 255.0
    return r.astype(img.dtype)


def rgb2ycbcr(img, only_y=True):
    return _ycbcr(img, _Y_RGB, _YCC_RGB, only_y)


def bgr2ycbcr(img, only_y=True):
    return _ycbcr(img, _Y_RGB[::-1], _YCC_RGB[::-1], only_y)


def gaussian_window(ksize=11, sigma=1.5):
    """cv2.getGaussianKernel(11, 1.5) outer itself: exp(-(i-c)^2 / (2 sigma^2)), normalised."""
    i = np.arange(ksize, dtype=np.float64) - (ksize - 1) / 2.0
    k = np.exp(-(i * i) / (2.0 * sigma * sigma))
    k /= k.sum()
    return np.outer(k, k)


def _ssim_plane(a, b):
    """util.py:117-137: 11x11 Gaussian-window SSIM over the valid region of two [0,255] planes.
    The filtering runs as a conv2d on whatever device the planes live on (float64)."""
    import torch
    import torch.nn.functional as F
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    a = torch.as_tensor(a, dtype=torch.float64)
    b = torch.as_tensor(b, dtype=torch.float64, device=a.device)
    w = torch.as_tensor(gaussian_window(), dtype=torch.float64, device=a.device)[None, None]
    stack = torch.stack([a, b, a * a, b * b, a * b])[:, None]           # 5 x 1 x H x W
    f = F.conv2d(stack, w)[:, 0]                                          # 'valid' == filter2D(...)[5:-5, 5:-5]
    mu1, mu2 = f[0], f[1]
    s1, s2, s12 = f[2] - mu1 * mu1, f[3] - mu2 * mu2, f[4] - mu1 * mu2
    m = ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2))
    return float(m.mean())


def calculate_ssim(img1, img2):
    """util.py:140-158, including its quirk: for 3-channel inputs the reference averages three calls
    on the FULL (H, W, 3) arrays — cv2.filter2D filters each channel, so that equals the mean over
    channels of the per-channel SSIM maps."""
    if img1.shape != img2.shape:
        raise ValueError('Input images must have the same dimensions.')
    if img1.ndim == 2:
        return _ssim_plane(img1, img2)
    if img1.ndim == 3:
        if img1.shape[2] == 3:
            return float(np.mean([_ssim_plane(img1[..., c], img2[..., c]) for c in range(3)]))
        if img1.shape[2] == 1:
            return _ssim_plane(np.squeeze(img1), np.squeeze(img2))
        return None             # util.py:151-156 falls off the end for 2- or 4-channel images: None, as the reference
    raise ValueError('Wrong input image dimensions.')


# ---- the same on the device (csrc/metrics.hip, esr_image_metrics) -------------------------------------
def _metrics_call(sr, hr, crop, y_only, min_max):
    import torch
    from . import _lib as L
    from . import engine as E
    E.require_cuda(sr, 'sr')
    a = sr.detach().squeeze().float().contiguous()
    if a.dim() == 2:
        a = a[None]
    C_, H, W = a.shape
    dev = a.device
    p = L.esr_img_metrics()
    p.sr, p.C, p.H, p.W, p.crop, p.y_only = a.data_ptr(), C_, H, W, int(crop), 1 if y_only else 0
    p.lo, p.hi = float(min_max[0]), float(min_max[1])
    keep = [a]
    img_sr = torch.empty((H, W, C_) if C_ == 3 else (H, W), dtype=torch.uint8, device=dev)
    p.img_sr = img_sr.data_ptr()
    img_hr = out = None
    if hr is not None:
        b = hr.detach().squeeze().float().contiguous()
        if b.dim() == 2:
            b = b[None]
        if b.shape != a.shape or b.device != dev:
            raise ValueError('Input images must have the same dimensions.')
        img_hr = torch.empty_like(img_sr)
        out = torch.empty(4, dtype=torch.float64, device=dev)
        p.hr, p.img_hr, p.out = b.data_ptr(), img_hr.data_ptr(), out.data_ptr()
        keep.append(b)
    if y_only:
        ys = torch.empty((2, H, W), dtype=torch.float64, device=dev)     # unrounded luma (codes/test.py:81-86)
        p.y_sr, p.y_hr = ys[0].data_ptr(), ys[1].data_ptr()
        keep.append(ys)
    k1 = gaussian_window()[5] / gaussian_window()[5].sum()       # the normalised 1-D kernel (outer(k, k) == window)
    for i in range(11):
        p.win[i] = float(k1[i])
    L.check(L.lib().esr_image_metrics(p, E.current_stream()), 'esr_image_metrics')
    return img_sr, img_hr, out, (C_, H, W), keep


def device_tensor2img(t, min_max=(0, 1)):
    """tensor2img on the tensor's GPU: uint8 HWC BGR (or HW) tensor, bit-identical with ``tensor2img``."""
    return _metrics_call(t, None, 0, False, min_max)[0]


def device_psnr_ssim(sr, hr, crop=4, y_only=False, min_max=(0, 1)):
    """(PSNR, SSIM) of two (C,H,W) tensors exactly as the validation loops compute them (tensor2img both, crop
    `crop` pixels per side), evaluated on the device; one small read-back.  y_only: PSNR_Y / SSIM_Y of
    codes/test.py:81-90 — ``bgr2ycbcr(img / 255., only_y=True)`` on the FLOAT images, i.e. unrounded luma."""
    _, _, out, (C_, H, W), keep = _metrics_call(sr, hr, crop, y_only, min_max)
    o = out.cpu().numpy()                       # synchronises with the metric kernels
    planes = 1 if (y_only or C_ == 1) else C_
    ch, cw = H - 2 * crop, W - 2 * crop
    mse = o[0] / (ch * cw * planes)
    psnr = float('inf') if mse == 0 else 20 * math.log10(255.0 / math.sqrt(mse))
    ssim = float(o[2] / ((ch - 10) * (cw - 10) * planes)) if (ch > 10 and cw > 10) else float('nan')
    return psnr, ssim


# ---- a whole image set at once (csrc/metrics_set.hip, esr_image_set_metrics; codes/test.py:69-110) -----------------
def _set_pairs(sr_images, hr_images):
    """The two image lists of a set metric as lists of equal length; every image a uint8 [H, W, 3] tensor (or, for the
    host restatement, array) with pixels, every pair of one shape.  ``functional._images_u8``'s checks and wording."""
    import torch
    from .functional import _images_u8
    lists = []
    for images in (sr_images, hr_images):
        images = [torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x for x in images]
        lists.append(_images_u8(images))
    sr, hr = lists
    if len(sr) != len(hr):
        raise ValueError('a set metric compares equally many images: %d sr, %d hr' % (len(sr), len(hr)))
    for a, b in zip(sr, hr):
        if a.shape != b.shape:
            raise ValueError('Input images must have the same dimensions.')
    return sr, hr


def _set_crop(sizes, crop):
    import operator
    try:
        if isinstance(crop, bool):
            raise TypeError
        crop = operator.index(crop)
    except TypeError:
        raise ValueError('crop of a set metric must be an int >= 0, got %r' % (crop,))
    if crop < 0:
        raise ValueError('crop of a set metric must be an int >= 0, got %r' % (crop,))
    for i, (H, W) in enumerate(sizes):
        if H - 2 * crop < 1 or W - 2 * crop < 1:
            raise ValueError('crop = %d leaves no pixels of image %d (%d x %d)' % (crop, i, H, W))
    return crop


def set_metrics_reference(sr_images, hr_images, crop, bgr=False):
    """Pure numpy restatement of ``device_set_metrics`` on any machine: (psnr, ssim, psnr_y, ssim_y) of every pair of
    uint8 [H, W, 3] images (arrays or CPU tensors) exactly as codes/test.py:71-90 computes them with ``calculate_psnr``,
    ``calculate_ssim`` and ``bgr2ycbcr`` — both images / 255., `crop` pixels cut from every side, the luma taken from
    the FLOAT images and therefore unrounded.  ``bgr=False``: the arrays hold R, G, B (PIL) and are flipped first; the
    script's images are cv2's B, G, R.  -> float64 array [n, 4]; ssim and ssim_y are nan where the cropped image has no
    11 x 11 window."""
    sr, hr = _set_pairs(sr_images, hr_images)
    crop = _set_crop([(x.shape[0], x.shape[1]) for x in sr], crop)
    out = np.empty((len(sr), 4), dtype=np.float64)
    for i, (a, b) in enumerate(zip(sr, hr)):
        a, b = a.detach().cpu().numpy(), b.detach().cpu().numpy()
        if not bgr:
            a, b = a[:, :, ::-1], b[:, :, ::-1]
        a, b = a / 255., b / 255.
        H, W = a.shape[:2]
        has_ssim = H - 2 * crop > 10 and W - 2 * crop > 10
        ca, cb = a[crop:H - crop, crop:W - crop, :], b[crop:H - crop, crop:W - crop, :]
        out[i, 0] = calculate_psnr(ca * 255, cb * 255)
        out[i, 1] = calculate_ssim(ca * 255, cb * 255) if has_ssim else float('nan')
        ya, yb = bgr2ycbcr(a, only_y=True)[crop:H - crop, crop:W - crop], bgr2ycbcr(b, only_y=True)[crop:H - crop, crop:W - crop]
        out[i, 2] = calculate_psnr(ya * 255, yb * 255)
        out[i, 3] = calculate_ssim(ya * 255, yb * 255) if has_ssim else float('nan')
    return out


class SetMetricsResult:
    """What ``device_set_metrics`` queued: ``sums`` is the float64 device tensor [n, 4] of esr_image_set_metrics' raw
    sums, complete once the stream it was queued on has run.  ``read()`` is the one read-back."""

    def __init__(self, sums, sizes, crop):
        self.sums, self.sizes, self.crop = sums, list(sizes), crop
        self._table = None

    def __len__(self):
        return len(self.sizes)

    def read(self):
        """-> float64 array [n, 4] of (psnr, ssim, psnr_y, ssim_y) per pair, ``device_psnr_ssim``'s formulas: psnr inf
        for zero error, ssim nan where the cropped image has no 11 x 11 window.  Synchronises with the metric kernels
        the first time; the table is kept."""
        if self._table is None:
            o = self.sums.cpu().numpy() if len(self.sizes) else np.zeros((0, 4))
            t = np.empty((len(self.sizes), 4), dtype=np.float64)
            for i, (H, W) in enumerate(self.sizes):
                ch, cw = H - 2 * self.crop, W - 2 * self.crop
                for k, planes in ((0, 3), (1, 1)):
                    mse = o[i, k] / (ch * cw * planes)
                    t[i, 2 * k] = float('inf') if mse == 0 else 20 * math.log10(255.0 / math.sqrt(mse))
                    t[i, 2 * k + 1] = o[i, 2 + k] / ((ch - 10) * (cw - 10) * planes) if (ch > 10 and cw > 10) else float('nan')
            self._table = t
        return self._table

    def averages(self):
        """(psnr, ssim, psnr_y, ssim_y) averaged as codes/test.py:102-108 does: ``sum(values) / len(values)``."""
        t = self.read()
        if not len(t):
            raise ValueError('an empty image set has no averages')
        return tuple(sum(float(v) for v in t[:, k]) / len(t) for k in range(4))


_set_rings = {}


def device_set_metrics(sr_images, hr_images, crop=4, bgr=False):
    """PSNR, SSIM, PSNR_Y and SSIM_Y of an image set in one device pass (csrc/metrics_set.hip): ``sr_images`` and
    ``hr_images`` are equally long sequences of ``torch.uint8`` tensors [H, W, 3] on one GPU, sizes free per pair —
    ``forward_images``' results and their ground truth.  ``crop`` pixels are cut from every side (codes/test.py:75: the
    scale); ``bgr``: byte 0 of a pixel is B (cv2, ``device_tensor2img``, ``forward_images(bgr=True)``), else R (PIL).
    The item table goes up through a pinned ring in one non-blocking copy; two launches on the current stream whatever
    the set, no synchronisation.  -> a ``SetMetricsResult``; its ``read()`` is the one read-back.  Two calls on the same
    images give the same bits, and an image's numbers do not depend on the rest of the set."""
    import torch
    from . import _lib as L
    from . import engine as E
    sr, hr = _set_pairs(sr_images, hr_images)
    sizes = [(int(x.shape[0]), int(x.shape[1])) for x in sr]
    crop = _set_crop(sizes, crop)
    if not sr:
        return SetMetricsResult(None, [], crop)
    dev = sr[0].device
    for i, x in enumerate(sr + hr):
        if x.device != dev:
            raise ValueError('image %d is on %s, image 0 on %s: a set metric runs on one device' % (i % len(sr), x.device, dev))
    if dev.type != 'cuda':
        raise ValueError('the images of a set metric are on %s: the HIP path needs tensors on an MI355X; there is no '
                         'CPU fallback (set_metrics_reference is the host restatement)' % (dev,))
    sr, hr = [x.detach().contiguous() for x in sr], [x.detach().contiguous() for x in hr]
    n = len(sr)
    th, tw = L.SET_METRICS_TILE_H, L.SET_METRICS_TILE_W
    hw = np.array(sizes, dtype=np.int32)
    units = (-(-(hw[:, 0].astype(np.int64) - 2 * crop) // th)) * (-(-(hw[:, 1].astype(np.int64) - 2 * crop) // tw))
    n_units = int(units.sum())
    if n_units > 2 ** 31 - 1:
        raise ValueError('%d tiles of %d x %d are more than one launch takes' % (n_units, th, tw))
    rec = np.zeros(n, dtype=np.dtype([('sr', '<u8'), ('hr', '<u8'), ('H', '<i4'), ('W', '<i4'), ('first', '<i4'),
                                      ('_pad', '<i4')]))              # esr_set_metrics_item
    rec['sr'] = np.array([x.data_ptr() for x in sr], dtype=np.uint64)
    rec['hr'] = np.array([x.data_ptr() for x in hr], dtype=np.uint64)
    rec['H'], rec['W'] = hw[:, 0], hw[:, 1]
    rec['first'] = np.concatenate([[0], np.cumsum(units)[:-1]])
    with torch.cuda.device(dev):
        ring = _set_rings.get(dev.index)
        if ring is None:
            ring = _set_rings[dev.index] = E.PinnedRing()
        table = ring.upload(rec, dev)
        sums = torch.empty((n, 4), dtype=torch.float64, device=dev)
        scratch = torch.empty(4 * n_units, dtype=torch.float64, device=dev)
        p = L.esr_set_metrics()
        p.n, p.crop, p.bgr, p.n_units = n, crop, 1 if bgr else 0, n_units
        hw = np.ascontiguousarray(hw)
        p.items, p.sizes_host, p.out, p.scratch = table.data_ptr(), hw.ctypes.data, sums.data_ptr(), scratch.data_ptr()
        k1 = gaussian_window()[5] / gaussian_window()[5].sum()       # the normalised 1-D kernel, as _metrics_call passes it
        for i in range(11):
            p.win[i] = float(k1[i])
        L.check(L.lib().esr_image_set_metrics(p, E.current_stream()), 'esr_image_set_metrics')
    return SetMetricsResult(sums, sizes, crop)
