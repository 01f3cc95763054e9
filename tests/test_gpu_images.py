"""8-bit image-in, image-out inference on the GPU: the gather that reads uint8 HWC images (csrc/tile_img.hip,
esr_tile_img) byte for byte against the existing ``esr_tile_many_op`` gather on the float image, the stitch that writes
them against torch's clamp / x 255 / round of the slots, then ``forward_images`` against ``device_tensor2img`` of
``forward_tiled_many`` and against ``images_reference``, the shared launch plans, the mode / autograd contract, the
reference's images for the five bundled inputs, ``tools/sr_infer.py --tile-u8`` and the entry's refusals."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from esrganplus_amd import functional as F
from esrganplus_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (LR sizes, tile, pad, slots per pass), as tests/test_gpu_tiled_many.py
CASES = [([(40, 52), (33, 70)], 16, 4, 5),     # 12 + 15 windows of 24 x 24: 6 passes, pass 2 crosses the images, 3 filler slots
         ([(33, 70), (45, 70)], 32, 8, 4)]     # 6 + 6 windows of 33 x 48 / 45 x 48 -> two groups; crosses the 32- and 64-wide edges
# 13 x 21: an odd width and a window (13 x 21) smaller than tile + 2 pad = 24; 16 x 16: a single tile
STITCH_CASES = CASES + [([(13, 21), (16, 16)], 16, 4, 5)]
MIXED = [(40, 52), (33, 70), (13, 21), (16, 16)]
SENTINEL = -77.25                              # exact in fp16 and fp32
FILL = 0xA5
ESR_ERR_INVALID, ESR_ERR_UNSUPPORTED = -1, -3
LUT = torch.arange(256, dtype=torch.float32) / 255.0       # the 256 quotients, divided on the CPU (a true division)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _same_bits(a, b):
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def _u8(seed, sizes, C_=3):
    """Seeded uint8 [H, W, C] CPU images that contain all 256 values."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for H, W in sizes:
        x = torch.randint(0, 256, (H, W, C_), generator=g, dtype=torch.uint8)
        x.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)[torch.randperm(256, generator=g)]
        assert len(torch.unique(x)) == 256
        out.append(x)
    return out


def _nchw(x, bgr=False):
    """The float32 [1, C, H, W] image the scripts make of the uint8 HWC image x (CPU), channel 0 = R."""
    return LUT[(x.flip(2) if bgr and x.shape[2] == 3 else x).permute(2, 0, 1).long()].unsqueeze(0).contiguous()


def _table(dev, entries):
    """[(tensor, H, W, t, live)] -> the uint8 device tensor of 24-byte item entries."""
    rec = np.zeros(len(entries), dtype=F._tile_item_dtype())
    for k, (img, H, W, t, live) in enumerate(entries):
        rec[k] = (img.data_ptr(), H, W, t, live)
    return torch.from_numpy(rec.view(np.uint8).copy()).to(dev)


def _op(kind, to_g32, table, n_slots, C_, tile, pad, th, tw, g=None, slots=None, prec='fp32', check=True, **over):
    """esr_tile_img_op (kind 'img') or the existing esr_tile_many_op (kind 'many') with the same fields."""
    from esrganplus_amd import _lib as L, engine as E
    d = L.esr_tile_img() if kind == 'img' else L.esr_tile_many()
    d.dtype = g.esr_dtype if g is not None else E._dt(prec)[0]
    d.to_g32, d.C, d.tile, d.pad, d.scale = to_g32, C_, tile, pad, 1 if to_g32 else 4
    d.th, d.tw, d.n_slots = th, tw, n_slots
    d.items = table.data_ptr() if table is not None else None
    if g is not None:
        d.g32 = g.view(0, C_)
    if slots is not None:
        d.slots_nchw = slots.data_ptr()
    for k, v in over.items():
        setattr(d, k, v)
    name = 'esr_tile_img_op' if kind == 'img' else 'esr_tile_many_op'
    rc = getattr(L.lib(), name)(C.byref(d), C.c_void_p(E.current_stream()))
    if check:
        L.check(rc, name)
    return rc


# ---- 1. the gather is the float gather on u8 / 255 ------------------------------------------------------------------
@pytest.mark.parametrize('bgr', [0, 1])
@pytest.mark.parametrize('C_', [3, 1])
@pytest.mark.parametrize('prec', ['fp16', 'fp32'])
def test_gather_equals_the_float_gather_on_the_divided_image(dev, prec, C_, bgr):
    from esrganplus_amd import engine as E
    for sizes, tile, pad, S in CASES:
        u8 = [x.to(dev) for x in _u8(11, sizes, C_)]
        xf = [_nchw(x.cpu(), bgr).to(dev) for x in u8]
        groups = F.tiled_many_passes(sizes, tile, pad, S)
        assert any(not l for _, _, _, ps in groups for p in ps for _, _, l in p)      # filler is covered
        for th, tw, Sg, passes in groups:
            for p in passes:
                ref, got = (E.G32(Sg, C_, th, tw, prec, dev) for _ in range(2))
                ref.t.fill_(SENTINEL)
                got.t.fill_(SENTINEL)
                _op('many', 1, _table(dev, [(xf[i], sizes[i][0], sizes[i][1], t, live) for i, t, live in p]),
                    Sg, C_, tile, pad, th, tw, g=ref)
                _op('img', 1, _table(dev, [(u8[i], sizes[i][0], sizes[i][1], t, live) for i, t, live in p]),
                    Sg, C_, tile, pad, th, tw, g=got, bgr=bgr)
                torch.cuda.synchronize()
                # the whole buffer, byte for byte: halo and padding still hold the sentinel in both
                assert _same_bits(got.t, ref.t), p
                assert not bool((got.t[:, 0, 1:th + 1, 1:tw + 1, :C_] == SENTINEL).any())
                assert bool((got.t[:, :, 0] == SENTINEL).all()) and bool((got.t[:, :, :, 0] == SENTINEL).all())
                assert bool((got.t[:, :, th + 1:] == SENTINEL).all()) and bool((got.t[:, :, :, tw + 1:] == SENTINEL).all())


# ---- 2. the stitch is torch's clamp, x 255, round of the owned rectangles -------------------------------------------
def _quant(v, bgr):
    """[C, h, w] float32 (CPU) -> uint8 [h, w, C] in the requested channel order."""
    q = (v.clamp(0, 1) * 255.0).round().to(torch.uint8).permute(1, 2, 0)
    return q.flip(2) if bgr and q.shape[2] == 3 else q


@pytest.mark.parametrize('bgr', [0, 1])
@pytest.mark.parametrize('C_', [3, 1])
def test_stitch_writes_the_quantised_owned_rectangles_and_nothing_else(dev, C_, bgr):
    for ci, (sizes, tile, pad, S) in enumerate(STITCH_CASES):
        groups = F.tiled_many_passes(sizes, tile, pad, S)
        geo = [F.tiled_geometry(H, W, tile, pad) for H, W in sizes]
        got = [torch.full((4 * H, 4 * W, C_), FILL, dtype=torch.uint8, device=dev) for H, W in sizes]
        want = [torch.full((4 * H, 4 * W, C_), FILL, dtype=torch.uint8) for H, W in sizes]
        covered = [torch.zeros((4 * H, 4 * W), dtype=torch.bool) for H, W in sizes]
        first = True
        for gi, (th, tw, Sg, passes) in enumerate(groups):
            for pi, p in enumerate(passes):
                s_cpu = synth.normal_like(1000 * ci + 100 * gi + pi, 'images.stitch', (Sg, C_, 4 * th, 4 * tw)) * 0.6 + 0.5
                below, above = float((s_cpu < 0).float().mean()), float((s_cpu > 1).float().mean())
                assert below >= 0.1 and above >= 0.1 and below + above < 0.9, (below, above)
                slots = s_cpu.to(dev)
                _op('img', 0, _table(dev, [(got[i], sizes[i][0], sizes[i][1], t, live) for i, t, live in p]),
                    Sg, C_, tile, pad, th, tw, slots=slots, bgr=bgr)
                for s, (i, t, live) in enumerate(p):
                    if live:
                        y0, y1, x0, x1, wy, wx = geo[i][4][t]
                        want[i][4 * y0:4 * y1, 4 * x0:4 * x1] = _quant(
                            s_cpu[s, :, 4 * (y0 - wy):4 * (y1 - wy), 4 * (x0 - wx):4 * (x1 - wx)], bgr)
                        assert not bool(covered[i][4 * y0:4 * y1, 4 * x0:4 * x1].any())
                        covered[i][4 * y0:4 * y1, 4 * x0:4 * x1] = True
                if first:
                    first = False
                    torch.cuda.synchronize()
                    # the first pass wrote its own live tiles' owned rectangles (want so far) and nothing else (FILL)
                    assert any(live for _, _, live in p) and not all(bool(c.all()) for c in covered)
                    for i in range(len(sizes)):
                        assert _same_bits(got[i], want[i]), (ci, i)
        torch.cuda.synchronize()
        for i in range(len(sizes)):
            assert bool(covered[i].all())                         # the live slots cover every image exactly once
            assert _same_bits(got[i], want[i]), (ci, i)


def test_stitch_skips_filler_slots(dev):
    """A pass of nothing but filler writes nothing, whatever its slots hold."""
    H, W, tile, pad = 13, 21, 8, 2
    y = torch.full((4 * H, 4 * W, 3), FILL, dtype=torch.uint8, device=dev)
    slots = synth.normal_like(5, 'images.filler', (3, 3, 48, 48)).to(dev)
    _op('img', 0, _table(dev, [(y, H, W, t, 0) for t in (0, 3, 5)]), 3, 3, tile, pad, 12, 12, slots=slots)
    torch.cuda.synchronize()
    assert bool((y == FILL).all())


# ---- nets -----------------------------------------------------------------------------------------------------------
def _wide_state_dict(nb=1, seed=1):
    """synth's weights with HR_conv1 scaled and shifted (12 y + 0.5): the synthetic net's outputs stay within +-0.1,
    whatever the seed, and would never reach the upper clamp; with this they run from below 0 to above 1."""
    sd = synth.rrdbnet_state_dict(nb=nb, seed=seed)
    sd['model.10.weight'] = sd['model.10.weight'] * 12.0
    sd['model.10.bias'] = sd['model.10.bias'] * 12.0 + 0.5
    return sd


def _net(dev, nb, sd, prec='fp32', cls='RRDBNet'):
    from esrganplus_amd import architecture as arch
    net = getattr(arch, cls)(3, 3, 64, nb).to(dev).eval()
    net.load_state_dict(sd, strict=True)
    return net.set_precision(prec)


def _keys(net, kind):
    return [k for k in net._plans if k[0] == kind]


# ---- 3. end to end: device_tensor2img of forward_tiled_many, and the restatement ------------------------------------
@pytest.mark.parametrize('prec', ['fp32', 'fp16'])
@pytest.mark.parametrize('cls', ['RRDBNet', 'RRDB_Net'])
def test_forward_images_is_tensor2img_of_forward_tiled_many(dev, prec, cls):
    from esrganplus_amd import metrics
    net = _net(dev, 1, _wide_state_dict(), prec, cls)
    net.max_cached_plans = 16                      # three plans each of forward_tiled_many, forward_images and net(x) stay cached
    groups = F.tiled_many_passes(MIXED, 16, 4, 5)
    assert [(th, tw, S) for th, tw, S, _ in groups] == [(24, 24, 5), (13, 21, 2), (16, 16, 1)]
    rgb = _u8(31, MIXED)                                                              # R, G, B in memory
    bgr = [x.flip(2).contiguous() for x in rgb]                                       # the same pictures, B, G, R in memory
    with torch.no_grad():
        before = net.forward_tiled_many([_nchw(x).to(dev) for x in rgb], 16, 4, 5)
        t2i = [metrics.device_tensor2img(y) for y in before]                          # uint8 HWC, B, G, R
        got_bgr = net.forward_images([x.to(dev) for x in bgr], 16, 4, 5, bgr=True)
        got_rgb = net.forward_images([x.to(dev) for x in rgb], 16, 4, 5)
        ref_bgr = F.images_reference(net, [x.to(dev) for x in bgr], 16, 4, 5, bgr=True)
        ref_rgb = F.images_reference(net, [x.to(dev) for x in rgb], 16, 4, 5)
        after = net.forward_tiled_many([_nchw(x).to(dev) for x in rgb], 16, 4, 5)
    assert isinstance(got_bgr, list) and len(got_bgr) == len(got_rgb) == len(MIXED)
    vals = torch.cat([y.reshape(-1) for y in got_rgb]).cpu()
    share = [float((vals == 0).float().mean()), float((vals == 255).float().mean())]
    print('forward_images %s %s: share of 0 %.3f, of 255 %.3f' % (cls, prec, share[0], share[1]))
    assert share[0] > 0.005 and share[1] > 0.005 and share[0] + share[1] < 0.9      # both clamps and the range between
    for k, (H, W) in enumerate(MIXED):
        for y in (got_bgr[k], got_rgb[k]):
            assert y.dtype == torch.uint8 and tuple(y.shape) == (4 * H, 4 * W, 3) and y.device == dev and y.is_contiguous()
        assert _same_bits(got_bgr[k], t2i[k]), (H, W)
        assert _same_bits(got_rgb[k], t2i[k].flip(2)), (H, W)
        assert _same_bits(got_bgr[k], ref_bgr[k]) and _same_bits(got_rgb[k], ref_rgb[k]), (H, W)
        assert _same_bits(before[k], after[k])                                        # forward_tiled_many is untouched
    # ---- 4. plans: no image size and no bgr in the key; other images with the same window shapes build nothing new
    keys = _keys(net, 'tiled_img')
    assert sorted(k[:5] for k in keys) == sorted(('tiled_img', S, th, tw, prec) for th, tw, S, _ in groups)
    assert all(len(k) == 6 for k in keys)
    plans = {k: net._plans[k] for k in net._plans}
    other = [(24, 30), (70, 33), (13, 21), (25, 24), (16, 16)]                        # 24 x 24 (S = 5), 13 x 21 (2), 16 x 16 (1)
    assert [(th, tw, S) for th, tw, S, _ in F.tiled_many_passes(other, 16, 4, 5)] == [(24, 24, 5), (13, 21, 2), (16, 16, 1)]
    xs = [x.to(dev) for x in _u8(41, other)]
    with torch.no_grad():
        ys = net.forward_images(xs, 16, 4, 5, bgr=True)
        refs = F.images_reference(net, xs, 16, 4, 5, bgr=True)
    assert list(net._plans) == list(plans) and all(net._plans[k] is v for k, v in plans.items())
    assert all(_same_bits(y, r) for y, r in zip(ys, refs))


# ---- 5. mode and autograd contract ----------------------------------------------------------------------------------
def test_forward_images_ignores_train_mode_and_leaves_the_module_alone(dev):
    net = _net(dev, 1, _wide_state_dict())
    big = _u8(51, [(13, 30)])[0].to(dev)
    xs = [big[:, 4:25], _u8(52, [(16, 16)])[0].to(dev)]                               # the first is not contiguous
    assert not xs[0].is_contiguous()
    y_eval = net.forward_images(xs, 8, 2)
    assert all(_same_bits(a, b) for a, b in zip(y_eval, net.forward_images([x.contiguous() for x in xs], 8, 2)))
    net.train()
    y_train = net.forward_images(xs, 8, 2)
    assert all(_same_bits(a, b) for a, b in zip(y_train, y_eval))
    assert net.training and all(m.training for m in net.modules())
    assert all(p.requires_grad for p in net.parameters())
    assert all(y.dtype == torch.uint8 and y.device == dev and y.requires_grad is False and y.grad_fn is None for y in y_train)
    assert net.forward_images([]) == [] and net.forward_images(()) == []
    assert all(k[0] == 'tiled_img' for k in net._plans)
    n_plans = len(net._plans)
    for bad in ([xs[0].float()], [xs[0][0]], [xs[0][:, :, :2]], [xs[0][:0]], [xs[0], xs[1].cpu()], [xs[1].cpu()]):
        with pytest.raises(ValueError):
            net.forward_images(bad, 8, 2)
    for kw in (dict(tile=0), dict(pad=-1), dict(windows_per_pass=0), dict(tile=8.0)):
        with pytest.raises(ValueError, match='of a tiled forward must be an int >='):
            net.forward_images(xs, **kw)
    assert len(net._plans) == n_plans                                                 # refused before any plan


# ---- 6. pinned by the reference's own images ------------------------------------------------------------------------
@pytest.fixture(scope='module')
def model23(dev):
    from esrganplus_amd import architecture as arch
    model = arch.RRDB_Net(3, 3, 64, 23, gc=32, upscale=4, norm_type=None, act_type='leakyrelu', mode='CNA', res_scale=1,
                          upsample_mode='upconv')
    model.load_state_dict(synth.rrdbnet_state_dict(23, 0), strict=False)
    return model.eval().to(dev).set_precision('fp32')


def test_whole_images_against_the_references_uint8_results(dev, model23, golden):
    g = golden('sr_infer')
    names = [str(n) for n in g['names']]
    assert names == ['baby', 'bird', 'butterfly', 'head', 'woman']
    lr = [torch.from_numpy(g['lr_' + n]).to(dev) for n in names]
    # tile 128 >= every side, pad 0: every image is one window, the whole image
    assert all(len(ps) == 1 and S == 1 for _, _, S, ps in F.tiled_many_passes([tuple(x.shape[:2]) for x in lr], 128, 0, 16))
    with torch.no_grad():
        ys = model23.forward_images(lr, tile=128, pad=0)
    for n, y in zip(names, ys):
        got, ref = y.cpu().numpy().astype(np.int32), g['sr_' + n].astype(np.int32)
        assert got.shape == ref.shape
        d = np.abs(got - ref)
        print('%-10s %s fp32: max|diff| %d LSB, differing pixels %.4f %%' % (n, got.shape[:2], d.max(), 100 * np.mean(d > 0)))
        # the bounds of tests/test_gpu_sr_infer.py for the same comparison
        assert d.max() <= 1 and np.mean(d > 0) <= 2e-3, (n, d.max(), np.mean(d > 0))


# ---- 7. the inference script ----------------------------------------------------------------------------------------
def test_sr_infer_tile_u8_over_the_five_bundled_images(dev, model23, tmp_path, golden):
    from PIL import Image
    g = golden('sr_infer')
    names = sorted(str(n) for n in g['names'])
    in_dir, out_dir = tmp_path / 'LR', tmp_path / 'results'
    in_dir.mkdir()
    for name in names:
        Image.fromarray(g['lr_' + name]).save(str(in_dir / (name + '.png')))
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'sr_infer.py'), 'synthetic', str(in_dir), str(out_dir), 'fp32']
    r = subprocess.run(cmd + ['--tile-u8', '16,4'], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert lines == ['%d %s %s -> %s' % (k + 1, n, g['lr_' + n].shape[:2], g['sr_' + n].shape[:2]) for k, n in enumerate(names)]
    # the same in-process, in the script's flushes (images queued until they hold 4 x 16 windows)
    flushes, queue, windows = [], [], 0
    for n in names:
        queue.append(n)
        windows += -(-g['lr_' + n].shape[0] // 16) * -(-g['lr_' + n].shape[1] // 16)
        if windows >= 64:
            flushes.append(queue)
            queue, windows = [], 0
    if queue:
        flushes.append(queue)
    assert len(flushes) > 1 and sorted(n for f in flushes for n in f) == names
    for f in flushes:
        with torch.no_grad():
            ys = model23.forward_images([torch.from_numpy(g['lr_' + n]).to(dev) for n in f], 16, 4)
        for n, y in zip(f, ys):
            got = np.array(Image.open(str(out_dir / (n + '_rlt.png'))).convert('RGB'))
            assert got.shape == tuple(y.shape) and np.array_equal(got, y.cpu().numpy()), n
    r = subprocess.run(cmd + ['--tile-u8=16', '--tile-many', '16'], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and '--tile-u8' in r.stderr and 'cannot be combined' in r.stderr, r.stderr[-500:]


# ---- 8. the op's refusals -------------------------------------------------------------------------------------------
def test_tile_img_op_refusals(dev):
    from esrganplus_amd import _lib as L, engine as E
    g = E.G32(4, 3, 12, 12, 'fp16', dev)                                             # 12 x 12 windows: tile 8, pad 2
    g.t.fill_(SENTINEL)
    x = torch.full((13, 21, 3), FILL, dtype=torch.uint8, device=dev)                 # 2 x 3 tiles
    y = torch.full((52, 84, 3), FILL, dtype=torch.uint8, device=dev)
    slots = torch.full((4, 3, 48, 48), SENTINEL, device=dev)
    tables = {1: _table(dev, [(x, 13, 21, t, 1) for t in range(4)]), 0: _table(dev, [(y, 13, 21, t, 1) for t in range(4)])}
    lib = L.lib()

    def both(rc, **over):
        """The gather and the stitch refuse alike, with a message that names the entry."""
        for to_g32 in (1, 0):
            lib.esr_tile_img_op(None, None)                                          # leaves another message behind
            kw = dict(n_slots=4, C_=3, tile=8, pad=2, th=12, tw=12, g=g, slots=slots, check=False)
            kw.update(over)
            assert _op('img', to_g32, tables[to_g32], **kw) == rc, (to_g32, over)
            msg = lib.esr_last_error()
            assert msg and b'esr_tile_img_op' in msg and b'invalid arguments' not in msg, msg

    assert lib.esr_tile_img_op(None, None) == ESR_ERR_INVALID
    assert b'esr_tile_img_op' in lib.esr_last_error()
    for C_ in (2, 4, 8):
        both(ESR_ERR_UNSUPPORTED, C=C_)
    both(ESR_ERR_INVALID, tile=0)
    both(ESR_ERR_INVALID, pad=-1)
    both(ESR_ERR_INVALID, scale=2)
    both(ESR_ERR_INVALID, n_slots=0)
    both(ESR_ERR_UNSUPPORTED, n_slots=65536)
    both(ESR_ERR_UNSUPPORTED, th=65535 * 4 + 1, tile=1 << 20)                        # taller than 65535 workgroups of 4 rows
    both(ESR_ERR_INVALID, th=13)                                                     # larger than tile + 2 pad
    for to_g32 in (1, 0):
        kw = dict(n_slots=4, C_=3, tile=8, pad=2, th=12, tw=12, g=g, slots=slots, check=False)
        assert _op('img', to_g32, tables[to_g32], scale=4 if to_g32 else 1, **kw) == ESR_ERR_UNSUPPORTED
        assert b'scale' in lib.esr_last_error()                                      # the other direction's scale
        assert _op('img', to_g32, None, **kw) == ESR_ERR_INVALID
        assert _op('img', to_g32, tables[to_g32], **dict(kw, th=0)) == ESR_ERR_INVALID
        assert _op('img', to_g32, tables[to_g32], dtype=7, **kw) == ESR_ERR_INVALID
        assert b'esr_tile_img_op' in lib.esr_last_error()
    kw = dict(n_slots=4, C_=3, tile=8, pad=2, check=False)
    assert _op('img', 1, tables[1], th=12, tw=12, slots=slots, **kw) == ESR_ERR_INVALID              # the gather without a G32 view
    assert _op('img', 0, tables[0], th=12, tw=12, g=g, **kw) == ESR_ERR_INVALID                      # the stitch without slots
    assert _op('img', 1, tables[1], th=12, tw=40, g=g, tile=40, pad=0, n_slots=4, C_=3, check=False) == ESR_ERR_INVALID
    assert b'narrower' in lib.esr_last_error()                                                       # a 40-wide window in a 12-wide view
    assert _op('img', 0, tables[0], th=12, tw=12, slots=slots, slots_nchw=slots.data_ptr() + 4, **kw) == ESR_ERR_INVALID
    assert b'aligned' in lib.esr_last_error() and b'esr_tile_img_op' in lib.esr_last_error()
    torch.cuda.synchronize()
    assert bool((g.t == SENTINEL).all()) and bool((slots == SENTINEL).all())         # nothing was launched
    assert bool((x == FILL).all()) and bool((y == FILL).all())
