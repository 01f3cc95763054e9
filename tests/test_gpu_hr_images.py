"""Scoring a generator from HR images alone, on the GPU: the gather that makes the LR window out of the 8-bit HR image
(csrc/tile_img.hip, esr_tile_hr) bit for bit against crops of ``data.imresize`` of the float image and within 2e-6 of the
reference dataset's LR (tests/golden/hr_val.npz); ``forward_hr_images`` against ``device_tensor2img`` of
``forward_tiled_many`` on that LR and against ``hr_images_reference``; ``evaluate_hr_images``; ``PSNRStep.validate_hr``;
``tools/sr_eval.py`` on an HR folder."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from esrganplus_amd import data as D
from esrganplus_amd import functional as F
from esrganplus_amd import metrics as M
from esrganplus_amd import synth
from tests.test_gpu_conv_backward import upload
from tests.test_gpu_far_views import END_FAMS, arena, far_runs, same_as_compact  # noqa: F401
from tests.test_gpu_images import _keys, _net, _same_bits, _wide_state_dict
from tests.test_gpu_set_metrics import _close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -77.25                              # exact in fp16 and fp32
SIZES = [(55, 86), (52, 240), (64, 64)]        # HR; LR 13 x 21 (both sides cut by modcrop), 13 x 60, 16 x 16
LR_SIZES = [(h // 4, w // 4) for h, w in SIZES]
LUT = torch.arange(256, dtype=torch.float32) / 255.0       # the 256 quotients, divided on the CPU (a true division)
# (images, tile, pad, slots per pass): the three images in one set — windows of 13 x 14 (22 of them: the last of five
# passes holds three filler slots) and 14 x 14, partial 16-tiles both; the 13 x 60 image with windows of 13 x 20: two LDS
# tiles along x, and the first source column of tiles 1 ... 3 is not 0
GATHER_CASES = [((0, 1, 2), 8, 3, 5), ((1,), 16, 2, 5)]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def hr_set(dev, golden):
    """The fixture's images (uint8 HWC, B, G, R) on the device, the dataset's LR (CPU, R, G, B), and per channel order of
    the bytes the float LR ``data.imresize`` makes on the device of the modcropped float image (slot channel 0 first);
    computed once."""
    g = golden('hr_val')
    bgr = [torch.from_numpy(g['img%d' % k]).to(dev) for k in range(3)]
    assert [tuple(x.shape[:2]) for x in bgr] == SIZES
    imgs = {1: bgr, 0: [x.flip(2).contiguous() for x in bgr]}                  # 0: the same pictures, R, G, B in memory
    lut = LUT.to(dev)
    floats = [lut[D.modcrop(x.flip(2).permute(2, 0, 1), 4).long()].contiguous() for x in bgr]      # R, G, B planes
    whole = [D.imresize(f, 0.25) for f in floats]
    torch.cuda.synchronize()
    assert [tuple(w.shape[1:]) for w in whole] == LR_SIZES
    return dict(imgs=imgs, floats=floats, whole=whole, lr=[torch.from_numpy(g['LR%d' % k]) for k in range(3)])


def _hr_tables(dev, x, H, W):
    (wy, iy, _), (wx, ix, _) = D.device_tables(4 * H, 0.25, dev), D.device_tables(4 * W, 0.25, dev)
    return wy, iy, wx, ix


def _hr_table(dev, images, entries):
    """[(image index, t, live)] over uint8 HR device images -> (uint8 device tensor: the 24-byte items, then one 64-byte
    descriptor per image, which the items name; what must stay alive)."""
    items = np.zeros(len(entries), dtype=F._tile_item_dtype())
    desc = np.zeros(len(images), dtype=F._hr_desc_dtype())
    keep = []
    for i, x in enumerate(images):
        H, W = x.shape[0] // 4, x.shape[1] // 4
        wy, iy, wx, ix = _hr_tables(dev, x, H, W)
        keep.append((x, wy, iy, wx, ix))
        assert x.is_contiguous()
        desc[i] = (x.data_ptr(), wy.data_ptr(), iy.data_ptr(), wx.data_ptr(), ix.data_ptr(), x.shape[1], 4 * H, 4 * W,
                   wy.shape[1], wx.shape[1], 0)
    table = torch.empty(items.nbytes + desc.nbytes, dtype=torch.uint8, device=dev)
    for k, (i, t, live) in enumerate(entries):
        items[k] = (table.data_ptr() + items.nbytes + 64 * i, images[i].shape[0] // 4, images[i].shape[1] // 4, t, live)
    table.copy_(torch.from_numpy(np.concatenate([items.view(np.uint8), desc.view(np.uint8)])))
    return table, keep


def _hr_op(table, n_slots, tile, pad, th, tw, g, bgr, check=True, over=None):
    from esrganplus_amd import _lib as L, engine as E
    d = L.esr_tile_hr()
    d.dtype, d.to_g32, d.C, d.tile, d.pad, d.scale = g.esr_dtype, 1, 3, tile, pad, 1
    d.th, d.tw, d.n_slots, d.bgr = th, tw, n_slots, bgr
    d.items = table.data_ptr()
    d.g32 = g.view(0, 3)
    for k, v in (over or {}).items():
        setattr(d, k, v)
    rc = L.lib().esr_tile_hr_op(C.byref(d), C.c_void_p(E.current_stream()))
    if check:
        L.check(rc, 'esr_tile_hr_op')
    return rc, d


# ---- 1. the gather alone, through the C ABI --------------------------------------------------------------------------
@pytest.mark.parametrize('bgr', [0, 1])
@pytest.mark.parametrize('prec', ['fp16', 'fp32'])
def test_gather_is_the_crop_of_imresize_of_the_float_image(dev, hr_set, prec, bgr):
    """Every slot, the whole buffer byte for byte: the window's crop of ``data.imresize(float_hr, 0.25)`` converted to
    the dtype (the layout kernel's conversion), channels >= 3 zero, halo and padding still the sentinel.  Against the
    dataset's LR: 2e-6 in fp32 — the bound of the generated LR of batch_assemble.npz — and in fp16 that plus the
    rounding of the conversion, 2^-11 of the value."""
    from esrganplus_amd import engine as E
    imgs, whole, lr_ref = hr_set['imgs'][bgr], hr_set['whole'], hr_set['lr']
    corners, shapes, first_cols, worst = set(), set(), set(), 0.0
    for members, tile, pad, S in GATHER_CASES:
        sizes = [LR_SIZES[i] for i in members]
        geo = [F.tiled_geometry(H, W, tile, pad) for H, W in sizes]
        groups = F.tiled_many_passes(sizes, tile, pad, S)
        for th, tw, Sg, passes in groups:
            shapes.add((th, tw))
            for p in passes:
                ref, got = (E.G32(Sg, 3, th, tw, prec, dev) for _ in range(2))
                ref.t.fill_(SENTINEL)
                got.t.fill_(SENTINEL)
                crops = []
                for i, t, live in p:
                    wy, wx = geo[i][4][t][4:6]
                    H, W = sizes[i]
                    corners |= {('top', wy == 0), ('bottom', wy == H - th), ('left', wx == 0), ('right', wx == W - tw)}
                    first_cols.add(wx)
                    crops.append(whole[members[i]][None, :, wy:wy + th, wx:wx + tw])
                want = torch.cat(crops, 0).contiguous()
                upload(ref, want)
                table, keep = _hr_table(dev, [imgs[m] for m in members], p)
                _hr_op(table, Sg, tile, pad, th, tw, got, bgr)
                torch.cuda.synchronize()
                assert _same_bits(got.t, ref.t), (members, tile, p)
                inner = got.t[:, 0, 1:th + 1, 1:tw + 1].float().cpu()
                assert not bool((inner[..., :3] == SENTINEL).any()) and bool((inner[..., 3:] == 0).all())
                assert bool((got.t[:, :, 0] == SENTINEL).all()) and bool((got.t[:, :, :, 0] == SENTINEL).all())
                assert bool((got.t[:, :, th + 1:] == SENTINEL).all()) and bool((got.t[:, :, :, tw + 1:] == SENTINEL).all())
                for s, (i, t, live) in enumerate(p):
                    wy, wx = geo[i][4][t][4:6]
                    gold = lr_ref[members[i]][:, wy:wy + th, wx:wx + tw].permute(1, 2, 0)
                    err = (inner[s, :, :, :3] - gold).abs() - ((gold.abs() + 2e-6) * 2.0 ** -11 if prec == 'fp16' else 0.0)
                    worst = max(worst, float(err.max()))
    print('esr_tile_hr gather %s bgr=%d: worst excess over the dataset LR %.3e (bound 2e-6)' % (prec, bgr, worst))
    assert worst <= 2e-6
    assert shapes == {(13, 14), (14, 14), (13, 20)}                            # partial 16-tiles; two LDS tiles along x
    assert {c for c in corners if c[1]} == {('top', True), ('bottom', True), ('left', True), ('right', True)}
    assert max(first_cols) >= 30                                               # a window whose first source column is far from 0


def test_gather_reads_a_modcropped_image_through_its_pitch(dev, hr_set):
    """The 55 x 86 image is handed over whole: hr_h x hr_w = 52 x 84 under a pitch of 86 pixels.  The same bytes come
    out of a contiguous cropped copy, and the last row and columns are never read: poisoning them changes nothing."""
    from esrganplus_amd import engine as E
    x = hr_set['imgs'][1][0]
    assert tuple(x.shape) == (55, 86, 3)
    th, tw, ny, nx, tiles = F.tiled_geometry(13, 21, 8, 3)
    p = [(0, t, 1) for t in range(ny * nx)]
    outs = []
    poisoned = x.clone()
    poisoned[52:] = 255 - poisoned[52:]
    poisoned[:, 84:] = 255 - poisoned[:, 84:]
    for img in (x, x[:52, :84].contiguous(), poisoned):
        got = E.G32(len(p), 3, th, tw, 'fp32', dev)
        got.t.fill_(SENTINEL)
        table, keep = _hr_table(dev, [img], p)
        rc, d = _hr_op(table, len(p), 8, 3, th, tw, got, 1)
        torch.cuda.synchronize()
        outs.append(got.t.clone())
    assert _same_bits(outs[0], outs[1]) and _same_bits(outs[0], outs[2])
    assert not bool((outs[0][:, 0, 1:th + 1, 1:tw + 1, :3] == SENTINEL).any())


def test_tile_hr_op_refusals(dev, hr_set):
    from esrganplus_amd import _lib as L, engine as E
    lib = L.lib()
    got = E.G32(2, 3, 12, 12, 'fp32', dev)
    got.t.fill_(SENTINEL)
    table, keep = _hr_table(dev, [hr_set['imgs'][1][2]], [(0, 0, 1), (0, 1, 1)])
    for over, rc_want, word in ((dict(C=1), -3, 'C = 1'), (dict(C=4), -3, 'C = 4'), (dict(scale=4), -3, 'scale 1'),
                                (dict(scale=2), -1, 'scale = 2'), (dict(tile=0), -1, 'tile = 0'), (dict(pad=-1), -1, 'pad = -1'),
                                (dict(n_slots=0), -1, 'n_slots'), (dict(n_slots=70000), -3, 'n_slots'),
                                (dict(th=13), -1, 'larger than'), (dict(items=None), -1, 'invalid arguments'),
                                (dict(dtype=7), -1, 'invalid arguments'), (dict(to_g32=0), -1, 'invalid arguments')):
        rc, _ = _hr_op(table, 2, 8, 2, 12, 12, got, 1, check=False, over=over)
        msg = lib.esr_last_error()
        assert rc == rc_want and b'esr_tile_hr_op' in msg and word.encode() in msg, (over, rc, msg)
    assert lib.esr_tile_hr_op(None, None) == -1 and b'esr_tile_hr_op' in lib.esr_last_error()
    rc, d = _hr_op(table, 2, 8, 2, 12, 12, got, 1, check=False)
    d.items = table.data_ptr() + 4
    assert lib.esr_tile_hr_op(C.byref(d), C.c_void_p(E.current_stream())) == -1 and b'8-byte alignment' in lib.esr_last_error()
    torch.cuda.synchronize()
    assert lib.esr_abi_version() == 6


@pytest.mark.parametrize('prec', ['fp16', 'fp32'])
def test_gather_on_far_slots(dev, arena, hr_set, prec):
    """The gather's G32 writes with the slot view far, as tests/test_gpu_far_views.py holds every other G32 writer: three
    slots of 12 x 12 windows of the 64 x 64 image (the last a filler); the far batch puts slot 1 past 2^31 and slot 2
    past 2^32, the near-limit plane stretches the rows.  Bit-identical to the compact run, no byte outside the windows
    moves."""
    from esrganplus_amd import _lib as L, engine as E
    from tests import far_views as FV
    x, whole = hr_set['imgs'][1][2], hr_set['whole'][2]
    th, tw, ny, nx, tiles = F.tiled_geometry(16, 16, 8, 2)
    assert (th, tw, ny * nx) == (12, 12, 4)
    p = [(0, 0, 1), (0, 3, 1), (0, 2, 0)]
    got, ref = (E.G32(3, 3, th, tw, prec, dev) for _ in range(2))
    got.t.fill_(SENTINEL)
    ref.t.fill_(SENTINEL)
    upload(ref, torch.cat([whole[None, :, tiles[t][4]:tiles[t][4] + th, tiles[t][5]:tiles[t][5] + tw] for _, t, _ in p], 0).contiguous())
    table, keep = _hr_table(dev, [x], p)
    pre = [got.t.clone()]
    rc, d = _hr_op(table, 3, 8, 2, th, tw, got, 1)
    torch.cuda.synchronize()
    assert _same_bits(got.t, ref.t)
    post = [got.t.clone()]
    call = lambda op: (L.check(L.lib().esr_tile_hr_op(C.byref(op), C.c_void_p(E.current_stream())), 'esr_tile_hr_op'),
                       torch.cuda.synchronize())
    for fam, rel in far_runs(arena, d, [got], pre, END_FAMS, lambda rel: call(rel.op), expect=[(3, 1) + FV.g32_dims(th, tw)]):
        assert torch.equal(got.t, post[0])
        same_as_compact(arena, rel, post, 'tile_hr %s' % fam)


# ---- 2. forward_hr_images --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', ['fp32', 'fp16'])
@pytest.mark.parametrize('cls', ['RRDBNet', 'RRDB_Net'])
def test_forward_hr_images_is_forward_images_of_the_dataset_lr(dev, hr_set, prec, cls):
    from esrganplus_amd import engine as E
    net = _net(dev, 1, _wide_state_dict(), prec, cls)
    net.max_cached_plans = 16
    groups = F.tiled_many_passes(LR_SIZES, 8, 3, 5)
    assert [(th, tw, S) for th, tw, S, _ in groups] == [(13, 14, 5), (14, 14, 4)]
    bgr, rgb, whole = hr_set['imgs'][1], hr_set['imgs'][0], hr_set['whole']
    with torch.no_grad():
        t2i = [M.device_tensor2img(y) for y in net.forward_tiled_many(whole, 8, 3, 5)]       # uint8 HWC, B, G, R
        got_bgr = net.forward_hr_images(bgr, 8, 3, 5, bgr=True)
        got_rgb = net.forward_hr_images(rgb, 8, 3, 5)
        ref_bgr = F.hr_images_reference(net, bgr, 8, 3, 5, bgr=True)
        ref_rgb = F.hr_images_reference(net, rgb, 8, 3, 5)
        again = net.forward_hr_images(bgr, 8, 3, 5, bgr=True)
        alone = net.forward_hr_images([bgr[1]], 8, 3, 5, bgr=True)
        keys = _keys(net, 'tiled_hr')
        # the whole-image route: a tile as large as the largest side makes every window an image
        one = net.forward_hr_images(bgr, 60, 0, bgr=True)
        plain = [M.device_tensor2img(net(w[None])) for w in whole]
    lr_ref, _ = F.hr_lr_reference(bgr, bgr=True)
    diff = [int((a != b).sum()) for a, b in zip(lr_ref, whole)]
    flips = [int((a != b).sum()) for a, b in zip(got_bgr, ref_bgr)]
    print('forward_hr_images %s %s: LR values where hr_lr_reference and data.imresize differ %s of %s; result bytes that '
          'differ from hr_images_reference %s' % (cls, prec, diff, [w.numel() for w in whole], flips))
    vals = torch.cat([y.reshape(-1) for y in got_rgb]).cpu()
    share = [float((vals == 0).float().mean()), float((vals == 255).float().mean())]
    print('share of 0 %.3f, of 255 %.3f' % (share[0], share[1]))
    assert share[0] + share[1] < 0.9 and len(torch.unique(vals)) > 100               # pictures, not a clamped plane
    assert diff == [0, 0, 0]                                     # the restatement's LR has data.imresize's bits
    for k, (H, W) in enumerate(SIZES):
        for y in (got_bgr[k], got_rgb[k]):
            assert y.dtype == torch.uint8 and tuple(y.shape) == (4 * (H // 4), 4 * (W // 4), 3) and y.device == dev
            assert y.is_contiguous() and not y.requires_grad
        assert _same_bits(got_bgr[k], t2i[k]), (H, W)
        assert _same_bits(got_rgb[k], t2i[k].flip(2)), (H, W)
        assert _same_bits(again[k], got_bgr[k])                                       # two calls, the same bytes
        assert _same_bits(one[k], plain[k]), (H, W)
    assert _same_bits(alone[0], got_bgr[1])                                           # alone and in a set
    # one plan per window shape: no image size and no bgr in the key
    assert sorted(k[:5] for k in keys) == sorted(('tiled_hr', S, th, tw, prec) for th, tw, S, _ in groups)
    assert all(len(k) == 6 for k in keys)
    for k in range(3):
        assert _same_bits(got_bgr[k], ref_bgr[k]) and _same_bits(got_rgb[k], ref_rgb[k]), (k, flips)
    # more calls than pinned tables, nothing synchronises in between: every call's table reaches its launches intact
    torch.cuda.synchronize()
    plans = list(net._plans)
    with torch.no_grad():
        outs = [net.forward_hr_images(bgr[k % 3:] + bgr[:k % 3], 8, 3, 5, bgr=True) for k in range(E.PinnedRing().n + 2)]
    torch.cuda.synchronize()
    for k, ys in enumerate(outs):
        assert all(_same_bits(y, got_bgr[(k + j) % 3]) for j, y in enumerate(ys))
    assert list(net._plans) == plans                                                  # any order of the set: the same two plans


def test_forward_hr_images_ignores_train_mode_and_refuses_before_a_plan(dev, hr_set):
    net = _net(dev, 1, _wide_state_dict())
    xs = hr_set['imgs'][0]
    wide = torch.cat([xs[2], xs[2]], 1)[:, 10:74]                                     # not contiguous
    assert not wide.is_contiguous()
    y_eval = net.forward_hr_images([xs[0], wide], 8, 3)
    assert _same_bits(y_eval[1], net.forward_hr_images([wide.contiguous()], 8, 3)[0])
    net.train()
    y_train = net.forward_hr_images([xs[0], wide], 8, 3)
    assert all(_same_bits(a, b) for a, b in zip(y_train, y_eval))
    assert net.training and all(p.requires_grad for p in net.parameters())
    assert all(k[0] == 'tiled_hr' for k in net._plans)
    n_plans = len(net._plans)
    for bad in ([xs[0].float()], [xs[0][:3]], [xs[0], xs[1].cpu()], [xs[1].cpu()], [xs[0][:, :, :2]]):
        with pytest.raises(ValueError):
            net.forward_hr_images(bad, 8, 3)
    with pytest.raises(TypeError):
        net.forward_hr_images(xs, 8, 3, x8=True)
    assert len(net._plans) == n_plans and net.forward_hr_images([]) == []


# ---- 3. evaluate_hr_images -------------------------------------------------------------------------------------------
def test_evaluate_hr_images_is_the_set_metric_of_the_route(dev, hr_set):
    net = _net(dev, 1, _wide_state_dict())
    bgr, whole = hr_set['imgs'][1], hr_set['whole']
    cropped = [x[:x.shape[0] - x.shape[0] % 4, :x.shape[1] - x.shape[1] % 4].contiguous() for x in bgr]
    with torch.no_grad():
        sr, res = net.evaluate_hr_images(bgr, 8, 3, 5, bgr=True)
        plain = net.forward_hr_images(bgr, 8, 3, 5, bgr=True)
    assert len(sr) == 3 and all(_same_bits(a, b) for a, b in zip(sr, plain)) and res.crop == 4
    table = res.read()
    assert table.shape == (3, 4) and np.isfinite(table).all()
    want = M.device_set_metrics(sr, cropped, 4, True).read()
    assert np.array_equal(table, want)                                                # bit for bit
    assert _close(table, M.set_metrics_reference([x.cpu() for x in sr], [x.cpu() for x in cropped], 4, bgr=True), 1e-9)
    # another crop, the other channel order
    _, res6 = net.evaluate_hr_images(hr_set['imgs'][0], 8, 3, 5, crop=6)
    sr_rgb = net.forward_hr_images(hr_set['imgs'][0], 8, 3, 5)
    assert _close(res6.read(), M.set_metrics_reference([x.cpu() for x in sr_rgb], [x.flip(2).cpu() for x in cropped], 6), 1e-9)
    # stored 8-bit LR files are another input: the paired route on the rounded resample gives other numbers
    lr8 = [M.device_tensor2img(w) for w in whole]                                     # uint8 HWC, B, G, R
    assert [tuple(x.shape[:2]) for x in lr8] == LR_SIZES
    with torch.no_grad():
        sr8, res8 = net.evaluate_images(lr8, cropped, 8, 3, 5, bgr=True)
    print('evaluate_hr_images averages %s; evaluate_images on the rounded LR %s' % (res.averages(), res8.averages()))
    assert any(not _same_bits(a, b) for a, b in zip(sr, sr8))
    assert not np.array_equal(res8.read(), table)
    for bad in (dict(crop=-1), dict(crop=26), dict(crop=2.5)):
        with pytest.raises(ValueError, match='crop'):
            net.evaluate_hr_images(bgr, 8, 3, 5, **bad)


# ---- 4. PSNRStep.validate_hr -----------------------------------------------------------------------------------------
def test_psnr_step_validate_hr_between_steps(dev, hr_set):
    from esrganplus_amd import architecture as arch, train
    netG = arch.RRDBNet(3, 3, 64, 1).to(dev).train().set_precision('fp32')
    netG.load_state_dict(synth.rrdbnet_state_dict(nb=1, seed=82), strict=True)
    st = train.PSNRStep(netG)
    batch = lambda i: (synth.image_batch(400 + i, 2, 3, 12, 12, name='val.lr').to(dev),
                       synth.image_batch(410 + i, 2, 3, 48, 48, name='val.hr').to(dev))
    for i in range(2):
        torch.manual_seed(6000 + i)
        st.step(*batch(i), sync_log=False)
    hr = hr_set['imgs'][0]
    psnr = st.validate_hr(hr, tile=8, pad=3, windows_per_pass=5)
    table = st.val_result.read()
    assert isinstance(psnr, float) and table.shape == (3, 4)
    assert psnr == st.val_result.averages()[0] == sum(float(v) for v in table[:, 0]) / 3
    assert netG.training and all(p.requires_grad for p in netG.parameters())          # as validate leaves it
    sr = netG.forward_hr_images(hr, tile=8, pad=3, windows_per_pass=5)
    cropped = [x[:x.shape[0] - x.shape[0] % 4, :x.shape[1] - x.shape[1] % 4].contiguous() for x in hr]
    assert _close(table, M.set_metrics_reference([x.cpu() for x in sr], [x.cpu() for x in cropped], 4), 1e-9)
    torch.manual_seed(6002)
    log = st.step(*batch(2))
    assert np.isfinite(log['l_pix'])


# ---- 5. tools/sr_eval.py on an HR folder -----------------------------------------------------------------------------
def test_sr_eval_on_an_hr_folder(dev, hr_set, tmp_path):
    from PIL import Image
    from esrganplus_amd import architecture as arch
    rgb = hr_set['imgs'][0]
    for k, x in enumerate(rgb):
        Image.fromarray(x.cpu().numpy()).save(str(tmp_path / ('im%d.png' % k)))
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'sr_eval.py'), 'synthetic', str(tmp_path), 'fp32',
                          '--tile-u8', '8,3', '--nb', '1'], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert sum(' - PSNR: ' in l for l in lines) == 3
    m = re.search(r'PSNR: ([-\d.]+) dB; SSIM: ([-\d.]+)\n\n.*\n\tPSNR_Y: ([-\d.]+) dB; SSIM_Y: ([-\d.]+)', out.stdout)
    assert m, out.stdout
    model = arch.RRDB_Net(3, 3, 64, 1, gc=32, upscale=4, norm_type=None, act_type='leakyrelu', mode='CNA', res_scale=1,
                          upsample_mode='upconv')
    model.load_state_dict(synth.rrdbnet_state_dict(1, 0), strict=False)
    model = model.eval().to(dev).set_precision('fp32')
    with torch.no_grad():
        ave = model.evaluate_hr_images(rgb, 8, 3)[1].averages()
    assert [m.group(i + 1) for i in range(4)] == ['{:.6f}'.format(v) for v in ave]
