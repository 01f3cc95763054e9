"""esr_image_set_metrics (csrc/metrics_set.hip) and the layers above it — metrics.device_set_metrics,
RRDBNet.evaluate_images, PSNRStep.validate — on the device: against the reference's own values (tests/golden/ssim.npz,
metrics_y.npz), against the host restatement ``metrics.set_metrics_reference`` on a set of the smallest sizes at which
tiling (16 x 32 tiles), halo, crop and the two-stage reduction can go wrong, bit for bit against itself, and against the
per-pair kernel ``device_psnr_ssim``."""
import ctypes

import numpy as np
import pytest
import torch

from esrganplus_amd import metrics as M
from esrganplus_amd import synth
from tests.test_set_metrics_host import COL, golden_pairs

pytestmark = pytest.mark.gpu

ESR_ERR_INVALID = -1
# (H, W) of the mixed set at crop 4: 19 x 19 -> 11 x 11, exactly one SSIM output; 18 x 40 -> cropped height 10, no SSIM;
# 9 x 9 -> one pixel; 33 x 47 and 30 x 27: rows of 3 W bytes that are no multiple of 4; 150 x 203: more than one tile
# both ways with ragged edges; 64 x 64 is the sr == hr pair
MIXED = [(19, 19), (18, 40), (9, 9), (33, 47), (30, 27), (150, 203), (64, 64)]
CROP = 4


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _pair(seed, h, w):
    """tests/test_gpu_metrics.py's pair: noise, out-of-range values and .5/255 steps in front of tensor2img."""
    hr = synth.image_batch(seed, 1, 3, h, w, name='setmet.hr')[0]
    sr = (hr + 0.08 * synth.normal_like(seed + 1, 'setmet.n', (3, h, w))).mul(255).round().div(255) + 0.5 / 255
    sr[0, 0, :3] = torch.tensor([-0.2, 1.3, 0.5])
    return sr, hr


@pytest.fixture(scope='module')
def mixed():
    """The mixed set as uint8 HWC arrays (sr, hr) and its host numbers for bgr True / False; computed once."""
    sr, hr = [], []
    for i, (h, w) in enumerate(MIXED):
        s, t = _pair(300 + 2 * i, h, w)
        b = M.tensor2img(t)
        sr.append(b.copy() if (h, w) == (64, 64) else M.tensor2img(s))
        hr.append(b)
    want = {bgr: M.set_metrics_reference(sr, hr, CROP, bgr=bgr) for bgr in (True, False)}
    return sr, hr, want


def _dev(arrays, dev):
    return [torch.from_numpy(a).to(dev) for a in arrays]


def _close(got, want, tol):
    """|got - want| <= tol where both are finite; inf and nan must sit in the same places."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want)), (got, want)
    err = np.abs(got[fin] - want[fin]).max() if fin.any() else 0.0
    print('largest difference %.3e (bound %.1e)' % (err, tol))
    return err <= tol


def test_goldens_one_call_per_crop(dev):
    pairs = [(p, ('ssim', 'ssim_y')) for p in golden_pairs('ssim')] + [(p, ('psnr', 'psnr_y')) for p in golden_pairs('mety')]
    assert sorted((p[0].shape[:2], p[2]) for p, _ in pairs[:4]) == sorted([((40, 52), 4), ((33, 47), 2), ((128, 96), 4), ((30, 27), 0)])
    for crop in sorted({p[2] for p, _ in pairs}):
        sel = [(p, keys) for p, keys in pairs if p[2] == crop]
        got = M.device_set_metrics(_dev([p[0] for p, _ in sel], dev), _dev([p[1] for p, _ in sel], dev), crop, bgr=True).read()
        for row, (p, keys) in zip(got, sel):
            for k in keys:
                err = abs(row[COL[k]] - p[3][k])
                print('crop %d %s %s: %.3e' % (crop, p[0].shape[:2], k, err))
                assert err <= (1e-7 if k == 'psnr_y' else 1e-9), (crop, p[0].shape, k, row[COL[k]], p[3][k])
            if 'ssim' in keys:                      # the ssim goldens' PSNR columns against the host restatement
                assert _close(row, M.set_metrics_reference([p[0]], [p[1]], crop, bgr=True)[0], 1e-9)


@pytest.mark.parametrize('bgr', [True, False])
def test_mixed_set_matches_the_host_restatement(dev, mixed, bgr):
    sr, hr, want = mixed
    got = M.device_set_metrics(_dev(sr, dev), _dev(hr, dev), CROP, bgr=bgr).read()
    w = want[bgr]
    assert np.isnan(w[1, 1]) and np.isnan(w[1, 3]) and np.isfinite(w[1, 0])          # 18 x 40: no SSIM, a PSNR
    assert np.isnan(w[2, 1]) and np.isfinite(w[2, 0])                                # 9 x 9: one pixel
    assert np.isinf(w[6, 0]) and np.isinf(w[6, 2])                                   # sr == hr
    assert _close(got, w, 1e-9)
    assert got[6, 0] == float('inf') and got[6, 2] == float('inf')
    assert abs(got[6, 1] - 1.0) <= 1e-12 and abs(got[6, 3] - 1.0) <= 1e-12


def test_sums_are_bit_identical_across_calls_sets_and_table_positions(dev, mixed):
    sr, hr, _ = mixed
    a, b = _dev(sr, dev), _dev(hr, dev)
    first = M.device_set_metrics(a, b, CROP, bgr=True).sums
    again = M.device_set_metrics(a, b, CROP, bgr=True).sums
    assert first.dtype == torch.float64 and first.shape == (len(sr), 4)
    assert torch.equal(first, again)
    for i in range(len(sr)):
        alone = M.device_set_metrics([a[i]], [b[i]], CROP, bgr=True).sums
        assert torch.equal(alone[0], first[i]), i
    j = len(sr) - 1 - 5                                                      # the 150 x 203 pair at another place, other neighbours
    moved = M.device_set_metrics(a[::-1], b[::-1], CROP, bgr=True).sums
    assert torch.equal(moved[j], first[5]) and torch.equal(moved.flip(0), first)


def test_agrees_with_the_per_pair_kernel(dev):
    hr = synth.image_batch(92, 1, 3, 128, 96, name='ssim.hr')[0]
    sr = hr + 0.06 * synth.normal_like(92, 'ssim.n', (3, 128, 96))
    got = M.device_set_metrics(_dev([M.tensor2img(sr)], dev), _dev([M.tensor2img(hr)], dev), 4, bgr=True).read()[0]
    psnr, ssim = M.device_psnr_ssim(sr.to(dev), hr.to(dev), crop=4)
    psnr_y, ssim_y = M.device_psnr_ssim(sr.to(dev), hr.to(dev), crop=4, y_only=True)
    assert _close(got, [psnr, ssim, psnr_y, ssim_y], 1e-9)


def test_two_queued_calls_do_not_disturb_each_other_or_their_inputs(dev, mixed):
    sr, hr, want = mixed
    a, b = _dev(sr, dev), _dev(hr, dev)
    keep = [x.clone() for x in a + b]
    r1 = M.device_set_metrics(a[:4], b[:4], CROP, bgr=True)
    r2 = M.device_set_metrics(a[3:], b[3:], CROP, bgr=False)              # queued before r1 is read
    assert _close(r1.read(), want[True][:4], 1e-9)
    assert _close(r2.read(), want[False][3:], 1e-9)
    assert all(torch.equal(x, k) for x, k in zip(a + b, keep))
    avg = r1.averages()
    assert avg[0] == sum(float(v) for v in r1.read()[:, 0]) / 4 and np.isnan(avg[1])


def test_c_entry_refuses_bad_arguments(dev):
    from esrganplus_amd import _lib as L
    lib = L.lib()
    assert lib.esr_image_set_metrics(None, None) == ESR_ERR_INVALID
    assert b'esr_image_set_metrics' in lib.esr_last_error()
    img = torch.zeros((20, 24, 3), dtype=torch.uint8, device=dev)
    item = L.esr_set_metrics_item(img.data_ptr(), img.data_ptr(), 20, 24, 0, 0)
    table = torch.frombuffer(bytearray(bytes(item)), dtype=torch.uint8).to(dev)
    out = torch.full((4,), -7.0, dtype=torch.float64, device=dev)
    scratch = torch.empty(4, dtype=torch.float64, device=dev)
    sizes = (ctypes.c_int32 * 2)(20, 24)

    def call(**kw):
        p = L.esr_set_metrics()
        p.n, p.crop, p.bgr, p.n_units = 1, 4, 1, 1
        p.items, p.sizes_host, p.out, p.scratch = table.data_ptr(), ctypes.addressof(sizes), out.data_ptr(), scratch.data_ptr()
        for k, v in kw.items():
            setattr(p, k, v)
        rc = lib.esr_image_set_metrics(p, None)
        return rc, lib.esr_last_error()

    for kw in (dict(n=0), dict(n=-2), dict(crop=-1), dict(crop=10), dict(crop=12), dict(items=None), dict(out=None),
               dict(scratch=None), dict(sizes_host=None), dict(n_units=2)):
        rc, msg = call(**kw)
        assert rc == ESR_ERR_INVALID and b'esr_image_set_metrics' in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())                                         # nothing was launched
    rc, _ = call()
    assert rc == 0
    torch.cuda.synchronize()
    o = out.tolist()                                                         # equal images: SSIM 1 at each of 2 x 6 positions
    assert o[:3] == [0.0, 0.0, 36.0] and abs(o[3] - 12.0) <= 1e-12, o


def _u8(h, w, seed, dev):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)).to(dev)


def test_evaluate_images_is_forward_images_plus_the_set_metric(dev):
    from esrganplus_amd import architecture as arch
    net = arch.RRDBNet(3, 3, 64, 1).to(dev).eval()
    net.load_state_dict(synth.rrdbnet_state_dict(nb=1, seed=81), strict=True)
    net.set_precision('fp32')
    lr = [_u8(24, 31, 1, dev), _u8(40, 40, 2, dev)]
    hr = [_u8(96, 124, 3, dev), _u8(160, 160, 4, dev)]
    sr, res = net.evaluate_images(lr, hr, tile=16, pad=8)
    plain = net.forward_images(lr, tile=16, pad=8)
    assert len(sr) == 2 and all(torch.equal(a, b) for a, b in zip(sr, plain))
    want = M.set_metrics_reference([x.cpu() for x in sr], [x.cpu() for x in hr], 4, bgr=False)
    assert res.crop == 4 and _close(res.read(), want, 1e-9)
    _, res_bgr = net.evaluate_images(lr, hr, tile=16, pad=8, bgr=True, crop=6)
    sr_bgr = net.forward_images(lr, tile=16, pad=8, bgr=True)
    assert _close(res_bgr.read(), M.set_metrics_reference([x.cpu() for x in sr_bgr], [x.cpu() for x in hr], 6, bgr=True), 1e-9)


def test_psnr_step_validate_between_steps(dev):
    from esrganplus_amd import architecture as arch, train
    netG = arch.RRDBNet(3, 3, 64, 1).to(dev).train().set_precision('fp32')
    netG.load_state_dict(synth.rrdbnet_state_dict(nb=1, seed=82), strict=True)
    st = train.PSNRStep(netG)
    batch = lambda i: (synth.image_batch(400 + i, 2, 3, 12, 12, name='val.lr').to(dev),
                       synth.image_batch(410 + i, 2, 3, 48, 48, name='val.hr').to(dev))
    for i in range(2):
        torch.manual_seed(6000 + i)
        st.step(*batch(i), sync_log=False)
    lr = [_u8(12, 17, 5, dev), _u8(20, 20, 6, dev)]
    hr = [_u8(48, 68, 7, dev), _u8(80, 80, 8, dev)]
    psnr = st.validate(lr, hr, tile=16, pad=8)
    table = st.val_result.read()
    assert isinstance(psnr, float) and table.shape == (2, 4)
    assert psnr == (float(table[0, 0]) + float(table[1, 0])) / 2
    assert netG.training
    sr = netG.forward_images(lr, tile=16, pad=8)
    assert _close(table, M.set_metrics_reference([x.cpu() for x in sr], [x.cpu() for x in hr], 4), 1e-9)
    torch.manual_seed(6002)
    log = st.step(*batch(2))
    assert np.isfinite(log['l_pix'])
