"""Host side of the image-set metrics (esr_image_set_metrics, metrics.device_set_metrics, evaluate_images): the numpy
restatement ``metrics.set_metrics_reference`` against the values the reference's own test script produced
(tests/golden/ssim.npz, metrics_y.npz; the tensors are the seeded ones of tests/test_gpu_metrics.py), the binding, and
every refusal that happens before a launch.  Runs without a GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from esrganplus_amd import metrics as M
from esrganplus_amd import synth
from tests.conftest import GOLDEN


def golden_pairs(which):
    """[(sr uint8 BGR, hr uint8 BGR, crop, {golden values})] of ssim.npz ('ssim') or metrics_y.npz ('mety')."""
    g = dict(np.load(os.path.join(GOLDEN, 'ssim.npz' if which == 'ssim' else 'metrics_y.npz')))
    seed0, n, keys = (90, 4, ('ssim', 'ssim_y')) if which == 'ssim' else (80, 3, ('psnr', 'psnr_y'))
    out = []
    for i in range(n):
        h, w = (int(v) for v in g['shape%d' % i])
        hr = synth.image_batch(seed0 + i, 1, 3, h, w, name=which + '.hr')[0]
        sr = hr + 0.06 * synth.normal_like(seed0 + i, which + '.n', (3, h, w))
        out.append((M.tensor2img(sr), M.tensor2img(hr), int(g['crop%d' % i]), {k: float(g['%s%d' % (k, i)]) for k in keys}))
    return out


COL = {'psnr': 0, 'ssim': 1, 'psnr_y': 2, 'ssim_y': 3}


@pytest.mark.parametrize('which', ['ssim', 'mety'])
def test_reference_reproduces_the_committed_reference_values(which):
    worst = 0.0
    for sr, hr, crop, want in golden_pairs(which):
        got = M.set_metrics_reference([sr], [hr], crop, bgr=True)
        assert got.shape == (1, 4) and got.dtype == np.float64
        for k, v in want.items():
            worst = max(worst, abs(got[0, COL[k]] - v))
        rgb = M.set_metrics_reference([sr[:, :, ::-1]], [torch.from_numpy(hr[:, :, ::-1].copy())], crop, bgr=False)
        assert np.abs(rgb - got).max() <= 1e-12
    print('largest difference from the goldens (%s): %.3e' % (which, worst))
    assert worst <= 1e-9


def test_reference_takes_a_set_and_marks_missing_ssim():
    pairs = golden_pairs('ssim')
    crop = 4
    sel = [p for p in pairs if p[2] == crop]
    small = np.arange(18 * 40 * 3, dtype=np.uint8).reshape(18, 40, 3)
    got = M.set_metrics_reference([p[0] for p in sel] + [small], [p[1] for p in sel] + [small], crop, bgr=True)
    for row, p in zip(got, sel):
        assert np.array_equal(row, M.set_metrics_reference([p[0]], [p[1]], crop, bgr=True)[0])
    assert got[-1, 0] == float('inf') and got[-1, 2] == float('inf') and np.isnan(got[-1, 1]) and np.isnan(got[-1, 3])
    assert M.set_metrics_reference([], [], 4).shape == (0, 4)


def test_symbol_is_bound_and_the_abi_is_unchanged():
    import __graft_entry__ as ge
    ge.build()
    from esrganplus_amd import _lib as L
    assert 'esr_image_set_metrics' in L.EXPORTS
    assert hasattr(ctypes.CDLL(L.LIB_PATH), 'esr_image_set_metrics')
    assert L.lib().esr_abi_version() == 6
    assert ctypes.sizeof(L.esr_set_metrics_item) == 32
    assert ctypes.sizeof(L.esr_set_metrics) == 48 + 11 * 8


def _u8(h, w, c=3, seed=0):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8))


@pytest.mark.parametrize('fn', ['device', 'reference'])
def test_set_metrics_refusals(fn):
    call = (lambda a, b, crop=4: M.device_set_metrics(a, b, crop)) if fn == 'device' else \
           (lambda a, b, crop=4: M.set_metrics_reference(a, b, crop))
    a = _u8(20, 24)
    with pytest.raises(ValueError, match='equally many'):
        call([a, a], [a])
    with pytest.raises(ValueError, match='Input images must have the same dimensions.'):
        call([a], [_u8(20, 25)])
    with pytest.raises(ValueError, match='must be a torch.uint8 tensor'):
        call([a.float()], [a])
    with pytest.raises(ValueError, match=r'must be \[H, W, 3\] \(HWC\), got rank 2'):
        call([a[:, :, 0]], [a[:, :, 0]])
    with pytest.raises(ValueError, match=r'must be \[H, W, 3\] \(HWC\): its last dimension is 4'):
        call([_u8(20, 24, 4)], [_u8(20, 24, 4)])
    with pytest.raises(ValueError, match='leaves no pixels of image 1'):
        call([a, _u8(8, 30)], [a, _u8(8, 30)])
    with pytest.raises(ValueError, match='crop of a set metric must be an int >= 0'):
        call([a], [a], -1)


def test_device_set_metrics_refuses_cpu_tensors_and_takes_an_empty_set():
    a = _u8(20, 24)
    with pytest.raises(ValueError, match='no CPU fallback'):
        M.device_set_metrics([a], [a])
    r = M.device_set_metrics([], [])
    assert len(r) == 0 and r.read().shape == (0, 4)
    with pytest.raises(ValueError, match='empty image set'):
        r.averages()


def test_evaluate_images_checks_sizes_and_scale_before_any_launch():
    from esrganplus_amd import architecture as arch
    net = arch.RRDBNet(3, 3, 64, 1)
    lr = [_u8(6, 7), _u8(5, 5)]
    with pytest.raises(ValueError, match=r'hr image 1 of evaluate_images must be \[20, 20, 3\]'):
        net.evaluate_images(lr, [_u8(24, 28), _u8(20, 21)])
    with pytest.raises(ValueError, match='equally many'):
        net.evaluate_images(lr, [_u8(24, 28)])
    with pytest.raises(ValueError, match='must be a torch.uint8 tensor'):
        net.evaluate_images(lr, [_u8(24, 28), _u8(20, 20).float()])
    with pytest.raises(ValueError, match='leaves no pixels'):
        net.evaluate_images(lr, [_u8(24, 28), _u8(20, 20)], crop=10)
    with pytest.raises(ValueError, match='no CPU fallback'):          # sizes are right: refused for the device, unlaunched
        net.evaluate_images(lr, [_u8(24, 28), _u8(20, 20)])
    x2 = arch.RRDBNet(3, 3, 64, 1, upscale=2)
    with pytest.raises(ValueError, match='evaluate_images: the tiled forms are x4-only'):
        x2.evaluate_images(lr, [_u8(12, 14), _u8(10, 10)])
    for cls in ('RRDBNet', 'RRDB_Net'):
        assert callable(getattr(getattr(arch, cls), 'evaluate_images'))


def test_train_steps_share_one_validate():
    from esrganplus_amd import train
    assert train.PSNRStep.validate is train.ESRGANPlusStep.validate is train.SRGANStep.validate
