"""x8 self-ensemble on the GPU: the two dihedral kernels (csrc/dihedral.hip) on their own — bit for bit against the
torch flips / transposes routed through the existing layout kernels — then ``forward_x8`` against the net's ordinary
forward (bit identity), against the reference's ``SRModel.test_x8`` (tests/golden/x8.npz, fp32 gate 1e-3), its mode /
autograd contract, the op's refusals and ``tools/sr_infer.py --x8``."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from esrganplus_amd import functional as F
from esrganplus_amd import synth
from tests.test_x8_host import CASES, x8_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LR_SHAPES = [(1, 3, 13, 21), (2, 3, 16, 16), (1, 3, 33, 70)]       # 33 x 70: crosses the 32- and 64-wide tile edges
HR_SHAPES = [(b, c, 4 * h, 4 * w) for b, c, h, w in LR_SHAPES]
SENTINEL = -77.25                                                   # exact in fp16 and fp32
ESR_ERR_INVALID, ESR_ERR_UNSUPPORTED = -1, -3


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _ranges(H, W, n):
    """The eight slots in passes of n (a pass cannot cross k = 4 unless H == W)."""
    assert n in (8, 4, 2, 1) and (n <= 4 or H == W)
    return [(k0, n) for k0 in range(0, 8, n)]


def _slot_buffers(dev, shape, prec, fill):
    """G32 buffers that hold all eight slots of `shape`: one of batch 8 B for square images, else one of 4 B at H x W
    (k 0..3) and one of 4 B at W x H (k 4..7).  -> {k: (buffer, first batch index of slot k)}"""
    from esrganplus_amd import engine as E
    B, C_, H, W = shape
    geoms = [(range(8), H, W)] if H == W else [(range(4), H, W), (range(4, 8), W, H)]
    out = {}
    for i, (ks, h, w) in enumerate(geoms):
        g = E.G32(len(ks) * B, C_, h, w, prec, dev)
        if fill == 'random':
            gen = torch.Generator().manual_seed(11 + i)
            g.t.copy_(torch.randn(g.t.shape, generator=gen).to(g.t.dtype))
        else:
            g.t.fill_(fill)
        for k in ks:
            out[k] = (g, (k - ks[0]) * B)
    return out


def _view(g, C_, b0):
    v = g.view(0, C_)
    v.ptr += b0 * g.bs
    return v


def _layout(g, b0, nchw, to_g32):
    """The existing NCHW <-> G32 kernels on images [b0, b0 + B) of g."""
    from esrganplus_amd import _lib as L, engine as E
    B, C_, H, W = nchw.shape
    lo = L.esr_layout()
    lo.dtype, lo.to_g32, lo.B, lo.C, lo.H, lo.W = g.esr_dtype, to_g32, B, C_, H, W
    lo.nchw, lo.g32 = nchw.data_ptr(), _view(g, C_, b0)
    L.check(L.lib().esr_convert_layout(C.byref(lo), C.c_void_p(E.current_stream())), 'esr_convert_layout')


def _dihedral(g, b0, nchw, to_g32, k0, n, accumulate=0, scale=1.0, slots=None, dtype=None, check=True):
    from esrganplus_amd import _lib as L, engine as E
    B, C_, H, W = nchw.shape
    d = L.esr_dihedral()
    d.dtype = g.esr_dtype if dtype is None else dtype
    d.to_g32, d.B, d.C, d.H, d.W = to_g32, B, C_, H, W
    d.nchw = nchw.data_ptr()
    if slots is not None:
        d.slots_nchw = slots.data_ptr()
    else:
        d.g32 = _view(g, min(C_, g.C), b0)
    d.k_begin, d.k_count, d.accumulate, d.scale = k0, n, accumulate, scale
    rc = L.lib().esr_dihedral_op(C.byref(d), C.c_void_p(E.current_stream()))
    if check:
        L.check(rc, 'esr_dihedral_op')
    return rc


def _same_bits(a, b):
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


# ---- 1. the import is a permutation ---------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', ['fp16', 'fp32'])
@pytest.mark.parametrize('shape', LR_SHAPES)
def test_import_equals_torch_transforms_through_the_layout_kernel(dev, shape, prec):
    B, C_, H, W = shape
    x = synth.normal_like(1, 'x8.import', shape).to(dev)
    ref = _slot_buffers(dev, shape, prec, SENTINEL)
    for k in range(8):
        g, b0 = ref[k]
        _layout(g, b0, F.x8_transform(x, k), 1)
    for n in ((8, 2) if H == W else (4, 1)):
        got = _slot_buffers(dev, shape, prec, SENTINEL)
        for k0, cnt in _ranges(H, W, n):
            g, b0 = got[k0]
            _dihedral(g, b0, x, 1, k0, cnt)
        torch.cuda.synchronize()
        for k in (0, 4):
            # the whole buffer, byte for byte: halo and padding still hold the sentinel in both
            assert _same_bits(got[k][0].t, ref[k][0].t), (n, k)
    interior = ref[0][0].t[:, :, 1:H + 1, 1:W + 1, :C_]
    assert not bool((interior == SENTINEL).any())


# ---- 2. the reduce is the sequential sum ----------------------------------------------------------------------------
@pytest.mark.parametrize('prec', ['fp16', 'fp32'])
@pytest.mark.parametrize('shape', HR_SHAPES)
def test_reduce_is_the_sequential_sum_however_it_is_split(dev, shape, prec):
    B, C_, H, W = shape
    bufs = _slot_buffers(dev, shape, prec, 'random')
    outs = []
    for k in range(8):
        g, b0 = bufs[k]
        o = torch.empty((B, C_, W, H) if k & 4 else (B, C_, H, W), device=dev)
        _layout(g, b0, o, 0)
        outs.append(o)
    acc = F.x8_inverse(outs[0], 0)
    for k in range(1, 8):
        acc = acc + F.x8_inverse(outs[k], k)
    ref = acc * 0.125
    for n in ((8, 4, 2, 1) if H == W else (4, 2, 1)):
        y = torch.full(shape, SENTINEL, device=dev)
        for k0, cnt in _ranges(H, W, n):
            g, b0 = bufs[k0]
            _dihedral(g, b0, y, 0, k0, cnt, accumulate=int(k0 > 0), scale=0.125 if k0 + cnt == 8 else 1.0)
        torch.cuda.synchronize()
        assert _same_bits(y, ref), n
    # the fp32 NCHW slot source (what the plans feed it: HR_conv1's unrounded output): the same sum
    y = torch.full(shape, SENTINEL, device=dev)
    for k0, cnt in _ranges(H, W, 4):
        _dihedral(None, 0, y, 0, k0, cnt, accumulate=int(k0 > 0), scale=0.125 if k0 else 1.0,
                  slots=torch.cat(outs[k0:k0 + cnt], 0), dtype=bufs[0][0].esr_dtype)
    torch.cuda.synchronize()
    assert _same_bits(y, ref)


# ---- nets -----------------------------------------------------------------------------------------------------------
def _net(dev, nb, sd, prec='fp32', cls='RRDBNet'):
    from esrganplus_amd import architecture as arch
    net = getattr(arch, cls)(3, 3, 64, nb).to(dev).eval()
    net.load_state_dict(sd, strict=True)
    return net.set_precision(prec)


@pytest.fixture(scope='module')
def small_net(dev):
    return _net(dev, 1, synth.rrdbnet_state_dict(nb=1, seed=81))


# ---- 3. forward_x8 against the net's own forward --------------------------------------------------------------------
@pytest.mark.parametrize('prec', ['fp32', 'fp16'])
@pytest.mark.parametrize('shape', [(2, 3, 16, 16), (1, 3, 13, 21)])
def test_forward_x8_is_x8_reference_over_the_ordinary_forward(dev, small_net, shape, prec, monkeypatch):
    net = small_net.set_precision(prec)
    x = synth.image_batch(2, *shape, name='x8.fwd').to(dev)
    monkeypatch.delenv('ESR_X8_SLOTS', raising=False)
    with torch.no_grad():
        ref = F.x8_reference(net, x)
        y = net.forward_x8(x)
        assert _same_bits(y, ref)
        assert _same_bits(F.run_rrdbnet_x8(net, x, slots_per_pass=4 if shape[2] != shape[3] else 8), ref)
        monkeypatch.setenv('ESR_X8_SLOTS', '2')
        y2 = net.forward_x8(x)
    err = (y2 - y).abs().max().item()
    print('ESR_X8_SLOTS=2 vs default, %s %s: max abs %.3e' % (shape, prec, err))
    # passes of 2 B may pick other tiles than the batch of 8 B / 4 B: the fp32 gate (1e-3), in both precisions, not
    # bit identity
    assert err <= 1e-3
    small_net.set_precision('fp32')


# ---- 4. forward_x8 against the reference's test_x8 ------------------------------------------------------------------
@pytest.mark.parametrize('cls', ['RRDBNet', 'RRDB_Net'])
@pytest.mark.parametrize('tag', CASES)
def test_forward_x8_against_the_references_test_x8(dev, golden, tag, cls):
    g = golden('x8')
    nb, sd, x = x8_case(g, tag)
    y = _net(dev, nb, sd, 'fp32', cls).forward_x8(x.to(dev)).cpu().numpy()
    err = np.abs(y - g[tag + '_y']).max()
    print('forward_x8 (%s, fp32) vs test_x8 [%s]: max abs %.3e' % (cls, tag, err))
    assert y.shape == g[tag + '_y'].shape
    assert err <= 1e-3


# ---- 5. mode and autograd contract ----------------------------------------------------------------------------------
def test_forward_x8_ignores_train_mode_and_leaves_the_module_alone(dev):
    net = _net(dev, 1, synth.rrdbnet_state_dict(nb=1, seed=81))
    x = synth.image_batch(2, 1, 3, 13, 21, name='x8.mode').to(dev)
    y_eval = net.forward_x8(x)
    net.train()
    y_train = net.forward_x8(x)
    assert _same_bits(y_train, y_eval)
    assert net.training and all(m.training for m in net.modules())
    assert all(p.requires_grad for p in net.parameters())
    assert not y_train.requires_grad and y_train.grad_fn is None and y_train.dtype == torch.float32
    assert net.forward_x8(x.requires_grad_(True)).requires_grad is False
    empty = net.forward_x8(x[:0])
    assert tuple(empty.shape) == (0, 3, 52, 84) and empty.dtype == torch.float32
    with pytest.raises(ValueError):
        net.forward_x8(x, slots_per_pass=3)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------
def test_dihedral_op_refusals(dev):
    from esrganplus_amd import _lib as L, engine as E
    g = E.G32(8, 32, 6, 6, 'fp16', dev)
    x = torch.zeros(1, 20, 6, 6, device=dev)
    assert _dihedral(g, 0, x, 1, 0, 8, check=False) == ESR_ERR_UNSUPPORTED           # two channel groups
    assert _dihedral(g, 0, x, 0, 0, 8, check=False) == ESR_ERR_UNSUPPORTED
    g = E.G32(8, 3, 7, 7, 'fp16', dev)
    x = torch.zeros(1, 3, 5, 7, device=dev)
    assert _dihedral(g, 0, x, 1, 6, 3, check=False) == ESR_ERR_INVALID               # beyond k = 7
    assert _dihedral(g, 0, x, 1, 2, 4, check=False) == ESR_ERR_INVALID               # k 2..5 with H != W
    assert _dihedral(g, 0, x, 0, 0, 8, check=False) == ESR_ERR_INVALID
    assert b'H == W' in L.lib().esr_last_error()
    torch.cuda.synchronize()
    assert float(g.t.abs().max()) == 0.0                                             # nothing was launched


# ---- 7. the inference script ----------------------------------------------------------------------------------------
def test_sr_infer_x8_runs_and_is_not_the_plain_output(tmp_path, golden):
    from PIL import Image
    g = golden('sr_infer')
    name = 'butterfly'
    in_dir, out_dir = tmp_path / 'LR', tmp_path / 'results'
    in_dir.mkdir()
    Image.fromarray(g['lr_' + name]).save(str(in_dir / (name + '.png')))
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'sr_infer.py'), 'synthetic', str(in_dir), str(out_dir),
                        'fp32', '--x8'], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.array(Image.open(str(out_dir / (name + '_rlt.png'))).convert('RGB')).astype(np.int32)
    plain = g['sr_' + name].astype(np.int32)
    assert got.shape == plain.shape
    d = np.abs(got - plain)
    print('sr_infer --x8 vs the plain output: max|diff| %d LSB, differing pixels %.2f %%' % (d.max(), 100 * np.mean(d > 0)))
    # the plain fp32 script output is within 1 LSB of this golden image on <= 0.2 % of the pixels
    # (tests/test_gpu_sr_infer.py); the ensemble is another function of the image
    assert d.max() > 1 and np.mean(d > 0) > 2e-3
