"""Tiled inference on the GPU: the gather and stitch kernels (csrc/tile_io.hip) on their own — bit for bit against torch
slicing, the gather's side routed through the existing layout kernel — then ``forward_tiled`` against
``tiled_reference`` over the net's ordinary forward (bit identity), against the whole-image forward (exact with enough
margin, visibly not without), the shared launch plan, the mode / autograd contract, the op's refusals and
``tools/sr_infer.py --tile``."""
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

# (LR shape, tile, pad, tiles per pass)
CASES = [((1, 3, 40, 52), 16, 4, 5),      # 3 x 4 tiles of 24 x 24 windows: the last pass has 2 tiles and 3 repeats
         ((2, 3, 33, 70), 32, 8, 4)]      # 2 x 3 tiles of 33 x 48 windows, crosses the 32- and 64-wide edges: 2 tiles, 2 repeats
SENTINEL = -77.25                         # exact in fp16 and fp32
ESR_ERR_INVALID, ESR_ERR_UNSUPPORTED = -1, -3


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _tile_op(to_g32, img, tile, pad, t0, n, g=None, slots=None, prec='fp32', check=True, **over):
    """esr_tile_op on the B images of `img` (the full image of this op's side), tiles [t0, t0 + n) of each; `over`
    overrides fields of the struct."""
    from esrganplus_amd import _lib as L, engine as E
    B, C_, H, W = img.shape
    d = L.esr_tile()
    d.dtype = g.esr_dtype if g is not None else E._dt(prec)[0]
    d.to_g32, d.B, d.C, d.H, d.W = to_g32, B, C_, H, W
    d.tile, d.pad, d.scale, d.t_begin, d.t_count = tile, pad, 1 if to_g32 else 4, t0, n
    d.nchw = img.data_ptr()
    if g is not None:
        d.g32 = g.view(0, C_)
    if slots is not None:
        d.slots_nchw = slots.data_ptr()
    for k, v in over.items():
        setattr(d, k, v)
    rc = L.lib().esr_tile_op(C.byref(d), C.c_void_p(E.current_stream()))
    if check:
        L.check(rc, 'esr_tile_op')
    return rc


def _layout_in(g, nchw):
    """The existing NCHW -> G32 kernel on the whole batch of g."""
    from esrganplus_amd import _lib as L, engine as E
    B, C_, H, W = nchw.shape
    lo = L.esr_layout()
    lo.dtype, lo.to_g32, lo.B, lo.C, lo.H, lo.W = g.esr_dtype, 1, B, C_, H, W
    lo.nchw, lo.g32 = nchw.data_ptr(), g.view(0, C_)
    L.check(L.lib().esr_convert_layout(C.byref(lo), C.c_void_p(E.current_stream())), 'esr_convert_layout')


def _same_bits(a, b):
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def _windows(x, tile, pad, idx):
    """Torch slicing: the windows of the tiles `idx` of x, slot-major."""
    th, tw, _, _, tiles = F.tiled_geometry(x.shape[2], x.shape[3], tile, pad)
    return torch.cat([x[:, :, tiles[t][4]:tiles[t][4] + th, tiles[t][5]:tiles[t][5] + tw] for t in idx], 0).contiguous()


# ---- 4. the gather is torch slicing ---------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', ['fp16', 'fp32'])
@pytest.mark.parametrize('case', CASES)
def test_gather_equals_torch_slicing_through_the_layout_kernel(dev, case, prec):
    from esrganplus_amd import engine as E
    shape, tile, pad, P = case
    B, C_, H, W = shape
    x = synth.normal_like(1, 'tiled.gather', shape).to(dev)
    th, tw, ny, nx, _ = F.tiled_geometry(H, W, tile, pad)
    assert ny * nx % P != 0                                   # the last pass repeats the last tile
    for t0 in range(0, ny * nx, P):
        ref, got = (E.G32(P * B, C_, th, tw, prec, dev) for _ in range(2))
        ref.t.fill_(SENTINEL)
        got.t.fill_(SENTINEL)
        _layout_in(ref, _windows(x, tile, pad, [min(t0 + s, ny * nx - 1) for s in range(P)]))
        _tile_op(1, x, tile, pad, t0, P, g=got)
        torch.cuda.synchronize()
        # the whole buffer, byte for byte: halo and padding still hold the sentinel in both
        assert _same_bits(got.t, ref.t), t0
        assert not bool((got.t[:, :, 1:th + 1, 1:tw + 1, :C_] == SENTINEL).any())
        assert bool((got.t[:, :, 0] == SENTINEL).all()) and bool((got.t[:, :, :, 0] == SENTINEL).all())


# ---- 5. the stitch is torch slicing ---------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES)
def test_stitch_copies_every_owned_rectangle_once(dev, case):
    shape, tile, pad, P = case
    B, C_, H, W = shape
    th, tw, ny, nx, tiles = F.tiled_geometry(H, W, tile, pad)
    n = ny * nx
    slots = [synth.normal_like(7 + t0, 'tiled.stitch', (P * B, C_, 4 * th, 4 * tw)).to(dev) for t0 in range(0, n, P)]
    ref = torch.full((B, C_, 4 * H, 4 * W), SENTINEL)
    for t, (y0, y1, x0, x1, wy, wx) in enumerate(tiles):
        s = slots[t // P].cpu()[(t % P) * B:(t % P + 1) * B]
        ref[:, :, 4 * y0:4 * y1, 4 * x0:4 * x1] = s[:, :, 4 * (y0 - wy):4 * (y1 - wy), 4 * (x0 - wx):4 * (x1 - wx)]
    assert not bool((ref == SENTINEL).any())
    y = torch.full((B, C_, 4 * H, 4 * W), SENTINEL, device=dev)
    for p, t0 in enumerate(range(0, n, P)):
        _tile_op(0, y, tile, pad, t0, P, slots=slots[p])
        if p == 0:
            torch.cuda.synchronize()
            first = y.cpu()
            # the first pass wrote its own tiles and nothing else
            for t, (y0, y1, x0, x1, _, _) in enumerate(tiles):
                blk, want = first[:, :, 4 * y0:4 * y1, 4 * x0:4 * x1], ref[:, :, 4 * y0:4 * y1, 4 * x0:4 * x1]
                assert _same_bits(blk, want) if t < P else bool((blk == SENTINEL).all()), t
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


def _tiled_keys(net):
    return [k for k in net._plans if k[0] == 'tiled']


# ---- 6. forward_tiled against the pure-torch restatement over the ordinary forward ----------------------------------
@pytest.mark.parametrize('prec', ['fp32', 'fp16'])
@pytest.mark.parametrize('case', CASES)
def test_forward_tiled_is_tiled_reference_over_the_ordinary_forward(dev, small_net, case, prec):
    shape, tile, pad, P = case
    net = small_net.set_precision(prec)
    x = synth.image_batch(2, *shape, name='tiled.fwd').to(dev)
    with torch.no_grad():
        y = net.forward_tiled(x, tile, pad, P)
        ref = F.tiled_reference(net, x, tile, pad, P)
    assert tuple(y.shape) == (shape[0], 3, 4 * shape[2], 4 * shape[3])
    assert _same_bits(y, ref)
    small_net.set_precision('fp32')


@pytest.mark.parametrize('prec', ['fp32', 'fp16'])
def test_forward_tiled_of_an_image_inside_one_window_is_the_forward(dev, small_net, prec):
    net = small_net.set_precision(prec)
    x = synth.image_batch(2, 2, 3, 24, 24, name='tiled.one').to(dev)
    with torch.no_grad():
        assert _same_bits(net.forward_tiled(x, 32, 4), net(x))
    small_net.set_precision('fp32')


# ---- 7. exactness ---------------------------------------------------------------------------------------------------
def test_forward_tiled_is_exact_with_enough_margin_and_not_without(dev, small_net):
    x = synth.image_batch(2, 1, 3, 45, 70, name='tiled').to(dev)
    with torch.no_grad():
        net = small_net.set_precision('fp32')
        whole = net(x)
        e19 = (net.forward_tiled(x, 16, 19) - whole).abs().max().item()
        e0 = (net.forward_tiled(x, 16, 0) - whole).abs().max().item()
        print('forward_tiled vs net(x), 45 x 70, tile 16, nb 1, fp32: pad 19 %.3e, pad 0 %.3e (output abs-max %.3f)'
              % (e19, e0, whole.abs().max().item()))
        net = small_net.set_precision('fp16')
        whole16 = net(x)
        h19 = (net.forward_tiled(x, 16, 19) - whole16).abs().max().item()
        h0 = (net.forward_tiled(x, 16, 0) - whole16).abs().max().item()
        print('the same in fp16 (not gated): pad 19 %.3e, pad 0 %.3e' % (h19, h0))
    small_net.set_precision('fp32')
    assert e19 <= 1e-3            # the project's fp32 gate; the CPU oracle gives 4e-9 against an output abs-max of 0.074
    assert e0 > 1e-2              # the CPU oracle gives 4.6e-2


# ---- 8. one plan for all image sizes --------------------------------------------------------------------------------
def test_images_of_any_size_share_one_tiled_plan(dev):
    net = _net(dev, 1, synth.rrdbnet_state_dict(nb=1, seed=81))
    xs = [synth.image_batch(2, *shape, name='tiled.fwd').to(dev) for shape in ((1, 3, 40, 52), (1, 3, 33, 70))]
    with torch.no_grad():
        ys = [net.forward_tiled(x, 16, 4, 5) for x in xs]
        keys = _tiled_keys(net)
        assert len(keys) == 1 and len(net._plans) == 1, list(net._plans)
        assert keys[0][:5] == ('tiled', 5, 1, 24, 24)
        plan = net._plans[keys[0]]
        ys.append(net.forward_tiled(xs[0], 16, 4, 5))
        assert net._plans[keys[0]] is plan and len(net._plans) == 1
        for x, y in zip(xs + xs[:1], ys):
            assert _same_bits(y, F.tiled_reference(net, x, 16, 4, 5))


# ---- 9. mode and autograd contract, refusals ------------------------------------------------------------------------
def test_forward_tiled_ignores_train_mode_and_leaves_the_module_alone(dev):
    net = _net(dev, 1, synth.rrdbnet_state_dict(nb=1, seed=81))
    x = synth.image_batch(2, 1, 3, 13, 21, name='tiled.mode').to(dev)
    y_eval = net.forward_tiled(x, 8, 2)
    net.train()
    y_train = net.forward_tiled(x, 8, 2)
    assert _same_bits(y_train, y_eval)
    assert net.training and all(m.training for m in net.modules())
    assert all(p.requires_grad for p in net.parameters())
    assert not y_train.requires_grad and y_train.grad_fn is None and y_train.dtype == torch.float32
    assert net.forward_tiled(x.requires_grad_(True), 8, 2).requires_grad is False
    empty = net.forward_tiled(x[:0])
    assert tuple(empty.shape) == (0, 3, 52, 84) and empty.dtype == torch.float32
    for kw in (dict(tile=0), dict(pad=-1), dict(tiles_per_pass=0), dict(tile=8.0)):
        with pytest.raises(ValueError):
            net.forward_tiled(x, **kw)
    with pytest.raises(ValueError):
        net.forward_tiled(x[:, :2])                                                  # channel check


def test_tile_op_refusals(dev):
    from esrganplus_amd import _lib as L, engine as E
    g = E.G32(4, 3, 12, 12, 'fp16', dev)                                             # 12 x 12 windows: tile 8, pad 2
    g.t.fill_(SENTINEL)
    x = torch.full((1, 3, 13, 21), SENTINEL, device=dev)                             # 2 x 3 tiles
    y = torch.full((1, 3, 52, 84), SENTINEL, device=dev)
    slots = torch.full((4, 3, 48, 48), SENTINEL, device=dev)
    wide = torch.full((1, 9, 13, 21), SENTINEL, device=dev)

    def both(rc, **over):
        """The gather and the stitch refuse alike, with a message."""
        for to_g32 in (1, 0):
            L.lib().esr_tile_op(None, None)                                          # leaves another message behind
            kw = dict(tile=8, pad=2, t0=0, n=4, g=g, slots=slots, check=False)
            kw.update(over)
            assert _tile_op(to_g32, x if to_g32 else y, kw.pop('tile'), kw.pop('pad'), kw.pop('t0'), kw.pop('n'), **kw) == rc, (to_g32, over)
            msg = L.lib().esr_last_error()
            assert msg and b'invalid arguments' not in msg, msg

    assert L.lib().esr_tile_op(None, None) == ESR_ERR_INVALID
    assert L.lib().esr_last_error()
    both(ESR_ERR_UNSUPPORTED, C=9)
    both(ESR_ERR_INVALID, tile=0)
    both(ESR_ERR_INVALID, pad=-1)
    both(ESR_ERR_INVALID, scale=2)
    both(ESR_ERR_INVALID, scale=0)
    both(ESR_ERR_INVALID, t0=-1)
    both(ESR_ERR_INVALID, t0=6)                                                      # ny nx = 6
    both(ESR_ERR_INVALID, n=0)
    both(ESR_ERR_UNSUPPORTED, n=65536)
    both(ESR_ERR_UNSUPPORTED, n=32768, B=2)
    for to_g32, img in ((1, x), (0, y)):
        assert _tile_op(to_g32, img, 8, 2, 0, 4, g=g, slots=slots, check=False, nchw=None) == ESR_ERR_INVALID
        assert L.lib().esr_last_error()
    assert _tile_op(1, x, 8, 2, 0, 4, slots=slots, check=False) == ESR_ERR_INVALID   # the gather without a G32 view
    assert _tile_op(0, y, 8, 2, 0, 4, g=g, check=False) == ESR_ERR_INVALID           # the stitch without slots
    assert _tile_op(1, wide, 8, 2, 0, 4, g=g, check=False) == ESR_ERR_UNSUPPORTED    # C = 9 as the caller would pass it
    torch.cuda.synchronize()
    for t in (g.t, x, y, slots):                                                     # nothing was launched
        assert bool((t == SENTINEL).all())


# ---- 10. the inference script ---------------------------------------------------------------------------------------
def test_sr_infer_tile_runs_and_refuses_x8(tmp_path, golden):
    from PIL import Image
    g = golden('sr_infer')
    name = 'butterfly'
    in_dir, out_dir = tmp_path / 'LR', tmp_path / 'results'
    in_dir.mkdir()
    Image.fromarray(g['lr_' + name]).save(str(in_dir / (name + '.png')))
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'sr_infer.py'), 'synthetic', str(in_dir), str(out_dir), 'fp32']
    r = subprocess.run(cmd + ['--tile', '64,16'], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.array(Image.open(str(out_dir / (name + '_rlt.png'))).convert('RGB')).astype(np.int32)
    plain = g['sr_' + name].astype(np.int32)
    assert got.shape == plain.shape
    d = np.abs(got - plain)
    print('sr_infer --tile 64,16 on %s LR vs the plain output: max|diff| %d LSB, differing pixels %.2f %%'
          % (g['lr_' + name].shape[:2], d.max(), 100 * np.mean(d > 0)))
    r = subprocess.run(cmd + ['--tile', '64', '--x8'], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0
    assert '--tile and --x8 cannot be combined' in r.stderr
