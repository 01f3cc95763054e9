"""Tiled x8 self-ensemble on the GPU: the gather-import and stitch-reduce kernels (csrc/tile_x8.hip) on their own — bit
for bit against torch slicing, flips and transposes, the gather's side routed through the existing layout kernel — then
``forward_tiled_x8`` against ``tiled_x8_reference`` over the net's ordinary forward (bit identity), against ``forward_x8``
(one window: bit identity; many windows: exact with enough margin, visibly not without), against the reference's own
``test_x8`` (tests/golden/tiled_x8.npz), the shared launch plan, the mode / autograd contract, the op's refusals and
``tools/sr_infer.py --tile-x8``."""
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
CASE_A = ((1, 3, 40, 52), 16, 4, 5)       # 3 x 4 tiles of square 24 x 24 windows (HR 96 x 96: three 32-pixel workgroup
#                                           tiles): 8 slots a pass; the last pass has 2 tiles and 3 repeats
CASE_B = ((2, 3, 33, 70), 32, 8, 4)       # 2 x 3 tiles of 33 x 48 windows: two plans of 4 slots; the last tile row owns one
#                                           LR row (4 HR rows); widths cross the 32- and 64-pixel edges; B = 2
CASES = [CASE_A, CASE_B]
# k ranges (first k, count) of the gather; B's second half runs on a tw x th view
GATHER_RANGES = {CASE_A: [(0, 8), (0, 4), (4, 4), (2, 2), (6, 1)], CASE_B: [(0, 4), (4, 4)]}
# ways to split the eight slots of the stitch-reduce
REDUCE_SPLITS = {CASE_A: [8, 4, 2, 1], CASE_B: [4, 2]}
SENTINEL = -77.25                         # exact in fp16 and fp32
ESR_ERR_INVALID, ESR_ERR_UNSUPPORTED = -1, -3


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _tile_x8_op(to_g32, img, tile, pad, t0, n, k0, kc, g=None, slots=None, accumulate=0, mean_scale=1.0, prec='fp32',
                check=True, **over):
    """esr_tile_x8_op on the B images of `img` (the full image of this op's side): tiles [t0, t0 + n) of each, slots
    [k0, k0 + kc); `over` overrides fields of the struct."""
    from esrganplus_amd import _lib as L, engine as E
    B, C_, H, W = img.shape
    d = L.esr_tile_x8()
    d.dtype = g.esr_dtype if g is not None else E._dt(prec)[0]
    d.to_g32, d.B, d.C, d.H, d.W = to_g32, B, C_, H, W
    d.tile, d.pad, d.scale, d.t_begin, d.t_count = tile, pad, 1 if to_g32 else 4, t0, n
    d.k_begin, d.k_count, d.accumulate, d.mean_scale = k0, kc, accumulate, mean_scale
    d.nchw = img.data_ptr()
    if g is not None:
        d.g32 = g.view(0, C_)
    if slots is not None:
        d.slots_nchw = slots.data_ptr()
    for k, v in over.items():
        setattr(d, k, v)
    rc = L.lib().esr_tile_x8_op(C.byref(d), C.c_void_p(E.current_stream()))
    if check:
        L.check(rc, 'esr_tile_x8_op')
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


# ---- 4. the gather-import is torch slicing + x8_transform -----------------------------------------------------------
@pytest.mark.parametrize('prec', ['fp16', 'fp32'])
@pytest.mark.parametrize('case', CASES)
def test_gather_import_equals_transformed_windows_through_the_layout_kernel(dev, case, prec):
    from esrganplus_amd import engine as E
    shape, tile, pad, P = case
    B, C_, H, W = shape
    x = synth.normal_like(1, 'tiled_x8.gather', shape).to(dev)
    th, tw, ny, nx, _ = F.tiled_geometry(H, W, tile, pad)
    assert ny * nx % P != 0                                   # the last pass repeats the last tile
    for t0 in range(0, ny * nx, P):
        wins = _windows(x, tile, pad, [min(t0 + s, ny * nx - 1) for s in range(P)])
        for k0, kc in GATHER_RANGES[case]:
            assert th == tw or k0 + kc <= 4 or k0 >= 4
            h, w = (tw, th) if k0 >= 4 else (th, tw)
            ref, got = (E.G32(kc * P * B, C_, h, w, prec, dev) for _ in range(2))
            ref.t.fill_(SENTINEL)
            got.t.fill_(SENTINEL)
            _layout_in(ref, torch.cat([F.x8_transform(wins, k) for k in range(k0, k0 + kc)], 0))
            _tile_x8_op(1, x, tile, pad, t0, P, k0, kc, g=got)
            torch.cuda.synchronize()
            # the whole buffer, byte for byte: halo and padding still hold the sentinel in both
            assert _same_bits(got.t, ref.t), (t0, k0, kc)
            assert not bool((got.t[:, :, 1:h + 1, 1:w + 1, :C_] == SENTINEL).any())
            assert bool((got.t[:, :, 0] == SENTINEL).all()) and bool((got.t[:, :, :, 0] == SENTINEL).all())


# ---- 5. the stitch-reduce is the sequential sum of the inverses, owned rectangles only ------------------------------
@pytest.mark.parametrize('case', CASES)
def test_stitch_reduce_is_the_sequential_sum_however_it_is_split(dev, case):
    shape, tile, pad, P = case
    B, C_, H, W = shape
    th, tw, ny, nx, tiles = F.tiled_geometry(H, W, tile, pad)
    n = ny * nx
    passes = list(range(0, n, P))
    # random slot outputs per pass and k: [P B][C][4 th][4 tw] for k < 4, [P B][C][4 tw][4 th] for k >= 4
    outs = [[synth.normal_like(100 * p + k, 'tiled_x8.reduce', (P * B, C_, 4 * tw, 4 * th) if k & 4 else (P * B, C_, 4 * th, 4 * tw))
             for k in range(8)] for p in range(len(passes))]
    ref = torch.full((B, C_, 4 * H, 4 * W), SENTINEL)
    for p, t0 in enumerate(passes):
        acc = F.x8_inverse(outs[p][0], 0)
        for k in range(1, 8):
            acc = acc + F.x8_inverse(outs[p][k], k)           # sequential fp32 adds in k order
        mean = acc * 0.125
        for s in range(min(P, n - t0)):                       # the tail pass's repeats contribute nothing
            y0, y1, x0, x1, wy, wx = tiles[t0 + s]
            ref[:, :, 4 * y0:4 * y1, 4 * x0:4 * x1] = mean[s * B:(s + 1) * B, :, 4 * (y0 - wy):4 * (y1 - wy), 4 * (x0 - wx):4 * (x1 - wx)]
    assert not bool((ref == SENTINEL).any())
    dev_outs = [[o.to(dev) for o in po] for po in outs]
    for cnt in REDUCE_SPLITS[case]:
        y = torch.full((B, C_, 4 * H, 4 * W), SENTINEL, device=dev)
        for p, t0 in enumerate(passes):
            for k0 in range(0, 8, cnt):
                _tile_x8_op(0, y, tile, pad, t0, P, k0, cnt, slots=torch.cat(dev_outs[p][k0:k0 + cnt], 0),
                            accumulate=int(k0 > 0), mean_scale=0.125 if k0 + cnt == 8 else 1.0)
            if p == 0:
                torch.cuda.synchronize()
                first = y.cpu()
                # the first pass wrote its own tiles' owned rectangles and nothing else
                for t, (y0, y1, x0, x1, _, _) in enumerate(tiles):
                    blk, want = first[:, :, 4 * y0:4 * y1, 4 * x0:4 * x1], ref[:, :, 4 * y0:4 * y1, 4 * x0:4 * x1]
                    assert _same_bits(blk, want) if t < P else bool((blk == SENTINEL).all()), (cnt, t)
        torch.cuda.synchronize()
        assert _same_bits(y, ref), cnt


# ---- nets -----------------------------------------------------------------------------------------------------------
def _net(dev, nb, sd, prec='fp32', cls='RRDBNet'):
    from esrganplus_amd import architecture as arch
    net = getattr(arch, cls)(3, 3, 64, nb).to(dev).eval()
    net.load_state_dict(sd, strict=True)
    return net.set_precision(prec)


@pytest.fixture(scope='module')
def small_net(dev):
    return _net(dev, 1, synth.rrdbnet_state_dict(nb=1, seed=81))


def _keys(net):
    return [k for k in net._plans if k[0] == 'tiled_x8']


# ---- 6. forward_tiled_x8 against the pure-torch restatement over the ordinary forward -------------------------------
@pytest.mark.parametrize('prec', ['fp32', 'fp16'])
@pytest.mark.parametrize('case', CASES)
def test_forward_tiled_x8_is_tiled_x8_reference_over_the_ordinary_forward(dev, small_net, case, prec, monkeypatch):
    shape, tile, pad, P = case
    net = small_net.set_precision(prec)
    x = synth.image_batch(2, *shape, name='tiled_x8.fwd').to(dev)
    monkeypatch.delenv('ESR_X8_SLOTS', raising=False)
    with torch.no_grad():
        y = net.forward_tiled_x8(x, tile, pad, P)
        assert tuple(y.shape) == (shape[0], 3, 4 * shape[2], 4 * shape[3]) and y.dtype == torch.float32
        assert _same_bits(y, F.tiled_x8_reference(net, x, tile, pad, P))
        y2 = net.forward_tiled_x8(x, tile, pad, P, slots_per_pass=2)
        assert _same_bits(y2, F.tiled_x8_reference(net, x, tile, pad, P, slots_per_pass=2))
        monkeypatch.setenv('ESR_X8_SLOTS', '2')
        y_env = net.forward_tiled_x8(x, tile, pad, P)
    assert _same_bits(y_env, y2)                              # the variable is the argument's default
    err = (y_env - y).abs().max().item()
    print('ESR_X8_SLOTS=2 vs default, %s tile %d pad %d %s: max abs %.3e' % (shape, tile, pad, prec, err))
    # passes of 2 P B windows may pick other conv tiles than 8 P B / 4 P B: the project's fp32 gate, not bit identity
    assert err <= 1e-3
    small_net.set_precision('fp32')


# ---- 7. one window: the whole-image ensemble ------------------------------------------------------------------------
@pytest.mark.parametrize('prec', ['fp32', 'fp16'])
def test_forward_tiled_x8_of_an_image_inside_one_window_is_forward_x8(dev, small_net, prec, monkeypatch):
    monkeypatch.delenv('ESR_X8_SLOTS', raising=False)
    net = small_net.set_precision(prec)
    x = synth.image_batch(2, 2, 3, 24, 24, name='tiled_x8.one').to(dev)
    with torch.no_grad():
        assert _same_bits(net.forward_tiled_x8(x, 32, 4), net.forward_x8(x))
    small_net.set_precision('fp32')


# ---- 8. exactness ---------------------------------------------------------------------------------------------------
def test_forward_tiled_x8_is_forward_x8_with_enough_margin_and_not_without(dev, small_net, monkeypatch):
    monkeypatch.delenv('ESR_X8_SLOTS', raising=False)
    x = synth.image_batch(2, 1, 3, 45, 70, name='tiled').to(dev)
    with torch.no_grad():
        net = small_net.set_precision('fp32')
        whole = net.forward_x8(x)
        e19 = (net.forward_tiled_x8(x, 16, 19) - whole).abs().max().item()
        e0 = (net.forward_tiled_x8(x, 16, 0) - whole).abs().max().item()
        print('forward_tiled_x8 vs forward_x8, 45 x 70, tile 16, nb 1, fp32: pad 19 %.3e, pad 0 %.3e (output abs-max %.3f)'
              % (e19, e0, whole.abs().max().item()))
        net = small_net.set_precision('fp16')
        whole16 = net.forward_x8(x)
        h19 = (net.forward_tiled_x8(x, 16, 19) - whole16).abs().max().item()
        h0 = (net.forward_tiled_x8(x, 16, 0) - whole16).abs().max().item()
        print('the same in fp16 (not gated): pad 19 %.3e, pad 0 %.3e' % (h19, h0))
    small_net.set_precision('fp32')
    assert e19 <= 1e-3            # the project's fp32 gate; the CPU oracle gives 0.0 against an output abs-max of 0.057
    assert e0 > 1e-2              # the CPU oracle gives 2.0e-2


# ---- 9. against the reference's own test_x8 -------------------------------------------------------------------------
@pytest.mark.parametrize('cls', ['RRDBNet', 'RRDB_Net'])
def test_forward_tiled_x8_against_the_references_test_x8(dev, golden, cls, monkeypatch):
    monkeypatch.delenv('ESR_X8_SLOTS', raising=False)
    g = golden('tiled_x8')
    nb, shape = int(g['nb']), tuple(int(v) for v in g['shape'])
    sd = synth.rrdbnet_state_dict(nb=nb, seed=int(g['sd_seed']))
    x = synth.image_batch(int(g['x_seed']), *shape, name=str(g['name']))
    y = _net(dev, nb, sd, 'fp32', cls).forward_tiled_x8(x.to(dev), 16, 15 * nb + 4).cpu().numpy()
    err = np.abs(y - g['y']).max()
    print('forward_tiled_x8 (%s, fp32, tile 16 pad 19) vs test_x8 on %s: max abs %.3e' % (cls, shape, err))
    assert y.shape == g['y'].shape
    assert err <= 1e-3


# ---- 10. one plan for all image sizes -------------------------------------------------------------------------------
def test_images_of_any_size_share_one_tiled_x8_plan(dev, monkeypatch):
    monkeypatch.delenv('ESR_X8_SLOTS', raising=False)
    net = _net(dev, 1, synth.rrdbnet_state_dict(nb=1, seed=81))
    xs = [synth.image_batch(2, *shape, name='tiled_x8.fwd').to(dev) for shape in ((1, 3, 40, 52), (1, 3, 33, 70))]
    with torch.no_grad():
        ys = [net.forward_tiled_x8(x, 16, 4, 5) for x in xs]
        keys = _keys(net)
        assert len(keys) == 1 and len(net._plans) == 1, list(net._plans)
        assert keys[0][:6] == ('tiled_x8', 8, 5, 1, 24, 24)
        plan = net._plans[keys[0]]
        ys.append(net.forward_tiled_x8(xs[0], 16, 4, 5))
        assert net._plans[keys[0]] is plan and len(net._plans) == 1
        for x, y in zip(xs + xs[:1], ys):
            assert _same_bits(y, F.tiled_x8_reference(net, x, 16, 4, 5))


# ---- 11. mode and autograd contract, the empty batch ----------------------------------------------------------------
def test_forward_tiled_x8_ignores_train_mode_and_leaves_the_module_alone(dev, monkeypatch):
    monkeypatch.delenv('ESR_X8_SLOTS', raising=False)
    net = _net(dev, 1, synth.rrdbnet_state_dict(nb=1, seed=81))
    x = synth.image_batch(2, 1, 3, 13, 21, name='tiled_x8.mode').to(dev)
    y_eval = net.forward_tiled_x8(x, 8, 2)
    net.train()
    y_train = net.forward_tiled_x8(x, 8, 2)
    assert _same_bits(y_train, y_eval)
    assert net.training and all(m.training for m in net.modules())
    assert all(p.requires_grad for p in net.parameters())
    assert not y_train.requires_grad and y_train.grad_fn is None and y_train.dtype == torch.float32
    assert net.forward_tiled_x8(x.requires_grad_(True), 8, 2).requires_grad is False
    empty = net.forward_tiled_x8(x[:0])
    assert tuple(empty.shape) == (0, 3, 52, 84) and empty.dtype == torch.float32
    for kw in (dict(tile=0), dict(pad=-1), dict(tiles_per_pass=0), dict(tile=8.0), dict(slots_per_pass=3)):
        with pytest.raises(ValueError):
            net.forward_tiled_x8(x, **kw)
    with pytest.raises(ValueError):
        net.forward_tiled_x8(x[:, :2])                                               # channel check


# ---- 12. refusals ---------------------------------------------------------------------------------------------------
def test_tile_x8_op_refusals(dev):
    from esrganplus_amd import _lib as L, engine as E
    g = E.G32(32, 3, 12, 12, 'fp16', dev)                                            # 8 slots of 4 windows of 12 x 12: tile 8, pad 2
    g.t.fill_(SENTINEL)
    x = torch.full((1, 3, 13, 21), SENTINEL, device=dev)                             # 2 x 3 tiles
    y = torch.full((1, 3, 52, 84), SENTINEL, device=dev)
    slots = torch.full((32, 3, 48, 48), SENTINEL, device=dev)
    wide = torch.full((1, 9, 13, 21), SENTINEL, device=dev)

    def one(to_g32, **over):
        kw = dict(tile=8, pad=2, t0=0, n=4, k0=0, kc=8, g=g, slots=slots, check=False)
        kw.update(over)
        return _tile_x8_op(to_g32, x if to_g32 else y, kw.pop('tile'), kw.pop('pad'), kw.pop('t0'), kw.pop('n'),
                           kw.pop('k0'), kw.pop('kc'), **kw)

    def both(rc, **over):
        """The gather-import and the stitch-reduce refuse alike, with a message."""
        for to_g32 in (1, 0):
            L.lib().esr_tile_x8_op(None, None)                                       # leaves another message behind
            assert one(to_g32, **over) == rc, (to_g32, over)
            msg = L.lib().esr_last_error()
            assert msg and b'invalid arguments' not in msg, msg

    assert L.lib().esr_tile_x8_op(None, None) == ESR_ERR_INVALID
    assert L.lib().esr_last_error()
    both(ESR_ERR_UNSUPPORTED, C=9)
    both(ESR_ERR_INVALID, tile=0)
    both(ESR_ERR_INVALID, pad=-1)
    both(ESR_ERR_INVALID, scale=2)
    both(ESR_ERR_INVALID, scale=0)
    both(ESR_ERR_INVALID, t0=-1)
    both(ESR_ERR_INVALID, t0=6)                                                      # ny nx = 6
    both(ESR_ERR_INVALID, n=0)
    both(ESR_ERR_INVALID, k0=-1)
    both(ESR_ERR_INVALID, kc=0)
    both(ESR_ERR_INVALID, k0=6, kc=3)                                                # beyond k = 7
    both(ESR_ERR_INVALID, pad=4, k0=2, kc=4)                                         # 13 x 16 windows: k 2..5 mixes two shapes
    assert b'square' in L.lib().esr_last_error()
    both(ESR_ERR_UNSUPPORTED, n=65536, kc=1)
    both(ESR_ERR_UNSUPPORTED, n=8192)                                                # 8 x 8192 x 1 slots: k counts
    both(ESR_ERR_UNSUPPORTED, n=4096, B=2)
    for to_g32 in (1, 0):
        assert one(to_g32, nchw=None) == ESR_ERR_INVALID
        assert L.lib().esr_last_error()
    assert one(1, g=None) == ESR_ERR_INVALID                                         # the gather without a G32 view
    assert one(0, slots=None) == ESR_ERR_INVALID                                     # the stitch without slots
    assert _tile_x8_op(1, wide, 8, 2, 0, 4, 0, 8, g=g, check=False) == ESR_ERR_UNSUPPORTED   # C = 9 as the caller would pass it
    # the stitch's pointers: esr_tile_op's rule, 16-byte alignment
    assert one(0, nchw=y.data_ptr() + 4) == ESR_ERR_INVALID
    assert b'aligned' in L.lib().esr_last_error()
    assert one(0, slots_nchw=slots.data_ptr() + 8) == ESR_ERR_INVALID
    torch.cuda.synchronize()
    for t in (g.t, x, y, slots):                                                     # nothing was launched
        assert bool((t == SENTINEL).all())


# ---- 13. the inference script ---------------------------------------------------------------------------------------
def test_sr_infer_tile_x8_runs_and_refuses_the_other_modes(tmp_path, golden):
    from PIL import Image
    g = golden('sr_infer')
    name = 'butterfly'
    in_dir, out_dir = tmp_path / 'LR', tmp_path / 'results'
    in_dir.mkdir()
    Image.fromarray(g['lr_' + name]).save(str(in_dir / (name + '.png')))
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'sr_infer.py'), 'synthetic', str(in_dir), str(out_dir), 'fp32']
    env = {k: v for k, v in os.environ.items() if k != 'ESR_X8_SLOTS'}
    r = subprocess.run(cmd + ['--tile-x8', '64,16'], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.array(Image.open(str(out_dir / (name + '_rlt.png'))).convert('RGB')).astype(np.int32)
    plain = g['sr_' + name].astype(np.int32)
    assert got.shape == plain.shape
    d = np.abs(got - plain)
    print('sr_infer --tile-x8 64,16 on %s LR vs the plain output: max|diff| %d LSB, differing pixels %.2f %%'
          % (g['lr_' + name].shape[:2], d.max(), 100 * np.mean(d > 0)))
    # the plain fp32 script output is within 1 LSB of this golden image on <= 0.2 % of the pixels
    # (tests/test_gpu_sr_infer.py); the ensemble is another function of the image
    assert d.max() > 1 and np.mean(d > 0) > 2e-3
    for extra in (['--x8'], ['--tile', '64'], ['--tile=64,8']):
        r = subprocess.run(cmd + ['--tile-x8=64'] + extra, capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode != 0 and '--tile-x8' in r.stderr, extra
