"""The x8 self-ensemble over an image set on the GPU: the table-driven gather-import and stitch-reduce kernels
(csrc/tile_set_x8.hip) on their own — the gather bit for bit against ``esr_tile_x8_op``'s gather of the same window, the
stitch-reduce against the sequential torch sum however the eight slots are split, with fp32 NCHW and uint8 HWC images
outside — then ``forward_tiled_many_x8`` / ``forward_images(x8=True)`` against their pure-torch references over the
net's ordinary forward (bit identity), one image against ``forward_tiled_x8``, exactness against ``forward_x8``, the
shared launch plans, ``evaluate_images`` / ``PSNRStep.validate`` with ``x8``, the mode / autograd contract, the op's
refusals and ``tools/sr_infer.py --tile-u8-x8``."""
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

SIZES = [(24, 24), (40, 52), (33, 70), (21, 37), (24, 24)]
# tile 16, pad 4: square 24 x 24 windows (35 of them, border-shifted ones among them; HR 96 x 96: three 32-pixel workgroup
# tiles) and 21 x 24 windows; tile 32, pad 8: 24 x 24 whole images, 40 x 48, 33 x 48 (the last tile row owns one LR row; 192
# HR columns cross the 32- and 64-pixel edges) and 21 x 37 windows
TILINGS = [(16, 4), (32, 8)]
WPP = 32                                  # 4 square windows (8 slots) or 8 non-square ones (4 slots) per pass
# k ranges (first k, count) of the gather
SQUARE_RANGES, OBLONG_RANGES = [(0, 8), (0, 4), (4, 4), (2, 2), (6, 1)], [(0, 4), (4, 4)]
SENTINEL = -77.25                         # exact in fp16 and fp32
SENTINEL_U8 = 0xAB
ESR_ERR_INVALID, ESR_ERR_UNSUPPORTED = -1, -3


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _same_bits(a, b):
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def _table(items, dev):
    """[(tensor, H, W, t, live)] as a device table of esr_tile_item entries."""
    rec = np.zeros(len(items), dtype=F._tile_item_dtype())
    for n, (x, H, W, t, live) in enumerate(items):
        rec[n] = (x.data_ptr(), H, W, t, live)
    return torch.from_numpy(rec.view(np.uint8).copy()).to(dev)


def _set_op(to_g32, table, P, C_, tile, pad, th, tw, k0, kc, g=None, slots=None, accumulate=0, mean_scale=1.0, img=0, bgr=0,
            acc=None, prec='fp32', check=True, **over):
    """esr_tile_set_x8_op on the P windows of `table`, slots [k0, k0 + kc); `over` overrides fields of the struct."""
    from esrganplus_amd import _lib as L, engine as E
    d = L.esr_tile_set_x8()
    d.dtype = g.esr_dtype if g is not None else E._dt(prec)[0]
    d.to_g32, d.C, d.tile, d.pad, d.scale = to_g32, C_, tile, pad, 1 if to_g32 else 4
    d.th, d.tw, d.n_windows = th, tw, P
    d.items = table.data_ptr() if table is not None else None
    d.k_begin, d.k_count, d.accumulate, d.mean_scale, d.img, d.bgr = k0, kc, accumulate, mean_scale, img, bgr
    if g is not None:
        d.g32 = g.view(0, C_)
    if slots is not None:
        d.slots_nchw = slots.data_ptr()
    if acc is not None:
        d.acc = acc.data_ptr() if isinstance(acc, torch.Tensor) else acc
    for k, v in over.items():
        setattr(d, k, v)
    rc = L.lib().esr_tile_set_x8_op(C.byref(d), C.c_void_p(E.current_stream()))
    if check:
        L.check(rc, 'esr_tile_set_x8_op')
    return rc


def _tile_x8_gather(x, tile, pad, t, k0, kc, g):
    """esr_tile_x8_op's gather-import of tile t of the one image x [1, C, H, W]."""
    from esrganplus_amd import _lib as L, engine as E
    d = L.esr_tile_x8()
    d.dtype, d.to_g32, d.B, d.C, d.H, d.W = g.esr_dtype, 1, 1, x.shape[1], x.shape[2], x.shape[3]
    d.tile, d.pad, d.scale, d.t_begin, d.t_count = tile, pad, 1, t, 1
    d.k_begin, d.k_count, d.accumulate, d.mean_scale = k0, kc, 0, 1.0
    d.nchw, d.g32 = x.data_ptr(), g.view(0, x.shape[1])
    L.check(L.lib().esr_tile_x8_op(C.byref(d), C.c_void_p(E.current_stream())), 'esr_tile_x8_op')


def _u8_images(seed, C_, dev):
    g = torch.Generator().manual_seed(seed)
    out = []
    for H, W in SIZES:
        x = torch.randint(0, 256, (H, W, C_), generator=g, dtype=torch.uint8)
        x.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)          # all 256 values
        out.append(x.to(dev))
    return out


def _divided(u8, bgr):
    """The fp32 [1, C, H, W] image the 8-bit gather must see: the look-up-table division of images_reference."""
    lut = (torch.arange(256, dtype=torch.float32) / 255.0).to(u8.device)
    x = u8.flip(2) if (bgr and u8.shape[2] == 3) else u8
    return lut[x.permute(2, 0, 1).long()].unsqueeze(0).contiguous()


# ---- 1. the gather-import against esr_tile_x8_op's --------------------------------------------------------------------
@pytest.mark.parametrize('img,C_,bgr', [(0, 3, 0), (0, 1, 0), (1, 3, 0), (1, 3, 1), (1, 1, 0)])
@pytest.mark.parametrize('prec', ['fp16', 'fp32'])
def test_gather_import_is_esr_tile_x8s_gather_of_every_window(dev, prec, img, C_, bgr, monkeypatch):
    from esrganplus_amd import engine as E
    monkeypatch.delenv('ESR_X8_SLOTS', raising=False)
    u8 = _u8_images(21, C_, dev)
    if img:
        outside, floats = u8, [_divided(x, bgr) for x in u8]
    else:
        floats = [synth.normal_like(30 + i, 'set_x8.gather', (1, C_, H, W)).to(dev) for i, (H, W) in enumerate(SIZES)]
        outside = floats
    fillers = 0
    for tile, pad in TILINGS:
        for th, tw, _, P, passes in F.tiled_many_x8_passes(SIZES, tile, pad, WPP):
            for p in passes:
                fillers += sum(1 for _, _, live in p if not live)
                table = _table([(outside[i], SIZES[i][0], SIZES[i][1], t, live) for i, t, live in p], dev)
                for k0, kc in (SQUARE_RANGES if th == tw else OBLONG_RANGES):
                    h, w = (tw, th) if k0 >= 4 else (th, tw)
                    got = E.G32(kc * P, C_, h, w, prec, dev)
                    got.t.fill_(SENTINEL)
                    _set_op(1, table, P, C_, tile, pad, th, tw, k0, kc, g=got, img=img, bgr=bgr)
                    for n, (i, t, _) in enumerate(p):                 # filler windows are gathered like any other
                        ref = E.G32(kc, C_, h, w, prec, dev)
                        ref.t.fill_(SENTINEL)
                        _tile_x8_gather(floats[i], tile, pad, t, k0, kc, ref)
                        # the whole padded planes, byte for byte: the halo still holds the sentinel in both
                        assert _same_bits(got.t[n::P], ref.t), (tile, pad, th, tw, k0, kc, n)
                    assert not bool((got.t[:, :, 1:h + 1, 1:w + 1, :C_] == SENTINEL).any())
    assert fillers                                                    # a group whose last pass holds filler


# ---- 2. the stitch-reduce ---------------------------------------------------------------------------------------------
def _reduce_case(tile, pad, C_, seed):
    """Per group and pass: random slot outputs per k and the sequential mean -> [(th, tw, P, pass, outs, mean)], and the
    float results every image must end with."""
    groups, ref = [], [torch.full((C_, 4 * H, 4 * W), SENTINEL) for H, W in SIZES]
    geo = [F.tiled_geometry(H, W, tile, pad)[4] for H, W in SIZES]
    for gi, (th, tw, _, P, passes) in enumerate(F.tiled_many_x8_passes(SIZES, tile, pad, WPP)):
        for pi, p in enumerate(passes):
            outs = [0.5 + 0.8 * synth.normal_like(seed + 1000 * gi + 10 * pi + k, 'set_x8.reduce',
                                                  (P, C_, 4 * tw, 4 * th) if k & 4 else (P, C_, 4 * th, 4 * tw)) for k in range(8)]
            acc = F.x8_inverse(outs[0], 0)
            for k in range(1, 8):
                acc = acc + F.x8_inverse(outs[k], k)                  # sequential fp32 adds in k order
            mean = acc * 0.125
            for n, (i, t, live) in enumerate(p):
                if live:
                    y0, y1, x0, x1, wy, wx = geo[i][t]
                    ref[i][:, 4 * y0:4 * y1, 4 * x0:4 * x1] = mean[n, :, 4 * (y0 - wy):4 * (y1 - wy), 4 * (x0 - wx):4 * (x1 - wx)]
            groups.append((th, tw, P, p, outs, mean))
    assert not any(bool((r == SENTINEL).any()) for r in ref)
    return groups, ref


def _quant(y, bgr):
    """rint(clamp(y, 0, 1) * 255) of a [C, H, W] float image as uint8 HWC."""
    q = (y.clamp(0, 1) * 255.0).round().to(torch.uint8).permute(1, 2, 0)
    return (q.flip(2) if bgr and q.shape[2] == 3 else q).contiguous()


@pytest.mark.parametrize('img,C_,bgr', [(0, 3, 0), (0, 1, 0), (1, 3, 0), (1, 3, 1), (1, 1, 0)])
@pytest.mark.parametrize('tile,pad', TILINGS)
def test_stitch_reduce_is_the_sequential_sum_however_it_is_split(dev, tile, pad, img, C_, bgr, monkeypatch):
    monkeypatch.delenv('ESR_X8_SLOTS', raising=False)
    groups, ref = _reduce_case(tile, pad, C_, 7)
    want = [_quant(r, bgr) for r in ref] if img else ref
    lo = sum(int((r < 0).sum()) for r in ref)
    hi = sum(int((r > 1).sum()) for r in ref)
    assert lo and hi                                                  # the clamp is exercised on both sides

    def fresh():
        if img:
            return [torch.full((4 * H, 4 * W, C_), SENTINEL_U8, dtype=torch.uint8, device=dev) for H, W in SIZES]
        return [torch.full((C_, 4 * H, 4 * W), SENTINEL, device=dev) for H, W in SIZES]

    dev_outs = [[o.to(dev) for o in outs] for _, _, _, _, outs, _ in groups]
    for cnt in (8, 4, 2, 1):
        ys = fresh()
        for (th, tw, P, p, _, _), outs in zip(groups, dev_outs):
            if th != tw and cnt == 8:
                continue
            table = _table([(ys[i], SIZES[i][0], SIZES[i][1], t, live) for i, t, live in p], dev)
            # between the ranges the 8-bit form's sums live in acc: NaN where no range has written yet
            acc = torch.full((P, C_, 4 * th, 4 * tw), float('nan'), device=dev) if img and cnt < 8 else None
            for k0 in range(0, 8, cnt):
                _set_op(0, table, P, C_, tile, pad, th, tw, k0, cnt, slots=torch.cat(outs[k0:k0 + cnt], 0),
                        accumulate=int(k0 > 0), mean_scale=0.125 if k0 + cnt == 8 else 1.0, img=img, bgr=bgr, acc=acc)
        torch.cuda.synchronize()
        for i, (y, w) in enumerate(zip(ys, want)):
            if cnt == 8 and min(tile + 2 * pad, SIZES[i][0]) != min(tile + 2 * pad, SIZES[i][1]):
                assert bool((y == (SENTINEL_U8 if img else SENTINEL)).all())      # (a non-square group: not run at 8)
            else:
                assert _same_bits(y, w), (cnt, i)


@pytest.mark.parametrize('img', [0, 1])
def test_stitch_reduce_writes_owned_rectangles_of_live_windows_only(dev, img, monkeypatch):
    """One pass on sentinel-filled results: its live windows' owned rectangles are written, nothing else is — and a
    filler entry that names a tile no live entry names leaves that tile alone."""
    monkeypatch.delenv('ESR_X8_SLOTS', raising=False)
    tile, pad, C_ = 16, 4, 3
    groups, ref = _reduce_case(tile, pad, C_, 9)
    geo = [F.tiled_geometry(H, W, tile, pad)[4] for H, W in SIZES]
    for th, tw, P, p, outs, _ in groups:
        if all(live for _, _, live in p):
            continue
        for cnt in (4, 2):
            if img:
                ys = [torch.full((4 * H, 4 * W, C_), SENTINEL_U8, dtype=torch.uint8, device=dev) for H, W in SIZES]
            else:
                ys = [torch.full((C_, 4 * H, 4 * W), SENTINEL, device=dev) for H, W in SIZES]
            # the filler entries name tile 0 of image 1, which no live entry of this pass names
            assert all((i, t) != (1, 0) for i, t, live in p if live)
            entries = [(i, t, 1) if live else (1, 0, 0) for i, t, live in p]
            table = _table([(ys[i], SIZES[i][0], SIZES[i][1], t, live) for i, t, live in entries], dev)
            acc = torch.full((P, C_, 4 * th, 4 * tw), SENTINEL, device=dev) if img else None
            for k0 in range(0, 8, cnt):
                _set_op(0, table, P, C_, tile, pad, th, tw, k0, cnt, slots=torch.cat([o.to(dev) for o in outs[k0:k0 + cnt]], 0),
                        accumulate=int(k0 > 0), mean_scale=0.125 if k0 + cnt == 8 else 1.0, img=img, acc=acc)
            torch.cuda.synchronize()
            want = [torch.full((C_, 4 * H, 4 * W), SENTINEL) for H, W in SIZES]
            for i, t, live in entries:
                if live:
                    y0, y1, x0, x1, _, _ = geo[i][t]
                    want[i][:, 4 * y0:4 * y1, 4 * x0:4 * x1] = ref[i][:, 4 * y0:4 * y1, 4 * x0:4 * x1]
            for i, (y, w) in enumerate(zip(ys, want)):
                if img:
                    q = _quant(w, 0)
                    q[(w == SENTINEL).permute(1, 2, 0)] = SENTINEL_U8
                    assert _same_bits(y, q), (cnt, i)
                else:
                    assert _same_bits(y, w), (cnt, i)
            if img:                                                   # the filler windows' acc entries are not touched
                for n, (_, _, live) in enumerate(entries):
                    assert live or bool((acc[n] == SENTINEL).all())


# ---- nets -------------------------------------------------------------------------------------------------------------
def _net(dev, prec='fp32', nb=1):
    from esrganplus_amd import architecture as arch
    net = arch.RRDBNet(3, 3, 64, nb).to(dev).eval()
    net.load_state_dict(synth.rrdbnet_state_dict(nb=nb, seed=81), strict=True)
    net.max_cached_plans = 64              # the form's plans and the ordinary plans of its reference stay cached side by side
    return net.set_precision(prec)


def _float_images(dev, seed=2):
    return [synth.image_batch(seed + i, 1, 3, H, W, name='set_x8.fwd').to(dev)[0] for i, (H, W) in enumerate(SIZES)]


def _keys(net):
    return [k for k in net._plans if isinstance(k[0], str) and k[0].startswith('tiled_set_x8')]


# ---- 3. against the references ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('spp', [None, 2])
@pytest.mark.parametrize('prec', ['fp32', 'fp16'])
@pytest.mark.parametrize('tile,pad', TILINGS)
def test_forward_tiled_many_x8_is_its_reference_over_the_ordinary_forward(dev, tile, pad, prec, spp, monkeypatch):
    monkeypatch.delenv('ESR_X8_SLOTS', raising=False)
    net = _net(dev, prec)
    xs = _float_images(dev)
    xs[1] = xs[1][None]                                               # ranks are kept
    with torch.no_grad():
        ys = net.forward_tiled_many_x8(xs, tile, pad, slots_per_pass=spp)
        refs = F.tiled_many_x8_reference(net, xs, tile, pad, slots_per_pass=spp)
    assert len(ys) == len(xs)
    for x, y, r in zip(xs, ys, refs):
        assert y.dtype == torch.float32 and tuple(y.shape) == tuple(x.shape[:-2]) + (4 * x.shape[-2], 4 * x.shape[-1])
        assert _same_bits(y, r)


@pytest.mark.parametrize('bgr', [False, True])
@pytest.mark.parametrize('tile,pad,prec,spp', [(16, 4, 'fp16', None), (32, 8, 'fp32', None), (16, 4, 'fp32', 2), (32, 8, 'fp16', 1)])
def test_forward_images_x8_is_its_reference_and_the_quantised_float_form(dev, tile, pad, prec, spp, bgr, monkeypatch):
    monkeypatch.delenv('ESR_X8_SLOTS', raising=False)
    net = _net(dev, prec)
    u8 = _u8_images(5, 3, dev)
    with torch.no_grad():
        ys = net.forward_images(u8, tile, pad, bgr=bgr, x8=True, slots_per_pass=spp)
        refs = F.images_x8_reference(net, u8, tile, pad, 16, spp, bgr)
        floats = net.forward_tiled_many_x8([_divided(x, bgr)[0] for x in u8], tile, pad, slots_per_pass=spp)
        plain = net.forward_images(u8, tile, pad, bgr=bgr)
    for x, y, r, f in zip(u8, ys, refs, floats):
        assert y.dtype == torch.uint8 and tuple(y.shape) == (4 * x.shape[0], 4 * x.shape[1], 3) and y.is_contiguous()
        assert _same_bits(y, r)
        assert _same_bits(y, _quant(f, bgr))
    assert any(not _same_bits(a, b) for a, b in zip(ys, plain))      # the ensemble is another function of the image
    kinds = {k[0] for k in _keys(net)}
    assert kinds == {'tiled_set_x8', 'tiled_set_x8_img'}


# ---- 4. one image: forward_tiled_x8 -------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', ['fp32', 'fp16'])
@pytest.mark.parametrize('shape,tile,pad,P,slots', [((40, 52), 16, 4, 5, 8), ((33, 70), 32, 8, 4, 4), ((33, 70), 32, 8, 2, 2)])
def test_one_image_is_forward_tiled_x8(dev, shape, tile, pad, P, slots, prec, monkeypatch):
    monkeypatch.delenv('ESR_X8_SLOTS', raising=False)
    net = _net(dev, prec)
    x = synth.image_batch(2, 1, 3, *shape, name='tiled_x8.fwd').to(dev)
    with torch.no_grad():
        (y,) = net.forward_tiled_many_x8([x[0]], tile, pad, windows_per_pass=slots * P, slots_per_pass=slots)
        want = net.forward_tiled_x8(x, tile, pad, P, slots)
    assert _same_bits(y[None], want)


# ---- 5. exactness ---------------------------------------------------------------------------------------------------------
def test_forward_tiled_many_x8_is_forward_x8_with_enough_margin_and_not_without(dev, monkeypatch):
    """forward_tiled_x8's comparison (tests/test_gpu_tiled_x8.py) through the image-set form: the project's fp32 gate at
    pad 19 = 15 nb + 4, where the CPU oracle gives 0.0, and visibly not at pad 0 (the CPU oracle: 2.0e-2)."""
    monkeypatch.delenv('ESR_X8_SLOTS', raising=False)
    net = _net(dev, 'fp32')
    x = synth.image_batch(2, 1, 3, 45, 70, name='tiled').to(dev)
    with torch.no_grad():
        whole = net.forward_x8(x)
        e19 = (net.forward_tiled_many_x8([x], 16, 19)[0] - whole).abs().max().item()
        e0 = (net.forward_tiled_many_x8([x], 16, 0)[0] - whole).abs().max().item()
    print('forward_tiled_many_x8 vs forward_x8, 45 x 70, tile 16, nb 1, fp32: pad 19 %.3e, pad 0 %.3e (output abs-max %.3f)'
          % (e19, e0, whole.abs().max().item()))
    assert e19 <= 1e-3
    assert e0 > 1e-2


# ---- 6. shared plans --------------------------------------------------------------------------------------------------------
def test_images_that_share_a_window_shape_share_the_plans(dev, monkeypatch):
    monkeypatch.delenv('ESR_X8_SLOTS', raising=False)
    net = _net(dev, 'fp16')
    a = [synth.image_batch(40 + i, 1, 3, H, W, name='set_x8.plans').to(dev)[0] for i, (H, W) in enumerate([(40, 52), (24, 24)])]
    b = [synth.image_batch(50 + i, 1, 3, H, W, name='set_x8.plans').to(dev)[0] for i, (H, W) in enumerate([(33, 70), (57, 24)])]
    ua, ub = [(x.permute(1, 2, 0) * 255).round().to(torch.uint8).contiguous() for x in a], [(x.permute(1, 2, 0) * 255).round().to(torch.uint8).contiguous() for x in b]
    with torch.no_grad():
        net.forward_tiled_many_x8(a, 16, 4)
        net.forward_images(ua, 16, 4, x8=True)
        keys = _keys(net)
        assert [k[:5] for k in keys] == [('tiled_set_x8', 8, 2, 24, 24), ('tiled_set_x8_img', 8, 2, 24, 24)] and len(net._plans) == 2
        plans = [net._plans[k] for k in keys]
        assert plans[0].acc is None and plans[1].acc is None          # all eight slots in one pass: no accumulator
        # other images of other sizes, the other channel order, another tile / pad with the same 24 x 24 window
        net.forward_tiled_many_x8(b, 16, 4)
        net.forward_images(ub, 16, 4, bgr=True, x8=True)
        net.forward_tiled_many_x8(b, 20, 2)
        net.forward_images(ub, 20, 2, x8=True)
        assert _keys(net) == keys and [net._plans[k] for k in keys] == plans and len(net._plans) == 2
        # fewer slots: another plan, with an accumulator of P windows that the two plans of a non-square shape share
        net.forward_images(ub, 20, 3, x8=True, slots_per_pass=2)
        new = [k for k in _keys(net) if k not in keys]
        assert [k[:5] for k in new] == [('tiled_set_x8_img', 2, 8, 26, 26), ('tiled_set_x8_img', 2, 6, 26, 24)]
        sq, ob = (net._plans[k] for k in new)
        assert tuple(sq.acc.shape) == (8, 3, 104, 104) and len(sq.plans) == 1
        assert tuple(ob.acc.shape) == (6, 3, 104, 96) and len(ob.plans) == 2
        arrs = [p.ops.array()[p.out_op].u.tile_set_x8 for p in ob.plans]
        assert arrs[0].acc == arrs[1].acc == ob.acc.data_ptr() and arrs[0].img == arrs[1].img == 1


# ---- 7. evaluate_images and validate ------------------------------------------------------------------------------------------
def test_evaluate_images_and_validate_with_x8(dev, monkeypatch):
    from esrganplus_amd import metrics as M, train
    monkeypatch.delenv('ESR_X8_SLOTS', raising=False)
    net = _net(dev, 'fp16')
    lr = _u8_images(6, 3, dev)
    g = torch.Generator().manual_seed(8)
    hr = [torch.randint(0, 256, (4 * H, 4 * W, 3), generator=g, dtype=torch.uint8).to(dev) for H, W in SIZES]
    with torch.no_grad():
        for bgr in (False, True):
            want = net.forward_images(lr, 16, 4, bgr=bgr, x8=True)
            sr, res = net.evaluate_images(lr, hr, 16, 4, bgr=bgr, x8=True)
            assert len(sr) == len(want) and all(_same_bits(a, b) for a, b in zip(sr, want))
            table = M.device_set_metrics(want, hr, 4, bgr).read()
            assert res.read().shape == (5, 4) and np.array_equal(res.read(), table)
        sr2, res2 = net.evaluate_images(lr, hr, 16, 4, x8=True, slots_per_pass=2)
        want2 = net.forward_images(lr, 16, 4, x8=True, slots_per_pass=2)
        assert all(_same_bits(a, b) for a, b in zip(sr2, want2))
        assert np.array_equal(res2.read(), M.device_set_metrics(want2, hr, 4, False).read())
        # x8=False is today's call
        plain = net.forward_images(lr, 16, 4)
        for sr0, res0 in (net.evaluate_images(lr, hr, 16, 4), net.evaluate_images(lr, hr, 16, 4, x8=False)):
            assert all(_same_bits(a, b) for a, b in zip(sr0, plain))
            assert np.array_equal(res0.read(), M.device_set_metrics(plain, hr, 4, False).read())
        assert all(_same_bits(a, b) for a, b in zip(net.forward_images(lr, 16, 4, x8=False), plain))
        assert any(not _same_bits(a, b) for a, b in zip(plain, sr))
    st = train.PSNRStep(net, pixel_criterion='l2')
    psnr8 = st.validate(lr, hr, x8=True, tile=16, pad=4)
    sr8, res8 = net.evaluate_images(lr, hr, 16, 4, x8=True)
    assert psnr8 == res8.averages()[0] == sum(float(v) for v in res8.read()[:, 0]) / 5
    assert np.array_equal(st.val_result.read(), res8.read())
    psnr1 = st.validate(lr, hr, tile=16, pad=4)
    assert psnr1 == st.validate(lr, hr, x8=False, tile=16, pad=4) == net.evaluate_images(lr, hr, 16, 4)[1].averages()[0]
    assert psnr1 != psnr8


# ---- 8. the module is left alone --------------------------------------------------------------------------------------------
def test_the_set_forms_ignore_train_mode_and_leave_the_module_alone(dev, monkeypatch):
    monkeypatch.delenv('ESR_X8_SLOTS', raising=False)
    net = _net(dev, 'fp32')
    xs = [x.requires_grad_(True) for x in _float_images(dev)[2:4]]
    u8 = _u8_images(6, 3, dev)[2:4]
    y_eval, u_eval = net.forward_tiled_many_x8(xs, 16, 4), net.forward_images(u8, 16, 4, x8=True)
    net.train()
    y_train, u_train = net.forward_tiled_many_x8(xs, 16, 4), net.forward_images(u8, 16, 4, x8=True)
    assert all(_same_bits(a, b) for a, b in zip(y_train + u_train, y_eval + u_eval))
    assert net.training and all(m.training for m in net.modules())
    assert all(p.requires_grad for p in net.parameters())
    assert all(not y.requires_grad and y.grad_fn is None for y in y_train + u_train)
    assert net.forward_tiled_many_x8([]) == [] and net.forward_images([], x8=True) == []


# ---- 9. the op's refusals -------------------------------------------------------------------------------------------------------
def test_tile_set_x8_op_refusals(dev):
    from esrganplus_amd import _lib as L, engine as E
    g = E.G32(32, 3, 12, 12, 'fp16', dev)                              # 8 slots of 4 windows of 12 x 12: tile 8, pad 2
    g.t.fill_(SENTINEL)
    x = torch.full((3, 13, 21), SENTINEL, device=dev)
    y = torch.full((3, 52, 84), SENTINEL, device=dev)
    u = torch.full((52, 84, 3), SENTINEL_U8, dtype=torch.uint8, device=dev)
    slots = torch.full((32, 3, 48, 48), SENTINEL, device=dev)
    acc = torch.full((4, 3, 48, 48), SENTINEL, device=dev)
    tables = {1: _table([(x, 13, 21, t, 1) for t in range(4)], dev), 0: _table([(y, 13, 21, t, 1) for t in range(4)], dev)}
    table_u = _table([(u, 13, 21, t, 1) for t in range(4)], dev)

    def one(to_g32, **over):
        kw = dict(table=tables[to_g32], P=4, C_=3, tile=8, pad=2, th=12, tw=12, k0=0, kc=8, g=g, slots=slots, check=False)
        kw.update(over)
        return _set_op(to_g32, kw.pop('table'), kw.pop('P'), kw.pop('C_'), kw.pop('tile'), kw.pop('pad'), kw.pop('th'),
                       kw.pop('tw'), kw.pop('k0'), kw.pop('kc'), **kw)

    def both(rc, word=None, **over):
        """The gather-import and the stitch-reduce refuse alike, with a message."""
        for to_g32 in (1, 0):
            L.lib().esr_tile_set_x8_op(None, None)                     # leaves another message behind
            assert one(to_g32, **over) == rc, (to_g32, over)
            msg = L.lib().esr_last_error()
            assert msg and b'invalid arguments' not in msg and (word is None or word in msg), msg

    assert L.lib().esr_tile_set_x8_op(None, None) == ESR_ERR_INVALID
    assert b'invalid arguments' in L.lib().esr_last_error()
    for to_g32 in (1, 0):                                              # null pointers
        assert one(to_g32, table=None) == ESR_ERR_INVALID
        assert L.lib().esr_last_error()
    assert one(1, g=None) == ESR_ERR_INVALID
    assert one(0, slots=None) == ESR_ERR_INVALID
    both(ESR_ERR_INVALID, b'tile', tile=0)
    both(ESR_ERR_INVALID, b'pad', pad=-1)
    both(ESR_ERR_INVALID, b'scale', scale=2)
    both(ESR_ERR_INVALID, b'scale', scale=0)
    assert one(1, scale=4) == ESR_ERR_UNSUPPORTED and one(0, scale=1) == ESR_ERR_UNSUPPORTED
    both(ESR_ERR_UNSUPPORTED, b'channel group', C=9)
    both(ESR_ERR_UNSUPPORTED, b'8-bit images', C=2, img=1)
    both(ESR_ERR_UNSUPPORTED, b'8-bit images', C=4, img=1)
    both(ESR_ERR_INVALID, b'of 8', k0=-1)
    both(ESR_ERR_INVALID, b'of 8', kc=0)
    both(ESR_ERR_INVALID, b'of 8', k0=6, kc=3)
    both(ESR_ERR_INVALID, b'of 8', k0=8, kc=1)
    both(ESR_ERR_INVALID, b'square', th=12, tw=10, k0=2, kc=4)          # k 2..5 mixes 12 x 10 and 10 x 12 slots
    both(ESR_ERR_INVALID, b'larger than tile', th=13, tw=13)            # tile + 2 pad = 12
    both(ESR_ERR_INVALID, b'larger than tile', tw=16, th=8, k0=0, kc=4)
    both(ESR_ERR_INVALID, b'n_windows', P=0)
    both(ESR_ERR_UNSUPPORTED, b'too many', P=8192)                      # 8 x 8192 batch entries: k counts
    both(ESR_ERR_UNSUPPORTED, b'too many', P=65536, kc=1)
    both(ESR_ERR_INVALID, b'8-byte', items=tables[1].data_ptr() + 4)
    # a G32 view narrower than the slots: the rows of 12 x 12 planes under the straight slots of 12 x 40 windows, and
    # under the transposed slots of 40 x 12 ones
    assert g.view(0, 3).wp < 42
    assert one(1, tile=40, pad=0, th=12, tw=40, k0=0, kc=4) == ESR_ERR_INVALID
    assert b'narrower' in L.lib().esr_last_error()
    assert one(1, tile=40, pad=0, th=40, tw=12, k0=4, kc=4) == ESR_ERR_INVALID
    assert b'narrower' in L.lib().esr_last_error()
    # the stitch-reduce's pointers
    assert one(0, slots_nchw=slots.data_ptr() + 8) == ESR_ERR_INVALID
    assert b'aligned' in L.lib().esr_last_error()
    for kw in (dict(k0=0, kc=4), dict(k0=4, kc=4, accumulate=1), dict(k0=2, kc=2, accumulate=1)):
        assert one(0, table=table_u, img=1, **kw) == ESR_ERR_INVALID    # an 8-bit result and no acc between the ranges
        assert b'need acc' in L.lib().esr_last_error()
        assert one(0, table=table_u, img=1, acc=acc.data_ptr() + 4, **kw) == ESR_ERR_INVALID
        assert b'acc needs 16-byte' in L.lib().esr_last_error()
    torch.cuda.synchronize()
    for t in (g.t, x, y, slots, acc):                                  # nothing was launched
        assert bool((t == SENTINEL).all())
    assert bool((u == SENTINEL_U8).all())
    # and what is not refused: all eight slots of an 8-bit result need no acc
    assert one(0, table=table_u, img=1, mean_scale=0.125) == 0
    torch.cuda.synchronize()
    assert bool((acc == SENTINEL).all()) and not bool((u == SENTINEL_U8).all())


# ---- 10. the inference script -------------------------------------------------------------------------------------------------
def test_sr_infer_tile_u8_x8_over_the_five_bundled_images(tmp_path, golden):
    from PIL import Image
    g = golden('sr_infer')
    names = sorted(str(n) for n in g['names'])
    in_dir = tmp_path / 'LR'
    in_dir.mkdir()
    for name in names:
        Image.fromarray(g['lr_' + name]).save(str(in_dir / (name + '.png')))
    env = {k: v for k, v in os.environ.items() if k != 'ESR_X8_SLOTS'}
    outs = {}
    for flag in ('--tile-u8-x8', '--tile-u8'):
        out_dir = tmp_path / flag.strip('-')
        cmd = [sys.executable, os.path.join(ROOT, 'tools', 'sr_infer.py'), 'synthetic', str(in_dir), str(out_dir), 'fp16', flag, '32,8']
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.strip()]
        assert lines == ['%d %s %s -> %s' % (k + 1, n, g['lr_' + n].shape[:2], g['sr_' + n].shape[:2]) for k, n in enumerate(names)]
        outs[flag] = [np.array(Image.open(str(out_dir / (n + '_rlt.png'))).convert('RGB')) for n in names]
    for n, a, b in zip(names, outs['--tile-u8-x8'], outs['--tile-u8']):
        assert a.shape == b.shape == g['sr_' + n].shape and a.dtype == np.uint8
        d = np.abs(a.astype(np.int32) - b.astype(np.int32))
        print('sr_infer --tile-u8-x8 32,8 vs --tile-u8 32,8 on %s %s fp16: max|diff| %d LSB, differing pixels %.2f %%'
              % (n, g['lr_' + n].shape[:2], d.max(), 100 * np.mean(d > 0)))
        assert d.max() > 0                                            # the ensemble is another function of the image
    for extra in (['--x8'], ['--tile-u8', '64']):
        cmd = [sys.executable, os.path.join(ROOT, 'tools', 'sr_infer.py'), 'synthetic', str(in_dir), str(tmp_path / 'no'), 'fp16']
        r = subprocess.run(cmd + ['--tile-u8-x8=64'] + extra, capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode != 0 and 'self-ensemble over the folder by itself' in r.stderr, extra
