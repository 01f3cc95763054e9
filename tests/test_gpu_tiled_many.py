"""Tiled inference over an image set on the GPU: the table-driven gather and stitch (csrc/tile_io.hip, esr_tile_many)
bit for bit against the per-image ``esr_tile_op`` filling the same slots one at a time, then ``forward_tiled_many``
against ``tiled_many_reference`` over the net's ordinary forward, against ``forward_tiled`` for one image, against the
whole-image forward (exact with enough margin, visibly not without), the shared launch plan, the mode / autograd
contract, the entry's refusals and ``tools/sr_infer.py --tile-many``."""
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

# (LR sizes that share a window shape, tile, pad, slots per pass)
CASES = [([(40, 52), (33, 70)], 16, 4, 5),     # 12 + 15 windows of 24 x 24: 6 passes, pass 2 crosses the images, 3 filler slots
         ([(33, 70), (45, 70)], 32, 8, 4)]     # 6 + 6 windows of 33 x 48 / 45 x 48 -> two groups; crosses the 32- and 64-wide edges
SENTINEL = -77.25                              # exact in fp16 and fp32
ESR_ERR_INVALID, ESR_ERR_UNSUPPORTED = -1, -3


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _same_bits(a, b):
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def _table(dev, entries):
    """[(tensor, H, W, t, live)] -> the uint8 device tensor of esr_tile_item entries."""
    rec = np.zeros(len(entries), dtype=F._tile_item_dtype())
    for k, (img, H, W, t, live) in enumerate(entries):
        rec[k] = (img.data_ptr(), H, W, t, live)
    return torch.from_numpy(rec.view(np.uint8).copy()).to(dev)


def _many_op(to_g32, table, n_slots, C_, tile, pad, th, tw, g=None, slots=None, prec='fp32', check=True, **over):
    from esrganplus_amd import _lib as L, engine as E
    d = L.esr_tile_many()
    d.dtype = g.esr_dtype if g is not None else E._dt(prec)[0]
    d.to_g32, d.C, d.tile, d.pad, d.scale = to_g32, C_, tile, pad, 1 if to_g32 else 4
    d.th, d.tw, d.n_slots = th, tw, n_slots
    d.items = table.data_ptr()
    if g is not None:
        d.g32 = g.view(0, C_)
    if slots is not None:
        d.slots_nchw = slots.data_ptr()
    for k, v in over.items():
        setattr(d, k, v)
    rc = L.lib().esr_tile_many_op(C.byref(d), C.c_void_p(E.current_stream()))
    if check:
        L.check(rc, 'esr_tile_many_op')
    return rc


def _one_tile_op(to_g32, img, tile, pad, t, g=None, slot=0, slots=None):
    """The existing per-image esr_tile_op on ONE tile of the [1, C, H, W] image `img`: the gather into batch entry `slot`
    of g, the stitch out of the one-window tensor `slots`."""
    from esrganplus_amd import _lib as L, engine as E
    _, C_, H, W = img.shape
    d = L.esr_tile()
    d.dtype = g.esr_dtype if g is not None else L.ESR_F32
    d.to_g32, d.B, d.C, d.H, d.W = to_g32, 1, C_, H, W
    d.tile, d.pad, d.scale, d.t_begin, d.t_count = tile, pad, 1 if to_g32 else 4, t, 1
    d.nchw = img.data_ptr()
    if g is not None:
        v = g.view(0, C_)
        v.ptr += slot * g.bs
        d.g32 = v
    if slots is not None:
        d.slots_nchw = slots.data_ptr()
    L.check(L.lib().esr_tile_op(C.byref(d), C.c_void_p(E.current_stream())), 'esr_tile_op')


def _images(dev, seed, sizes, C_=3, name='tiled_many'):
    return [synth.normal_like(seed + i, name, (1, C_, H, W)).to(dev) for i, (H, W) in enumerate(sizes)]


# ---- 1. the gather is the per-image gather, slot by slot ------------------------------------------------------------
def _check_gather(dev, sizes, tile, pad, S, prec, C_=3):
    from esrganplus_amd import engine as E
    xs = _images(dev, 11, sizes, C_)
    groups = F.tiled_many_passes(sizes, tile, pad, S)
    assert any(not l for _, _, _, ps in groups for p in ps for _, _, l in p)          # filler is covered
    assert any(len({i for i, _, _ in p}) > 1 for _, _, _, ps in groups for p in ps) or len(groups) > 1
    for th, tw, Sg, passes in groups:
        for p in passes:
            ref, got = (E.G32(Sg, C_, th, tw, prec, dev) for _ in range(2))
            ref.t.fill_(SENTINEL)
            got.t.fill_(SENTINEL)
            for s, (i, t, _) in enumerate(p):
                _one_tile_op(1, xs[i], tile, pad, t, g=ref, slot=s)
            table = _table(dev, [(xs[i], sizes[i][0], sizes[i][1], t, live) for i, t, live in p])
            _many_op(1, table, Sg, C_, tile, pad, th, tw, g=got)
            torch.cuda.synchronize()
            # the whole buffer, byte for byte: halo and padding still hold the sentinel in both
            assert _same_bits(got.t, ref.t), p
            assert not bool((got.t[:, 0, 1:th + 1, 1:tw + 1, :C_] == SENTINEL).any())
            assert bool((got.t[:, :, 0] == SENTINEL).all()) and bool((got.t[:, :, :, 0] == SENTINEL).all())


@pytest.mark.parametrize('prec', ['fp16', 'fp32'])
@pytest.mark.parametrize('case', CASES)
def test_gather_equals_the_per_image_gather_slot_by_slot(dev, case, prec):
    _check_gather(dev, *case, prec)


@pytest.mark.parametrize('C_', [1, 8])
def test_gather_and_stitch_with_one_and_eight_channels(dev, C_):
    sizes, tile, pad, S = CASES[0]
    _check_gather(dev, sizes, tile, pad, S, 'fp32', C_)
    _check_gather(dev, sizes, tile, pad, S, 'fp16', C_)
    _check_stitch(dev, sizes, tile, pad, S, C_)


# ---- 2. the stitch is the per-image stitch --------------------------------------------------------------------------
def _check_stitch(dev, sizes, tile, pad, S, C_=3):
    groups = F.tiled_many_passes(sizes, tile, pad, S)
    geo = [F.tiled_geometry(H, W, tile, pad) for H, W in sizes]
    ref = [torch.full((1, C_, 4 * H, 4 * W), SENTINEL, device=dev) for H, W in sizes]
    got = [torch.full((1, C_, 4 * H, 4 * W), SENTINEL, device=dev) for H, W in sizes]
    first = True
    for gi, (th, tw, Sg, passes) in enumerate(groups):
        for pi, p in enumerate(passes):
            slots = synth.normal_like(100 * gi + pi, 'tiled_many.stitch', (Sg, C_, 4 * th, 4 * tw)).to(dev)
            for s, (i, t, live) in enumerate(p):
                if live:
                    _one_tile_op(0, ref[i], tile, pad, t, slots=slots[s])
            table = _table(dev, [(got[i], sizes[i][0], sizes[i][1], t, live) for i, t, live in p])
            _many_op(0, table, Sg, C_, tile, pad, th, tw, slots=slots)
            if first:
                first = False
                torch.cuda.synchronize()
                # the first pass wrote its own live tiles and nothing else
                mine = {(i, t) for i, t, live in p if live}
                for i, (H, W) in enumerate(sizes):
                    y, s_ = got[i].cpu(), slots.cpu()
                    for t, (y0, y1, x0, x1, wy, wx) in enumerate(geo[i][4]):
                        blk = y[:, :, 4 * y0:4 * y1, 4 * x0:4 * x1]
                        if (i, t) in mine:
                            s = [k for k, w in enumerate(p) if w == (i, t, 1)][0]
                            want = s_[s:s + 1, :, 4 * (y0 - wy):4 * (y1 - wy), 4 * (x0 - wx):4 * (x1 - wx)]
                            assert _same_bits(blk, want), (i, t)
                        else:
                            assert bool((blk == SENTINEL).all()), (i, t)
    torch.cuda.synchronize()
    for i in range(len(sizes)):
        assert not bool((ref[i] == SENTINEL).any())               # the live slots cover every image exactly
        assert _same_bits(got[i], ref[i]), i


@pytest.mark.parametrize('case', CASES)
def test_stitch_equals_the_per_image_stitch(dev, case):
    sizes, tile, pad, S = case
    passes = [p for _, _, _, ps in F.tiled_many_passes(sizes, tile, pad, S) for p in ps]
    if case is CASES[0]:
        assert any(len({i for i, _, _ in p}) > 1 for p in passes)                     # a pass ends one image and begins the next
    _check_stitch(dev, sizes, tile, pad, S)


def test_stitch_skips_filler_slots(dev):
    """A pass of nothing but filler writes nothing, whatever its slots hold."""
    H, W, tile, pad = 13, 21, 8, 2
    y = torch.full((1, 3, 4 * H, 4 * W), SENTINEL, device=dev)
    slots = synth.normal_like(5, 'tiled_many.filler', (3, 3, 48, 48)).to(dev)
    _many_op(0, _table(dev, [(y, H, W, t, 0) for t in (0, 3, 5)]), 3, 3, tile, pad, 12, 12, slots=slots)
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all())


# ---- nets -----------------------------------------------------------------------------------------------------------
def _net(dev, nb, sd, prec='fp32', cls='RRDBNet'):
    from esrganplus_amd import architecture as arch
    net = getattr(arch, cls)(3, 3, 64, nb).to(dev).eval()
    net.load_state_dict(sd, strict=True)
    return net.set_precision(prec)


@pytest.fixture(scope='module')
def small_net(dev):
    return _net(dev, 1, synth.rrdbnet_state_dict(nb=1, seed=81))


def _keys(net, kind):
    return [k for k in net._plans if k[0] == kind]


# ---- 3. forward_tiled_many against the pure-torch restatement over the ordinary forward -----------------------------
# tile 16, pad 4: 24 x 24 windows (12 + 15 + 4 = 31, S = 5: 7 passes, 4 filler slots), 13 x 21 smaller than the window (two
# tiles, the same window twice, S = 2) and 16 x 16, a single tile (S = 1)
MIXED = [(40, 52), (13, 21), (33, 70), (16, 16), (24, 24)]


@pytest.mark.parametrize('prec', ['fp32', 'fp16'])
@pytest.mark.parametrize('cls', ['RRDBNet', 'RRDB_Net'])
def test_forward_tiled_many_is_tiled_many_reference_over_the_ordinary_forward(dev, small_net, prec, cls):
    net = small_net.set_precision(prec) if cls == 'RRDBNet' else _net(dev, 1, synth.rrdbnet_state_dict(nb=1, seed=81), prec, cls)
    groups = F.tiled_many_passes(MIXED, 16, 4, 5)
    assert [(th, tw, S) for th, tw, S, _ in groups] == [(24, 24, 5), (13, 21, 2), (16, 16, 1)]
    assert sum(len(p) for _, _, _, p in groups) == 9 and 31 % 5 != 0
    xs = [synth.image_batch(2 + i, 1, 3, H, W, name='tiled_many.fwd').to(dev) for i, (H, W) in enumerate(MIXED)]
    xs[1], xs[4] = xs[1][0], xs[4][0]                                                 # [C, H, W] and [1, C, H, W] mixed
    with torch.no_grad():
        ys = net.forward_tiled_many(xs, 16, 4, 5)
        refs = F.tiled_many_reference(net, xs, 16, 4, 5)
    assert isinstance(ys, list) and len(ys) == len(xs)
    for x, y, r, (H, W) in zip(xs, ys, refs, MIXED):
        assert tuple(y.shape) == ((1, 3, 4 * H, 4 * W) if x.dim() == 4 else (3, 4 * H, 4 * W))
        assert y.dtype == torch.float32 and y.device == x.device
        assert _same_bits(y, r), (H, W)
    small_net.set_precision('fp32')


# ---- 4. a one-image list is forward_tiled ---------------------------------------------------------------------------
@pytest.mark.parametrize('prec', ['fp32', 'fp16'])
@pytest.mark.parametrize('shape,tile,pad,S', [((40, 52), 16, 4, 5), ((33, 70), 32, 8, 4), ((13, 21), 16, 4, 16)])
def test_a_one_image_list_is_forward_tiled(dev, small_net, prec, shape, tile, pad, S):
    net = small_net.set_precision(prec)
    x = synth.image_batch(2, 1, 3, *shape, name='tiled_many.one').to(dev)
    with torch.no_grad():
        got = net.forward_tiled_many([x], tile, pad, S)
        want = net.forward_tiled(x, tile, pad, tiles_per_pass=S)
    assert len(got) == 1 and _same_bits(got[0], want)
    small_net.set_precision('fp32')


# ---- 5. exactness ---------------------------------------------------------------------------------------------------
def test_forward_tiled_many_is_exact_with_enough_margin_and_not_without(dev, small_net):
    """pad 19 = 15 nb + 4 at nb = 1: every output within 1e-3 of net(x), the project's fp32 gate; pad 0 visibly not."""
    net = small_net.set_precision('fp32')
    xs = [synth.image_batch(2, 1, 3, 45, 70, name='tiled').to(dev), synth.image_batch(3, 1, 3, 40, 52, name='tiled_many.exact').to(dev)]
    with torch.no_grad():
        whole = [net(x) for x in xs]
        e19 = [(y - w).abs().max().item() for y, w in zip(net.forward_tiled_many(xs, 16, 19, 5), whole)]
        e0 = [(y - w).abs().max().item() for y, w in zip(net.forward_tiled_many(xs, 16, 0, 5), whole)]
    print('forward_tiled_many vs net(x), 45 x 70 and 40 x 52, tile 16, nb 1, fp32: pad 19 %s, pad 0 %s' % (e19, e0))
    assert all(e <= 1e-3 for e in e19), e19
    assert max(e0) > 1e-2, e0


# ---- 6. one plan for all image lists --------------------------------------------------------------------------------
def test_image_lists_that_share_a_window_shape_share_one_plan(dev):
    net = _net(dev, 1, synth.rrdbnet_state_dict(nb=1, seed=81))
    a = [synth.image_batch(2 + i, 1, 3, H, W, name='tiled_many.plan').to(dev) for i, (H, W) in enumerate([(40, 52), (33, 70)])]
    b = [synth.image_batch(7 + i, 1, 3, H, W, name='tiled_many.plan').to(dev) for i, (H, W) in enumerate([(24, 30), (70, 33), (25, 24)])]
    with torch.no_grad():
        single = net.forward_tiled(a[0], 16, 4, 5)
        before = {k: v for k, v in net._plans.items()}
        assert [k[:5] for k in _keys(net, 'tiled')] == [('tiled', 5, 1, 24, 24)]
        ya = net.forward_tiled_many(a, 16, 4, 5)
        keys = _keys(net, 'tiled_many')
        assert len(keys) == 1 and keys[0][:4] == ('tiled_many', 5, 24, 24) and len(net._plans) == 2, list(net._plans)
        plan = net._plans[keys[0]]
        yb = net.forward_tiled_many(b, 16, 4, 5)
        assert _keys(net, 'tiled_many') == keys and net._plans[keys[0]] is plan and len(net._plans) == 2
        for k, v in before.items():
            assert net._plans[k] is v                                                 # forward_tiled's plans are not touched
        assert _same_bits(net.forward_tiled(a[0], 16, 4, 5), single)
        for xs, ys in ((a, ya), (b, yb)):
            for y, r in zip(ys, F.tiled_many_reference(net, xs, 16, 4, 5)):
                assert _same_bits(y, r)
        # max_cached_plans as the other forms: a full cache is emptied before the next plan is built
        net.max_cached_plans = 2
        net.forward_tiled_many(a, 16, 4, 4)
        assert list(net._plans) == [('tiled_many', 4, 24, 24) + keys[0][4:]]


def test_back_to_back_calls_go_round_the_table_ring(dev, small_net):
    """More calls than pinned tables, no synchronisation in between: every call's table reaches its launches intact."""
    from esrganplus_amd import engine as E
    net = small_net.set_precision('fp32')
    lists = [[synth.image_batch(20 + k, 1, 3, 13 + k, 21, name='tiled_many.ring').to(dev),
              synth.image_batch(40 + k, 1, 3, 24, 17 + k, name='tiled_many.ring').to(dev)] for k in range(E.PinnedRing().n + 2)]
    with torch.no_grad():
        ys = [net.forward_tiled_many(xs, 8, 2, 4) for xs in lists]
        torch.cuda.synchronize()
        for xs, y in zip(lists, ys):
            for got, want in zip(y, F.tiled_many_reference(net, xs, 8, 2, 4)):
                assert _same_bits(got, want)


# ---- 7. mode and autograd contract, refusals ------------------------------------------------------------------------
def test_forward_tiled_many_ignores_train_mode_and_leaves_the_module_alone(dev):
    net = _net(dev, 1, synth.rrdbnet_state_dict(nb=1, seed=81))
    xs = [synth.image_batch(2, 1, 3, 13, 21, name='tiled_many.mode').to(dev), synth.image_batch(3, 1, 3, 9, 9, name='tiled_many.mode')[0].to(dev)]
    y_eval = net.forward_tiled_many(xs, 8, 2)
    net.train()
    y_train = net.forward_tiled_many(xs, 8, 2)
    assert all(_same_bits(a, b) for a, b in zip(y_train, y_eval))
    assert net.training and all(m.training for m in net.modules())
    assert all(p.requires_grad for p in net.parameters())
    assert all(not y.requires_grad and y.grad_fn is None and y.dtype == torch.float32 for y in y_train)
    assert all(not y.requires_grad for y in net.forward_tiled_many([x.clone().requires_grad_(True) for x in xs], 8, 2))
    assert net.forward_tiled_many([]) == [] and net.forward_tiled_many(()) == []
    assert not net._plans or all(k[0] == 'tiled_many' for k in net._plans)
    n_plans = len(net._plans)
    for kw in (dict(tile=0), dict(pad=-1), dict(windows_per_pass=0), dict(tile=8.0), dict(windows_per_pass=True)):
        with pytest.raises(ValueError):
            net.forward_tiled_many(xs, **kw)
    for bad in ([xs[0][:, :2]], [xs[0], xs[0].cpu()], [xs[0].cpu()], [xs[0][0, 0]], [torch.cat([xs[0], xs[0]])], [xs[0][:, :, :0]]):
        with pytest.raises(ValueError):
            net.forward_tiled_many(bad, 8, 2)
    assert len(net._plans) == n_plans                                                 # refused before any plan


def test_tile_many_op_refusals(dev):
    from esrganplus_amd import _lib as L, engine as E
    g = E.G32(4, 3, 12, 12, 'fp16', dev)                                             # 12 x 12 windows: tile 8, pad 2
    g.t.fill_(SENTINEL)
    x = torch.full((1, 3, 13, 21), SENTINEL, device=dev)                             # 2 x 3 tiles
    y = torch.full((1, 3, 52, 84), SENTINEL, device=dev)
    slots = torch.full((4, 3, 48, 48), SENTINEL, device=dev)
    tables = {1: _table(dev, [(x, 13, 21, t, 1) for t in range(4)]), 0: _table(dev, [(y, 13, 21, t, 1) for t in range(4)])}
    lib = L.lib()

    def both(rc, **over):
        """The gather and the stitch refuse alike, with a message."""
        for to_g32 in (1, 0):
            lib.esr_tile_many_op(None, None)                                         # leaves another message behind
            kw = dict(n_slots=4, C_=3, tile=8, pad=2, th=12, tw=12, g=g, slots=slots, check=False)
            kw.update(over)
            assert _many_op(to_g32, tables[to_g32], **kw) == rc, (to_g32, over)
            msg = lib.esr_last_error()
            assert msg and b'esr_tile_many_op' in msg and b'invalid arguments' not in msg, msg

    assert lib.esr_tile_many_op(None, None) == ESR_ERR_INVALID
    assert b'esr_tile_many_op' in lib.esr_last_error()
    both(ESR_ERR_UNSUPPORTED, C=9)
    both(ESR_ERR_INVALID, tile=0)
    both(ESR_ERR_INVALID, pad=-1)
    both(ESR_ERR_INVALID, scale=2)
    both(ESR_ERR_INVALID, scale=0)
    both(ESR_ERR_INVALID, n_slots=0)
    both(ESR_ERR_INVALID, n_slots=-3)
    both(ESR_ERR_UNSUPPORTED, n_slots=65536)
    both(ESR_ERR_UNSUPPORTED, th=65535 * 4 + 1, tile=1 << 20)                        # taller than 65535 workgroups of 4 rows
    both(ESR_ERR_INVALID, th=13)                                                     # larger than tile + 2 pad
    for to_g32 in (1, 0):
        kw = dict(n_slots=4, C_=3, tile=8, pad=2, th=12, tw=12, g=g, slots=slots, check=False)
        assert _many_op(to_g32, tables[to_g32], scale=4 if to_g32 else 1, **kw) == ESR_ERR_UNSUPPORTED
        assert b'scale' in lib.esr_last_error()                                      # the other direction's scale
        assert _many_op(to_g32, tables[to_g32], items=None, **kw) == ESR_ERR_INVALID
        assert _many_op(to_g32, tables[to_g32], **dict(kw, th=0)) == ESR_ERR_INVALID
        assert _many_op(to_g32, tables[to_g32], dtype=7, **kw) == ESR_ERR_INVALID
        assert lib.esr_last_error()
    kw = dict(n_slots=4, C_=3, tile=8, pad=2, check=False)
    assert _many_op(1, tables[1], th=12, tw=12, slots=slots, **kw) == ESR_ERR_INVALID            # the gather without a G32 view
    assert _many_op(0, tables[0], th=12, tw=12, g=g, **kw) == ESR_ERR_INVALID                    # the stitch without slots
    assert _many_op(1, tables[1], th=12, tw=40, g=g, tile=40, pad=0, n_slots=4, C_=3, check=False) == ESR_ERR_INVALID
    assert b'narrower' in lib.esr_last_error()                                                   # a 40-wide window in a 12-wide view
    assert _many_op(0, tables[0], th=12, tw=12, slots=slots, slots_nchw=slots.data_ptr() + 4, **kw) == ESR_ERR_INVALID
    assert b'aligned' in lib.esr_last_error()
    torch.cuda.synchronize()
    for t in (g.t, x, y, slots):                                                     # nothing was launched
        assert bool((t == SENTINEL).all())


# ---- 8. the inference script ----------------------------------------------------------------------------------------
def test_sr_infer_tile_many_over_the_five_bundled_images(dev, tmp_path, golden):
    from PIL import Image
    from esrganplus_amd import architecture as arch
    g = golden('sr_infer')
    names = sorted(str(n) for n in g['names'])
    in_dir, out_dir = tmp_path / 'LR', tmp_path / 'results'
    in_dir.mkdir()
    for name in names:
        Image.fromarray(g['lr_' + name]).save(str(in_dir / (name + '.png')))
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'sr_infer.py'), 'synthetic', str(in_dir), str(out_dir), 'fp32']
    r = subprocess.run(cmd + ['--tile-many', '16,4'], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert lines == ['%d %s %s -> %s' % (k + 1, n, g['lr_' + n].shape[:2], g['sr_' + n].shape[:2]) for k, n in enumerate(names)]
    # the same in-process: the script's flushes (images queued until they hold 4 x 16 windows) and its rounding
    model = arch.RRDB_Net(3, 3, 64, 23, gc=32, upscale=4, norm_type=None, act_type='leakyrelu', mode='CNA', res_scale=1,
                          upsample_mode='upconv')
    model.load_state_dict(synth.rrdbnet_state_dict(23, 0), strict=False)
    model = model.eval().to(dev).set_precision('fp32')
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
        xs = [torch.from_numpy(np.transpose(g['lr_' + n].astype(np.float64) / 255, (2, 0, 1))).float().unsqueeze(0).to(dev) for n in f]
        with torch.no_grad():
            ys = model.forward_tiled_many(xs, 16, 4)
        for n, y in zip(f, ys):
            want = (np.transpose(y.squeeze().float().cpu().clamp_(0, 1).numpy(), (1, 2, 0)) * 255.0).round().astype(np.uint8)
            got = np.array(Image.open(str(out_dir / (n + '_rlt.png'))).convert('RGB'))
            assert got.shape == want.shape and np.array_equal(got, want), n
    for extra in (['--x8'], ['--tile', '16'], ['--tile-x8=16,4']):
        r = subprocess.run(cmd + ['--tile-many=16'] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode != 0 and '--tile-many' in r.stderr and 'cannot be combined' in r.stderr, (extra, r.stderr[-500:])
    r = subprocess.run(cmd + ['--tile-many', '16', '--scale', '2'], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and 'x4-only' in r.stderr
    r = subprocess.run(cmd + ['--tile-many', 'x'], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and '--tile-many takes N or N,PAD' in r.stderr
