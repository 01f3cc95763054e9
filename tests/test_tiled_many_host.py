"""Tiled inference over an image set, host side: the pass planner (``tiled_many_passes``), the pure-torch
``tiled_many_reference`` against per-image ``tiled_reference``, the refusals that need no device, and the ctypes mirror
of the new op (include/esrgan_hip.h: esr_tile_many)."""
import ctypes as C
import random

import pytest
import torch

from esrganplus_amd import functional as F
from esrganplus_amd import synth

SIZES = [(40, 52), (33, 70), (40, 52), (13, 21), (24, 24)]
SIZEOF_ESR_OP = 552          # C.sizeof(_lib.esr_op) of the commit before esr_tile_many: the union must not grow


def _tiles(H, W, tile):
    return -(-H // tile) * -(-W // tile)


def _check_plan(sizes, tile, pad, S, groups):
    """Every property the planner promises, for any size list."""
    shapes = [(min(tile + 2 * pad, H), min(tile + 2 * pad, W)) for H, W in sizes]
    order = list(dict.fromkeys(shapes))
    assert [(th, tw) for th, tw, _, _ in groups] == order                    # groups in order of first appearance
    total = 0
    for th, tw, Sg, passes in groups:
        want = [(i, t) for i, s in enumerate(shapes) if s == (th, tw) for t in range(_tiles(*sizes[i], tile))]
        assert Sg == min(S, len(want)) and len(passes) == -(-len(want) // Sg)
        assert all(len(p) == Sg for p in passes)
        flat = [w for p in passes for w in p]
        live = [(i, t) for i, t, l in flat if l]
        assert live == want                                                 # each window once, images in list order, tiles row-major
        assert all(l for p in passes[:-1] for _, _, l in p)                 # filler only in the last pass ...
        tail = passes[-1]
        k = len(want) - (len(passes) - 1) * Sg
        assert all(l for _, _, l in tail[:k])
        assert all(w == (want[-1][0], want[-1][1], 0) for w in tail[k:])    # ... and it is the group's last window
        total += len(passes)
    return total


def test_planner_groups_by_window_shape_and_fills_only_the_last_pass():
    groups = F.tiled_many_passes(SIZES, 16, 4, 5)
    # 40 x 52, 33 x 70, 40 x 52 -> 24 x 24 windows (12 + 15 + 12 = 39 windows: 8 passes, one filler slot);
    # 13 x 21 -> 13 x 21 (2 windows, S = 2); 24 x 24 -> 24 x 24, the first group again (4 more windows: 43, 9 passes)
    assert [(th, tw, S, len(p)) for th, tw, S, p in groups] == [(24, 24, 5, 9), (13, 21, 2, 1)]
    assert _check_plan(SIZES, 16, 4, 5, groups) == 10
    assert sum(l == 0 for _, _, _, ps in groups for p in ps for _, _, l in p) == 2
    # an image set and a pass that crosses from one image into the next
    assert groups[0][3][2] == ((0, 10, 1), (0, 11, 1), (1, 0, 1), (1, 1, 1), (1, 2, 1))
    assert groups[0][3][-1] == ((4, 1, 1), (4, 2, 1), (4, 3, 1), (4, 3, 0), (4, 3, 0))
    assert groups[1][3] == [((3, 0, 1), (3, 1, 1))]


def test_planner_never_takes_more_passes_than_the_per_image_loop():
    rnd = random.Random(20240611)
    for _ in range(300):
        sizes = [(rnd.randint(1, 90), rnd.randint(1, 90)) for _ in range(rnd.randint(1, 7))]
        tile, pad, S = rnd.choice((1, 7, 16, 32, 96)), rnd.choice((0, 3, 8, 16)), rnd.choice((1, 3, 5, 16))
        if tile == 1:
            sizes = [(min(h, 12), min(w, 12)) for h, w in sizes]
        groups = F.tiled_many_passes(sizes, tile, pad, S)
        total = _check_plan(sizes, tile, pad, S, groups)
        loop = sum(-(-_tiles(H, W, tile) // min(S, _tiles(H, W, tile))) for H, W in sizes)
        assert total <= loop, (sizes, tile, pad, S)


def test_planner_on_the_two_documented_folders():
    for sizes, want, loop in (([(339, 510)] * 8, 12, 16), ([(128, 128)] * 16, 4, 16)):
        groups = F.tiled_many_passes(sizes, 96, 16, 16)
        assert [(th, tw, S) for th, tw, S, _ in groups] == [(128, 128, 16)]
        assert _check_plan(sizes, 96, 16, 16, groups) == want
        assert sum(-(-_tiles(H, W, 96) // min(16, _tiles(H, W, 96))) for H, W in sizes) == loop
        assert all(l for _, _, _, ps in groups for p in ps for _, _, l in p)          # both fill their passes exactly


def _ramp_fn(seen=None):
    """Per pixel and per sample, so the batch cannot matter: nearest x4 plus a ramp over the position in the window's
    OUTPUT (tests/test_tiled_x8_host.py), which a wrong window offset would move."""
    def fn(t):
        if seen is not None:
            seen.append(tuple(t.shape))
        y = torch.nn.functional.interpolate(t, scale_factor=4, mode='nearest')
        ry = torch.arange(y.shape[2], dtype=torch.float32).view(1, 1, -1, 1) / 64
        rx = torch.arange(y.shape[3], dtype=torch.float32).view(1, 1, 1, -1) / 1024
        return y + ry + rx
    return fn


@pytest.mark.parametrize('tile,pad,S', [(16, 4, 5), (32, 8, 4), (16, 0, 16), (96, 16, 16)])
def test_tiled_many_reference_equals_per_image_tiled_reference(tile, pad, S):
    imgs = [synth.image_batch(3 + i, 1, 3, H, W, name='tiled_many.host') for i, (H, W) in enumerate(SIZES)]
    imgs[1], imgs[3] = imgs[1][0], imgs[3][0]                                         # rank 3 and rank 4 mixed
    seen = []
    got = F.tiled_many_reference(_ramp_fn(seen), imgs, tile, pad, S)
    assert len(got) == len(imgs)
    for x, y in zip(imgs, got):
        x4 = x if x.dim() == 4 else x[None]
        want = F.tiled_reference(_ramp_fn(), x4, tile, pad)
        assert y.dtype == torch.float32 and y.dim() == x.dim()
        assert torch.equal(y if y.dim() == 4 else y[None], want)
    groups = F.tiled_many_passes(SIZES, tile, pad, S)
    assert seen == [(Sg, 3, th, tw) for th, tw, Sg, passes in groups for _ in passes]  # exactly S windows of one shape
    assert F.tiled_many_reference(_ramp_fn(), [], tile, pad, S) == []


class _Net:
    """What ``run_rrdbnet_tiled_many`` reads of a net before it touches a device."""
    in_nc, out_nc = 3, 3


def test_refusals_that_need_no_device():
    x = torch.zeros(3, 13, 21)
    run = lambda images, **kw: F.run_rrdbnet_tiled_many(_Net(), images, **kw)
    for bad in (dict(tile=0), dict(pad=-1), dict(windows_per_pass=0), dict(tile=2.5), dict(pad=None), dict(tile=True),
                dict(windows_per_pass=True), dict(windows_per_pass=4.0)):
        with pytest.raises(ValueError, match='of a tiled forward must be an int >='):
            run([x], **bad)
        with pytest.raises(ValueError, match='of a tiled forward must be an int >='):
            run([], **bad)                                                            # checked before the empty list returns
        kw = dict(tile=8, pad=2, windows_per_pass=16)
        kw.update(bad)
        with pytest.raises(ValueError):
            F.tiled_many_passes([(13, 21)], **kw)
        with pytest.raises(ValueError):
            F.tiled_many_reference(_ramp_fn(), [x], **kw)
    assert run([]) == []
    for images in ([torch.zeros(13, 21)], [torch.zeros(2, 3, 13, 21)], [torch.zeros(1, 1, 3, 13, 21)], [None],
                   [x, torch.zeros(2, 13, 21)], [torch.zeros(1, 4, 13, 21)],                   # rank, channel count
                   [torch.zeros(3, 0, 21)], [x, torch.zeros(1, 3, 13, 0)]):                    # no pixels
        with pytest.raises(ValueError):
            run(images)
    with pytest.raises(ValueError, match='no pixels'):
        F.tiled_many_passes([(13, 21), (0, 5)], 8, 2, 16)
    with pytest.raises(ValueError, match='one device'):
        run([x, torch.zeros(3, 13, 21, device='meta')])
    with pytest.raises(ValueError, match='no CPU fallback'):
        run([x])                                                                      # a CPU tensor
    with pytest.raises(ValueError, match='no CPU fallback'):
        run([torch.zeros(3, 13, 21, device='meta')])
    # 256 x 257 at tile 1 has 65792 windows: more than a launch takes when they are asked for in one pass
    big = torch.zeros(3, 256, 257, device='meta')
    with pytest.raises(ValueError, match='65535'):
        run([big], tile=1, pad=0, windows_per_pass=70000)
    with pytest.raises(ValueError, match='65535'):
        F.tiled_many_passes([(256, 257)], 1, 0, 65536)
    assert F.tiled_many_passes([(256, 257)], 1, 0, 65535)[0][2] == 65535


def test_other_scales_are_refused_before_anything_else():
    from esrganplus_amd import architecture as arch
    for cls in (arch.RRDBNet, arch.RRDB_Net):
        net = cls(3, 3, 64, 1, upscale=2)
        with pytest.raises(ValueError, match='x4-only'):
            net.forward_tiled_many([torch.zeros(3, 13, 21)])
        with pytest.raises(ValueError, match='x4-only'):
            net.forward_tiled_many([])
        net4 = cls(3, 3, 64, 1)
        assert net4.forward_tiled_many([]) == []
        with pytest.raises(ValueError, match='no CPU fallback'):
            net4.forward_tiled_many([torch.zeros(3, 13, 21)])
        with pytest.raises(ValueError, match='must be an int'):
            net4.forward_tiled_many([torch.zeros(3, 13, 21)], windows_per_pass=0)


def test_lib_mirrors_the_tile_many_op():
    from esrganplus_amd import _lib as L
    assert L.OP_TILE_MANY == 19
    assert 'esr_tile_many_op' in L.EXPORTS
    assert [f[0] for f in L.esr_tile_many._fields_] == ['dtype', 'to_g32', 'C', 'tile', 'pad', 'scale', 'th', 'tw', 'n_slots',
                                                        'items', 'g32', 'slots_nchw']
    assert [f[0] for f in L.esr_tile_item._fields_] == ['nchw', 'H', 'W', 't', 'live']
    assert C.sizeof(L.esr_tile_item) == 24 == F._tile_item_dtype().itemsize
    assert 'tile_many' in [f[0] for f in L._op_union._fields_]
    assert C.sizeof(L.esr_tile_many) <= C.sizeof(L.esr_tile)
    assert C.sizeof(L.esr_op) == SIZEOF_ESR_OP
    lib = L.lib()                                             # loads the library: symbol present, sizeof(esr_op) agrees
    assert lib.esr_abi_version() == 6
    assert lib.esr_sizeof_op() == SIZEOF_ESR_OP
    assert hasattr(lib, 'esr_tile_many_op')
