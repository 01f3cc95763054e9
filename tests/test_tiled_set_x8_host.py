"""The x8 self-ensemble over an image set, host side: the pass planner (``tiled_many_x8_passes``), the two pure-torch
references on the CPU, the refusals that need no device, and the ctypes mirror of the new op (include/esrgan_hip.h:
esr_tile_set_x8) against the header compiled as C."""
import ctypes as C
import os
import subprocess

import pytest
import torch

from esrganplus_amd import functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(24, 24), (40, 52), (33, 70), (21, 37), (24, 24)]
SIZEOF_ESR_OP = 552          # C.sizeof(_lib.esr_op) of the parent commit: the union must not grow


def _tiles(H, W, tile):
    return -(-H // tile) * -(-W // tile)


def _check_plan(sizes, tile, pad, wpp, spp, groups):
    """Every property the planner promises, for any size list -> passes in all."""
    shapes = [(min(tile + 2 * pad, H), min(tile + 2 * pad, W)) for H, W in sizes]
    assert [(th, tw) for th, tw, _, _, _ in groups] == list(dict.fromkeys(shapes))     # groups in order of first appearance
    total = 0
    for th, tw, slots, P, passes in groups:
        want = [(i, t) for i, s in enumerate(shapes) if s == (th, tw) for t in range(_tiles(*sizes[i], tile))]
        assert slots == min(spp or 8, 8 if th == tw else 4)
        assert P == min(max(1, wpp // slots), len(want)) and len(passes) == -(-len(want) // P)
        assert all(len(p) == P for p in passes)
        assert [(i, t) for p in passes for i, t, l in p if l] == want       # each window once, images in order, tiles row-major
        assert all(l for p in passes[:-1] for _, _, l in p)                 # filler only in the last pass ...
        k = len(want) - (len(passes) - 1) * P
        assert all(l for _, _, l in passes[-1][:k])
        assert all(w == (want[-1][0], want[-1][1], 0) for w in passes[-1][k:])   # ... and it is the group's last window
        total += len(passes)
    return total


def test_planner_counts_for_mixed_sizes(monkeypatch):
    monkeypatch.delenv('ESR_X8_SLOTS', raising=False)
    # tile 16, pad 4: 24 x 24 windows of images 0, 1, 2, 4 (4 + 12 + 15 + 4 = 35, square: 8 slots, P = 2: 18 passes, one
    # filler window), 21 x 24 windows of image 3 (2 x 3 = 6, non-square: 4 slots, P = 4: 2 passes, two filler windows)
    groups = F.tiled_many_x8_passes(SIZES, 16, 4)
    assert [(th, tw, s, P, len(p)) for th, tw, s, P, p in groups] == [(24, 24, 8, 2, 18), (21, 24, 4, 4, 2)]
    assert _check_plan(SIZES, 16, 4, 16, None, groups) == 20
    assert groups[0][4][1] == ((0, 2, 1), (0, 3, 1)) and groups[0][4][2] == ((1, 0, 1), (1, 1, 1))
    assert groups[0][4][-1] == ((4, 3, 1), (4, 3, 0))
    assert groups[1][4] == [((3, 0, 1), (3, 1, 1), (3, 2, 1), (3, 3, 1)), ((3, 4, 1), (3, 5, 1), (3, 5, 0), (3, 5, 0))]
    # tile 32, pad 8: 24 x 24 whole images (2 windows: a group smaller than P = 16 // 4 at 4 slots), 40 x 48, 33 x 48,
    # 21 x 37 non-square
    groups = F.tiled_many_x8_passes(SIZES, 32, 8, 16, 4)
    assert [(th, tw, s, P, len(p)) for th, tw, s, P, p in groups] == [(24, 24, 4, 2, 1), (40, 48, 4, 4, 1), (33, 48, 4, 4, 2),
                                                                      (21, 37, 4, 2, 1)]
    assert _check_plan(SIZES, 32, 8, 16, 4, groups) == 5
    assert sum(l == 0 for g in groups for p in g[4] for _, _, l in p) == 2          # 6 windows of 33 x 48 in 2 passes of 4
    # windows_per_pass below the slots: one window per pass, never none
    for wpp in (1, 3, 7):
        groups = F.tiled_many_x8_passes(SIZES, 16, 4, wpp)
        assert [(s, P, len(p)) for _, _, s, P, p in groups] == [(8, 1, 35), (4, 1, 6)]
        assert _check_plan(SIZES, 16, 4, wpp, None, groups) == 41
    for spp in (8, 4, 2, 1):
        for wpp in (16, 5, 64):
            _check_plan(SIZES, 16, 4, wpp, spp, F.tiled_many_x8_passes(SIZES, 16, 4, wpp, spp))
    # 16 single-window square images (tile >= the image) at the default pass: 8 passes of 2 windows x 8 slots, where the
    # per-image loop runs 16 passes of 1 x 8; at tile 96 a 128 x 128 image has four windows of 128 x 128
    assert [(s, P, len(p)) for _, _, s, P, p in F.tiled_many_x8_passes([(128, 128)] * 16, 128, 0)] == [(8, 2, 8)]
    assert [(s, P, len(p)) for _, _, s, P, p in F.tiled_many_x8_passes([(128, 128)] * 16, 96, 16)] == [(8, 2, 32)]
    assert F.tiled_many_x8_passes([], 16, 4) == []


def test_planner_refusals():
    for bad in (dict(tile=0), dict(pad=-1), dict(windows_per_pass=0), dict(tile=2.5), dict(tile=True)):
        with pytest.raises(ValueError, match='of a tiled forward must be an int >='):
            F.tiled_many_x8_passes(SIZES, **dict(dict(tile=16, pad=4), **bad))
    for spp in (0, 3, 16, -1, True, 'a'):
        with pytest.raises(ValueError, match='slots per pass'):
            F.tiled_many_x8_passes(SIZES, 16, 4, 16, spp)
    with pytest.raises(ValueError, match='no pixels'):
        F.tiled_many_x8_passes([(0, 4)], 16, 4)
    with pytest.raises(ValueError, match='65535'):
        F.tiled_many_x8_passes([(300, 300)], 1, 0, 8 * 70000)


def test_lib_mirrors_the_tile_set_x8_op(tmp_path):
    from esrganplus_amd import _lib as L
    assert L.OP_TILE_SET_X8 == 21
    assert 'esr_tile_set_x8_op' in L.EXPORTS
    names = ['dtype', 'to_g32', 'C', 'tile', 'pad', 'scale', 'th', 'tw', 'n_windows', 'items', 'g32', 'slots_nchw',
             'k_begin', 'k_count', 'accumulate', 'mean_scale', 'img', 'bgr', 'acc']
    assert [f[0] for f in L.esr_tile_set_x8._fields_] == names
    # the pass-level fields lie where esr_tile_many's do
    for name in names[:12]:
        other = 'n_slots' if name == 'n_windows' else name
        assert getattr(L.esr_tile_set_x8, name).offset == getattr(L.esr_tile_many, other).offset
    assert 'tile_set_x8' in [f[0] for f in L._op_union._fields_]
    assert C.sizeof(L.esr_tile_set_x8) <= SIZEOF_ESR_OP - 8 and C.sizeof(L.esr_op) == SIZEOF_ESR_OP
    # size, offsets and the enum value against the header compiled as C
    hdr = os.path.join(ROOT, 'include', 'esrgan_hip.h')
    prints = ['printf("kind %d\\n", (int)ESR_OP_TILE_SET_X8);', 'printf("sizeof %zu\\n", sizeof(esr_tile_set_x8));',
              'printf("op %zu\\n", sizeof(esr_op));', 'printf("item %zu\\n", sizeof(esr_tile_item));']
    prints += ['printf("%s %%zu\\n", offsetof(esr_tile_set_x8, %s));' % (n, n) for n in names]
    src = tmp_path / 'sx8.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void){%s return 0;}\n' % (hdr, '\n'.join(prints)))
    exe = tmp_path / 'sx8'
    subprocess.check_call(['gcc', '-std=c99', str(src), '-o', str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got['kind']) == 21 and int(got['sizeof']) == C.sizeof(L.esr_tile_set_x8)
    assert int(got['op']) == SIZEOF_ESR_OP and int(got['item']) == 24 == F._tile_item_dtype().itemsize
    for n in names:
        assert int(got[n]) == getattr(L.esr_tile_set_x8, n).offset, n
    lib = L.lib()                                             # loads the library: symbol present, sizeof(esr_op) agrees
    assert lib.esr_abi_version() == 6
    assert lib.esr_sizeof_op() == SIZEOF_ESR_OP
    assert hasattr(lib, 'esr_tile_set_x8_op')


def test_engine_registers_the_ends():
    from esrganplus_amd import _lib as L
    from esrganplus_amd import engine as E
    assert E.ENDS_OF_KIND[L.OP_TILE_SET_X8] is E.TileSetX8Ends and issubclass(E.TileSetX8Ends, E.TileManyEnds)
    assert (E.TileSetX8Ends.field, E.TileSetX8Ends.ptr, E.TileSetX8Ends.struct) == ('tile_set_x8', 'items', L.esr_tile_set_x8)
    assert set(E.TileSetX8Ends.per_run) == {'tile', 'pad', 'bgr', 'k_begin', 'accumulate', 'scale'}
    assert E.TileSetX8Ends.per_run['scale'] == (None, 'mean_scale') and E.TileSetX8Ends.per_run['accumulate'] == (None, 'accumulate')


class _Net:
    """What the entry functions read of a net before they touch a device."""
    in_nc, out_nc, upscale = 3, 3, 4


def test_refusals_that_need_no_device():
    x = torch.zeros(3, 13, 21)
    u = torch.zeros(13, 21, 3, dtype=torch.uint8)
    many = lambda images, net=None, **kw: F.run_rrdbnet_tiled_many_x8(net or _Net(), images, **kw)
    imgs = lambda images, net=None, **kw: F.run_rrdbnet_images(net or _Net(), images, **kw)
    evalu = lambda lr, hr, net=None, **kw: F.run_rrdbnet_evaluate(net or _Net(), lr, hr, **kw)
    assert many([]) == [] and imgs([], x8=True) == [] and imgs([], x8=True, slots_per_pass=2) == []
    for spp in (0, 3, 16, True, 'a', 2.5):                                 # slots_per_pass outside {8, 4, 2, 1}
        with pytest.raises(ValueError, match='slots per pass'):
            many([x], slots_per_pass=spp)
        with pytest.raises(ValueError, match='slots per pass'):
            imgs([u], x8=True, slots_per_pass=spp)
        with pytest.raises(ValueError, match='slots per pass'):
            evalu([u], [u], x8=True, slots_per_pass=spp)
    for call in (lambda: imgs([u], slots_per_pass=4), lambda: imgs([], slots_per_pass=4),
                 lambda: evalu([u], [u], slots_per_pass=4), lambda: imgs([u], x8=False, slots_per_pass=8)):
        with pytest.raises(ValueError, match='pass x8=True'):              # slots_per_pass without x8
            call()
    for bad in (dict(tile=0), dict(pad=-1), dict(windows_per_pass=0), dict(tile=2.5)):
        with pytest.raises(ValueError, match='of a tiled forward must be an int >='):
            many([x], **bad)
        with pytest.raises(ValueError, match='of a tiled forward must be an int >='):
            imgs([u], x8=True, **bad)
    with pytest.raises(ValueError, match='no CPU fallback'):               # CPU tensors
        many([x])
    with pytest.raises(ValueError, match='no CPU fallback'):
        imgs([u], x8=True)
    with pytest.raises(ValueError, match='no CPU fallback'):
        many([torch.zeros(3, 13, 21, device='meta')], slots_per_pass=2)
    with pytest.raises(ValueError, match='one device'):                    # mixed devices
        many([x, torch.zeros(3, 13, 21, device='meta')])
    with pytest.raises(ValueError, match='one device'):
        imgs([u, torch.zeros(13, 21, 3, dtype=torch.uint8, device='meta')], x8=True)
    for nc in ((1, 3), (3, 1), (4, 4)):                                    # the uint8 form is 3 channels in and out
        net = _Net()
        net.in_nc, net.out_nc = nc
        with pytest.raises(ValueError, match='in_nc'):
            imgs([u], net, x8=True)
    with pytest.raises(ValueError, match='input channels'):
        many([torch.zeros(4, 13, 21)])
    with pytest.raises(ValueError, match='uint8'):
        imgs([x], x8=True)
    with pytest.raises(ValueError, match='must be a'):
        many([torch.zeros(2, 3, 13, 21)])
    with pytest.raises(ValueError, match='65535'):
        many([torch.zeros(3, 256, 257, device='meta')], tile=1, pad=0, windows_per_pass=8 * 70000)


def test_modules_refuse_before_a_plan_exists():
    from esrganplus_amd import architecture as arch
    x = torch.zeros(3, 13, 21)
    u = torch.zeros(13, 21, 3, dtype=torch.uint8)
    for cls in (arch.RRDBNet, arch.RRDB_Net):
        net2 = cls(3, 3, 64, 1, upscale=2)                                 # upscale != 4
        for call in (lambda: net2.forward_tiled_many_x8([x]), lambda: net2.forward_tiled_many_x8([]),
                     lambda: net2.forward_images([u], x8=True), lambda: net2.evaluate_images([u], [u], x8=True)):
            with pytest.raises(ValueError, match='x4-only'):
                call()
        wide = cls(9, 9, 64, 1)                                            # more than 8 channels
        with pytest.raises(ValueError, match='at most 8 image channels'):
            wide.forward_tiled_many_x8([torch.zeros(9, 13, 21)])
        with pytest.raises(ValueError, match='in_nc'):
            cls(1, 1, 64, 1).forward_images([u], x8=True)
        net = cls(3, 3, 64, 1)
        assert net.forward_tiled_many_x8([]) == [] and net.forward_images([], x8=True) == []
        with pytest.raises(ValueError, match='no CPU fallback'):
            net.forward_tiled_many_x8([x])
        with pytest.raises(ValueError, match='no CPU fallback'):
            net.forward_images([u], x8=True, slots_per_pass=4)
        with pytest.raises(ValueError, match='slots per pass'):
            net.forward_tiled_many_x8([x], slots_per_pass=3)
        with pytest.raises(ValueError, match='pass x8=True'):
            net.forward_images([u], slots_per_pass=4)
        with pytest.raises(ValueError, match='pass x8=True'):
            net.evaluate_images([u], [torch.zeros(52, 84, 3, dtype=torch.uint8)], slots_per_pass=4)
        assert not net._plans and not net2._plans and not wide._plans


def test_train_steps_take_x8():
    import inspect
    from esrganplus_amd import train as T
    steps = [c for c in vars(T).values() if inspect.isclass(c) and 'validate' in vars(c)]
    assert len(steps) == 3
    for c in steps:
        assert inspect.signature(c.validate).parameters['x8'].default is False


def _conv_stack(seed=5):
    """A small x4 torch forward that is neither symmetric under the eight transforms nor local to a pixel."""
    g = torch.Generator().manual_seed(seed)
    w1, w2 = torch.randn(6, 3, 3, 3, generator=g) * 0.3, torch.randn(3, 6, 3, 3, generator=g) * 0.3

    def fn(t):
        h = torch.nn.functional.leaky_relu(torch.nn.functional.conv2d(t, w1, padding=1), 0.2)
        h = torch.nn.functional.interpolate(h, scale_factor=4, mode='nearest')
        return torch.nn.functional.conv2d(h, w2, padding=1) + 0.5
    return fn


def _per_sample(fn):
    """fn run one sample at a time: the CPU convolution may pick its algorithm by the batch, and these tests compare
    bits between different batchings."""
    return lambda t: torch.cat([fn(t[i:i + 1]) for i in range(t.shape[0])], 0)


@pytest.mark.parametrize('spp', [None, 2])
def test_references_agree_with_x8_reference_when_a_tile_is_the_image(spp, monkeypatch):
    monkeypatch.delenv('ESR_X8_SLOTS', raising=False)
    fn = _per_sample(_conv_stack())
    g = torch.Generator().manual_seed(3)
    xs = [torch.rand(3, H, W, generator=g) for H, W in [(9, 9), (7, 12), (12, 7), (9, 9)]]
    xs[1] = xs[1][None]                                                    # ranks are kept
    got = F.tiled_many_x8_reference(fn, xs, 16, 0, 16, spp)
    assert len(got) == 4 and [y.dim() for y in got] == [3, 4, 3, 3]
    for x, y in zip(xs, got):
        want = F.x8_reference(fn, x if x.dim() == 4 else x[None])
        assert y.dtype == torch.float32 and torch.equal(y if y.dim() == 4 else y[None], want)
    # and a tiled set equals the tiled self-ensemble per image (one window per pass on both sides)
    got = F.tiled_many_x8_reference(fn, xs, 4, 2, 1, spp)
    for x, y in zip(xs, got):
        want = F.tiled_x8_reference(fn, x if x.dim() == 4 else x[None], 4, 2, 1, spp)
        assert torch.equal(y if y.dim() == 4 else y[None], want)


@pytest.mark.parametrize('bgr', [False, True])
def test_images_x8_reference_is_the_quantisation_of_the_float_reference(bgr):
    fn = _per_sample(_conv_stack())
    g = torch.Generator().manual_seed(4)
    imgs = [torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8) for H, W in [(9, 9), (7, 12), (10, 13)]]
    got = F.images_x8_reference(fn, imgs, 4, 2, 6, None, bgr)
    lut = torch.arange(256, dtype=torch.float32) / 255.0
    xs = [lut[(x.flip(2) if bgr else x).permute(2, 0, 1).long()] for x in imgs]
    ys = F.tiled_many_x8_reference(fn, xs, 4, 2, 6)
    lo = hi = 0
    for x, y, o in zip(imgs, ys, got):
        want = (y.clamp(0, 1) * 255.0).round().to(torch.uint8).permute(1, 2, 0)
        want = want.flip(2) if bgr else want
        assert o.dtype == torch.uint8 and tuple(o.shape) == (4 * x.shape[0], 4 * x.shape[1], 3) and o.is_contiguous()
        assert torch.equal(o, want)
        lo, hi = lo + int((y < 0).sum()), hi + int((y > 1).sum())
    assert lo and hi                                                       # the clamp is exercised on both sides
    other = F.images_x8_reference(fn, imgs, 4, 2, 6, None, not bgr)
    assert any(not torch.equal(a, b) for a, b in zip(got, other))
    plain = F.images_reference(fn, imgs, 4, 2, 6, bgr)
    assert any(not torch.equal(a, b) for a, b in zip(got, plain))          # the ensemble is not the single forward
