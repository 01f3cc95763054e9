"""Scoring from HR images alone, host side: ``functional.hr_lr_reference`` against the reference dataset's own ``LR`` and
``HR`` tensors (tests/golden/hr_val.npz, tools/gen_hr_val_golden.py), the bound on the source columns an LDS row of the
gather must hold, the refusals that need no device, and the ctypes mirror of the new op (include/esrgan_hip.h:
esr_tile_hr) against the header compiled as C."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from esrganplus_amd import data as D
from esrganplus_amd import functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZEOF_ESR_OP = 552          # C.sizeof(_lib.esr_op) of the parent commit: the union must not grow
SIZES = [(55, 86), (52, 240), (64, 64)]


def _images(golden):
    g = golden('hr_val')
    assert int(g['n_images']) == 3
    imgs = [torch.from_numpy(g['img%d' % k]) for k in range(3)]
    assert [tuple(x.shape) for x in imgs] == [s + (3,) for s in SIZES] and all(x.dtype == torch.uint8 for x in imgs)
    return g, imgs


def test_reference_lr_and_hr_against_the_reference_dataset(golden):
    """The generated LR within 2e-6 — the bound tests/test_batch_host.py holds the generated LR of batch_assemble.npz
    to — and the cropped HR bit for bit.  The fixture's images are cv2's (B, G, R); the dataset's tensors are R, G, B."""
    g, imgs = _images(golden)
    lrs, hrs = F.hr_lr_reference(imgs, bgr=True)
    for k, (H, W) in enumerate(SIZES):
        assert tuple(hrs[k].shape) == (3, H - H % 4, W - W % 4) and tuple(lrs[k].shape) == (3, H // 4, W // 4)
        assert hrs[k].dtype == lrs[k].dtype == torch.float32
        assert np.array_equal(hrs[k].numpy(), g['HR%d' % k]), k
        d = float(np.abs(lrs[k].numpy() - g['LR%d' % k]).max())
        print('image %d: LR max difference to the reference %.3e' % (k, d))
        assert d <= 2e-6, (k, d)
    # the other channel order is the other picture, and a stored LR is another LR: the dataset's is not 8-bit
    other, _ = F.hr_lr_reference(imgs, bgr=False)
    assert not torch.equal(other[2], lrs[2]) and torch.equal(other[2].flip(0), lrs[2])
    assert float(((lrs[2] * 255).round() / 255 - lrs[2]).abs().max()) > 1e-4


def test_hr_images_reference_is_the_image_route_on_the_dataset_lr(golden):
    """With a x4 torch forward: tiled_many_reference on hr_lr_reference's LR, quantised as images_reference does."""
    _, imgs = _images(golden)
    gen = torch.Generator().manual_seed(5)
    w1, w2 = torch.randn(6, 3, 3, 3, generator=gen) * 0.3, torch.randn(3, 6, 3, 3, generator=gen) * 0.3

    def fn(t):
        h = torch.nn.functional.leaky_relu(torch.nn.functional.conv2d(t, w1, padding=1), 0.2)
        h = torch.nn.functional.interpolate(h, scale_factor=4, mode='nearest')
        return torch.cat([torch.nn.functional.conv2d(h[i:i + 1], w2, padding=1) + 0.5 for i in range(h.shape[0])], 0)
    for bgr in (False, True):
        got = F.hr_images_reference(fn, imgs, 8, 3, 5, bgr)
        lrs, _ = F.hr_lr_reference(imgs, bgr)
        ys = F.tiled_many_reference(fn, lrs, 8, 3, 5)
        for (H, W), o, y in zip(SIZES, got, ys):
            want = (y.clamp(0, 1) * 255.0).round().to(torch.uint8).permute(1, 2, 0)
            assert o.dtype == torch.uint8 and tuple(o.shape) == (4 * (H // 4), 4 * (W // 4), 3) and o.is_contiguous()
            assert torch.equal(o, want.flip(2) if bgr else want)
    assert F.hr_images_reference(fn, [], 8, 3) == []


def test_span_of_sixteen_lr_columns_fits_the_lds_row():
    """Every HR length 4 ... 1600 in steps of 4 and every start x0 of 16 consecutive LR columns, the last partial group
    included: the source columns ``resample_tables(n, 0.25)`` names span at most the kernel's LDS row (_lib.TILE_HR_SPAN
    = ESR_TILE_HR_SPAN of the header, which test_lib_mirrors_the_tile_hr_op reads back from C)."""
    from esrganplus_amd import _lib as L
    assert L.TILE_HR_SPAN == 15 * 4 + 17
    worst = taps_max = 0
    for n in range(4, 1604, 4):
        w, idx, out_len = D.resample_tables(n, 0.25)
        assert out_len == n // 4 and tuple(idx.shape) == tuple(w.shape) == (out_len, w.shape[1])
        taps_max = max(taps_max, w.shape[1])
        idx = idx.numpy()
        assert idx.min() >= 0 and idx.max() < n
        lo, hi = idx.min(axis=1), idx.max(axis=1)
        for x0 in range(out_len):                      # the kernel's groups start at any window column
            span = int(hi[x0:x0 + 16].max() - lo[x0:x0 + 16].min()) + 1
            worst = max(worst, span)
            assert span <= L.TILE_HR_SPAN, (n, x0, span)
    print('taps at x4: at most %d; widest span of 16 LR columns: %d of %d' % (taps_max, worst, L.TILE_HR_SPAN))
    assert taps_max <= 17 and worst > 60


def test_lib_mirrors_the_tile_hr_op(tmp_path):
    from esrganplus_amd import _lib as L
    assert L.OP_TILE_HR == 22
    assert 'esr_tile_hr_op' in L.EXPORTS
    names = [f[0] for f in L.esr_tile_img._fields_]
    assert [f[0] for f in L.esr_tile_hr._fields_] == names
    for n in names:
        assert getattr(L.esr_tile_hr, n).offset == getattr(L.esr_tile_img, n).offset
    assert [f[0] for f in L.esr_tile_hr_item._fields_] == ['ptr', 'H', 'W', 't', 'live']
    assert C.sizeof(L.esr_tile_hr_item) == 24 == C.sizeof(L.esr_tile_item) == F._tile_item_dtype().itemsize
    for name, other in (('ptr', 'nchw'), ('H', 'H'), ('W', 'W'), ('t', 't'), ('live', 'live')):
        assert getattr(L.esr_tile_hr_item, name).offset == getattr(L.esr_tile_item, other).offset
    dnames = [f[0] for f in L.esr_tile_hr_desc._fields_]
    assert dnames == ['hr', 'wy', 'iy', 'wx', 'ix', 'pitch', 'hr_h', 'hr_w', 'taps_y', 'taps_x', '_pad']
    assert C.sizeof(L.esr_tile_hr_desc) == 64 == F._hr_desc_dtype().itemsize
    assert all(F._hr_desc_dtype().fields[n][1] == getattr(L.esr_tile_hr_desc, n).offset for n in dnames)
    assert 'tile_hr' in [f[0] for f in L._op_union._fields_]
    assert C.sizeof(L.esr_tile_hr) <= SIZEOF_ESR_OP - 8 and C.sizeof(L.esr_op) == SIZEOF_ESR_OP
    # sizes, offsets, the enum value and the LDS constant against the header compiled as C
    hdr = os.path.join(ROOT, 'include', 'esrgan_hip.h')
    prints = ['printf("kind %d\\n", (int)ESR_OP_TILE_HR);', 'printf("sizeof %zu\\n", sizeof(esr_tile_hr));',
              'printf("op %zu\\n", sizeof(esr_op));', 'printf("item %zu\\n", sizeof(esr_tile_hr_item));',
              'printf("desc %zu\\n", sizeof(esr_tile_hr_desc));', 'printf("span %d\\n", (int)ESR_TILE_HR_SPAN);']
    prints += ['printf("%s %%zu\\n", offsetof(esr_tile_hr, %s));' % (n, n) for n in names]
    prints += ['printf("d_%s %%zu\\n", offsetof(esr_tile_hr_desc, %s));' % (n, n) for n in dnames]
    src = tmp_path / 'thr.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void){%s return 0;}\n' % (hdr, '\n'.join(prints)))
    exe = tmp_path / 'thr'
    subprocess.check_call(['gcc', '-std=c99', str(src), '-o', str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got['kind']) == 22 and int(got['sizeof']) == C.sizeof(L.esr_tile_hr)
    assert int(got['op']) == SIZEOF_ESR_OP and int(got['item']) == 24 and int(got['desc']) == 64
    assert int(got['span']) == L.TILE_HR_SPAN
    for n in names:
        assert int(got[n]) == getattr(L.esr_tile_hr, n).offset, n
    for n in dnames:
        assert int(got['d_' + n]) == getattr(L.esr_tile_hr_desc, n).offset, n
    lib = L.lib()                                             # loads the library: symbol present, sizeof(esr_op) agrees
    assert lib.esr_abi_version() == 6
    assert lib.esr_sizeof_op() == SIZEOF_ESR_OP
    assert hasattr(lib, 'esr_tile_hr_op')


def test_engine_registers_the_ends():
    from esrganplus_amd import _lib as L
    from esrganplus_amd import engine as E
    assert E.ENDS_OF_KIND[22] is E.TileHrEnds and E.ENDS_OF_KIND[L.OP_TILE_HR] is E.TileHrEnds
    assert issubclass(E.TileHrEnds, E.TileImgEnds)
    assert (E.TileHrEnds.kind, E.TileHrEnds.field, E.TileHrEnds.ptr, E.TileHrEnds.struct) == (22, 'tile_hr', 'items', L.esr_tile_hr)
    assert set(E.TileHrEnds.per_run) == {'tile', 'pad', 'bgr'}
    assert E.ENDS_OF_KIND[L.OP_TILE_IMG] is E.TileImgEnds                     # the sibling keeps its place


class _Net:
    """What the entry functions read of a net before they touch a device."""
    in_nc, out_nc, upscale = 3, 3, 4


def test_refusals_that_need_no_device():
    u = torch.zeros(52, 84, 3, dtype=torch.uint8)
    run = lambda images, net=None, **kw: F.run_rrdbnet_hr_images(net or _Net(), images, **kw)
    evalu = lambda images, net=None, **kw: F.run_rrdbnet_evaluate_hr(net or _Net(), images, **kw)
    assert run([]) == [] and run(()) == []
    for call in (run, evalu):
        for bad in ([u.float()], [u[0]], [u[:, :, :2]], [u[:0]], [u.numpy()]):            # what _images_u8 refuses
            with pytest.raises(ValueError, match='of forward_images must be|no pixels'):
                call(bad)
        for small in (u[:3], u[:, :3], u[:3, :3]):                                         # an HR side below 4
            with pytest.raises(ValueError, match='hr image 1 .*below 4'):
                call([u, small])
        for nc in ((1, 3), (3, 1), (4, 4)):                                                # nets that are not 3 -> 3
            net = _Net()
            net.in_nc, net.out_nc = nc
            with pytest.raises(ValueError, match='in_nc'):
                call([u], net)
        with pytest.raises(ValueError, match='one device'):                                # more than one device
            call([u, torch.zeros(52, 84, 3, dtype=torch.uint8, device='meta')])
        with pytest.raises(ValueError, match='no CPU fallback'):                           # CPU tensors
            call([u])
        with pytest.raises(ValueError, match='no CPU fallback'):
            call([torch.zeros(52, 84, 3, dtype=torch.uint8, device='meta')])
        for kw in (dict(tile=0), dict(pad=-1), dict(windows_per_pass=0), dict(tile=2.5), dict(tile=True)):
            with pytest.raises(ValueError, match='of a tiled forward must be an int >='):
                call([u], **kw)
        with pytest.raises(TypeError):                                                     # no x8 on this route
            call([u], x8=True)
    for crop in (-1, 2.5, True, 26):                                                       # 52 - 2 * 26 leaves nothing
        with pytest.raises(ValueError, match='crop'):
            evalu([u], crop=crop)
    with pytest.raises(ValueError, match='65535'):
        run([torch.zeros(1024, 1028, 3, dtype=torch.uint8, device='meta')], tile=1, pad=0, windows_per_pass=70000)


def test_modules_refuse_before_a_plan_exists():
    from esrganplus_amd import architecture as arch
    u = torch.zeros(52, 84, 3, dtype=torch.uint8)
    for cls in (arch.RRDBNet, arch.RRDB_Net):
        net2 = cls(3, 3, 64, 1, upscale=2)                                 # upscale != 4
        for call in (lambda: net2.forward_hr_images([u]), lambda: net2.forward_hr_images([]),
                     lambda: net2.evaluate_hr_images([u]), lambda: net2.evaluate_hr_images([])):
            with pytest.raises(ValueError, match='x4-only'):
                call()
        with pytest.raises(ValueError, match='in_nc'):
            cls(1, 1, 64, 1).forward_hr_images([u])
        net = cls(3, 3, 64, 1)
        assert net.forward_hr_images([]) == [] and net.forward_hr_images(()) == []
        with pytest.raises(ValueError, match='no CPU fallback'):
            net.forward_hr_images([u])
        with pytest.raises(ValueError, match='no CPU fallback'):
            net.evaluate_hr_images([u], 8, 3)
        with pytest.raises(ValueError, match='below 4'):
            net.forward_hr_images([u[:2]])
        with pytest.raises(TypeError):
            net.forward_hr_images([u], x8=True)
        assert not net._plans and not net2._plans


def test_train_steps_have_validate_hr():
    import inspect
    from esrganplus_amd import train as T
    steps = [c for c in vars(T).values() if inspect.isclass(c) and 'validate_hr' in vars(c)]
    assert sorted(c.__name__ for c in steps) == ['ESRGANPlusStep', 'PSNRStep', 'SRGANStep']
    for c in steps:
        assert list(inspect.signature(c.validate_hr).parameters)[:2] == ['self', 'hr_images']
        assert 'x8' not in inspect.signature(c.validate_hr).parameters
        assert 'validate' in vars(c)                                       # the paired form stays
