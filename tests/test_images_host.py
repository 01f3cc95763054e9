"""8-bit image-in, image-out inference, host side: the bits of the input conversion, the pure-torch ``images_reference``
against a direct per-image computation in both channel orders, the refusals that need no device, and the ctypes mirror
of the new op (include/esrgan_hip.h: esr_tile_img)."""
import ctypes as C

import numpy as np
import pytest
import torch

from esrganplus_amd import functional as F

SIZES = [(40, 52), (33, 70), (13, 21), (16, 16)]
SIZEOF_ESR_OP = 552          # the union must not grow
# per channel a x + b on x in [0, 1]: R runs from below 0 to above 1, G stays inside, B from above 1 to below 0
A, B_ = (1.5, 0.75, -1.625), (-0.25, 0.125, 1.3125)


def _u8_images(seed, sizes):
    """Seeded uint8 HWC images that contain all 256 values."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for H, W in sizes:
        x = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
        x.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)
        out.append(x)
    return out


def _affine_fn(t):
    """Nearest x4 of a_c x + b_c: per pixel and per sample, so neither the batch nor the window can matter."""
    a, b = torch.tensor(A).view(1, 3, 1, 1), torch.tensor(B_).view(1, 3, 1, 1)
    return torch.nn.functional.interpolate(t * a + b, scale_factor=4, mode='nearest')


def test_the_input_conversion_is_the_scripts_float64_division_bit_for_bit():
    v = np.arange(256, dtype=np.uint8)
    want = torch.from_numpy(v.astype(np.float64) / 255).float()
    seen = []

    def fn(t):
        seen.append(t.clone())
        return torch.nn.functional.interpolate(t, scale_factor=4, mode='nearest')

    img = torch.from_numpy(v).view(16, 16, 1).repeat(1, 1, 3).contiguous()
    out = F.images_reference(fn, [img], 16, 0)
    assert len(seen) == 1 and seen[0].dtype == torch.float32 and tuple(seen[0].shape) == (1, 3, 16, 16)
    for c in range(3):
        assert torch.equal(seen[0][0, c].reshape(-1).view(torch.int32), want.view(torch.int32))
    # what the kernel is told NOT to do differs for 126 of the 256 values
    recip = torch.from_numpy(v).float() * torch.tensor(1.0 / 255, dtype=torch.float32)
    assert int((recip.view(torch.int32) != want.view(torch.int32)).sum()) == 126
    # and x / 255 -> x 255, round is the identity on bytes
    assert torch.equal(out[0][::4, ::4], img)


@pytest.mark.parametrize('bgr', [False, True])
def test_images_reference_equals_the_direct_per_image_computation(bgr):
    imgs = _u8_images(7, SIZES)
    got = F.images_reference(_affine_fn, imgs, 16, 4, 5, bgr=bgr)
    assert len(got) == len(imgs)
    lo = mid = hi = 0
    for x, y in zip(imgs, got):
        rgb = torch.from_numpy(x.numpy()[:, :, ::-1].copy()) if bgr else x
        f = torch.from_numpy(np.transpose(rgb.numpy().astype(np.float64) / 255, (2, 0, 1))).float().unsqueeze(0)
        v = _affine_fn(f)[0]
        lo, mid, hi = lo + int((v < 0).sum()), mid + int(((v > 0) & (v < 1)).sum()), hi + int((v > 1).sum())
        want = (v.clamp(0, 1) * 255.0).round().to(torch.uint8).permute(1, 2, 0)
        want = want.flip(2) if bgr else want
        assert y.dtype == torch.uint8 and tuple(y.shape) == (4 * x.shape[0], 4 * x.shape[1], 3) and y.is_contiguous()
        assert torch.equal(y, want)
    assert lo and mid and hi                                  # below 0, inside and above 1: the clamp is exercised
    other = F.images_reference(_affine_fn, imgs, 16, 4, 5, bgr=not bgr)
    assert any(not torch.equal(a, b) for a, b in zip(got, other))       # the channel order matters


class _Net:
    """What ``run_rrdbnet_images`` reads of a net before it touches a device."""
    in_nc, out_nc = 3, 3


def test_refusals_that_need_no_device():
    x = torch.zeros(13, 21, 3, dtype=torch.uint8)
    run = lambda images, net=None, **kw: F.run_rrdbnet_images(net or _Net(), images, **kw)
    for bad in (dict(tile=0), dict(pad=-1), dict(windows_per_pass=0), dict(tile=2.5), dict(pad=None), dict(tile=True)):
        with pytest.raises(ValueError, match='of a tiled forward must be an int >='):
            run([x], **bad)
    assert run([]) == [] and run(()) == []
    for images in ([x.float()], [x.to(torch.int8)], [None], [x.numpy()]):                 # dtype
        with pytest.raises(ValueError, match='uint8'):
            run(images)
    for images in ([x[0]], [x[None]], [x, torch.zeros(13, 21, dtype=torch.uint8)]):       # rank
        with pytest.raises(ValueError, match='rank'):
            run(images)
    for images in ([x[:, :, :1]], [torch.zeros(13, 21, 4, dtype=torch.uint8)], [x.permute(2, 0, 1)]):
        with pytest.raises(ValueError, match='last dimension'):
            run(images)
    for nc in ((1, 3), (3, 1), (4, 4)):
        net = _Net()
        net.in_nc, net.out_nc = nc
        with pytest.raises(ValueError, match='in_nc'):
            run([x], net)
    for images in ([x[:0]], [x, x[:, :0]]):
        with pytest.raises(ValueError, match='no pixels'):
            run(images)
    with pytest.raises(ValueError, match='one device'):
        run([x, torch.zeros(13, 21, 3, dtype=torch.uint8, device='meta')])
    with pytest.raises(ValueError, match='no CPU fallback'):
        run([x])
    with pytest.raises(ValueError, match='no CPU fallback'):
        run([torch.zeros(13, 21, 3, dtype=torch.uint8, device='meta')])
    with pytest.raises(ValueError, match='65535'):
        run([torch.zeros(256, 257, 3, dtype=torch.uint8, device='meta')], tile=1, pad=0, windows_per_pass=70000)
    for images in ([x.float()], [x[0]], [x[:, :, :1]], [x[:0]]):                          # the restatement refuses alike
        with pytest.raises(ValueError):
            F.images_reference(_affine_fn, images, 8, 2)


def test_other_scales_are_refused_before_anything_else():
    from esrganplus_amd import architecture as arch
    x = torch.zeros(13, 21, 3, dtype=torch.uint8)
    for cls in (arch.RRDBNet, arch.RRDB_Net):
        net = cls(3, 3, 64, 1, upscale=2)
        for images in ([x], [], [x.float()]):
            with pytest.raises(ValueError, match='x4-only'):
                net.forward_images(images)
        net4 = cls(3, 3, 64, 1)
        assert net4.forward_images([]) == []
        with pytest.raises(ValueError, match='no CPU fallback'):
            net4.forward_images([x])
        with pytest.raises(ValueError, match='no CPU fallback'):
            net4.forward_images([x], bgr=True)
        with pytest.raises(ValueError, match='must be an int'):
            net4.forward_images([x], windows_per_pass=0)
        with pytest.raises(ValueError, match='uint8'):
            net4.forward_images([x.float()])
        with pytest.raises(ValueError, match='in_nc'):
            cls(1, 1, 64, 1).forward_images([x])
        assert not net4._plans


def test_lib_mirrors_the_tile_img_op():
    from esrganplus_amd import _lib as L
    assert L.OP_TILE_IMG == 20
    assert 'esr_tile_img_op' in L.EXPORTS
    assert [f[0] for f in L.esr_tile_img._fields_] == ['dtype', 'to_g32', 'C', 'tile', 'pad', 'scale', 'th', 'tw', 'n_slots',
                                                       'items', 'g32', 'slots_nchw', 'bgr']
    assert [f[0] for f in L.esr_tile_img_item._fields_] == ['hwc', 'H', 'W', 't', 'live']
    assert C.sizeof(L.esr_tile_img_item) == 24 == C.sizeof(L.esr_tile_item) == F._tile_item_dtype().itemsize
    for name in ('hwc', 'H', 'W', 't', 'live'):              # the shared table builder writes esr_tile_item's offsets
        other = 'nchw' if name == 'hwc' else name
        assert getattr(L.esr_tile_img_item, name).offset == getattr(L.esr_tile_item, other).offset
    assert 'tile_img' in [f[0] for f in L._op_union._fields_]
    assert C.sizeof(L.esr_op) == SIZEOF_ESR_OP
    lib = L.lib()                                             # loads the library: symbol present, sizeof(esr_op) agrees
    assert lib.esr_abi_version() == 6
    assert lib.esr_sizeof_op() == SIZEOF_ESR_OP
    assert hasattr(lib, 'esr_tile_img_op')
