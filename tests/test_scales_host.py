"""RRDBNet / RRDB_Net at upscale 1, 2, 3, 4 and 8, host side: module trees and state-dict keys against the reference's own
key lists (tests/golden/rrdbnet_scales.npz, tools/gen_scales_golden.py), the refusals, and the identity behind the x3
up-conv — nearest-x3 + 3x3 conv = folded 3x3 conv to 576 channels + 3x pixel shuffle — in fp64."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from esrganplus_amd import synth
from tests import scales_refs as SR

SCALES = (1, 2, 3, 8)


@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as ge
    ge.build()
    from esrganplus_amd import _lib
    return _lib


def _fixture_keys(g, tag):
    return [str(k) for k in g[tag + '_keys']], [tuple(int(v) for v in row if v >= 0) for row in g[tag + '_shapes']]


@pytest.mark.parametrize('s', SCALES)
def test_state_dict_keys_and_shapes_are_the_references(golden, s):
    from esrganplus_amd import architecture as arch
    g = golden('rrdbnet_scales')
    keys, shapes = _fixture_keys(g, 'x%d' % s)
    net = arch.RRDBNet(3, 3, 64, int(g['nb']), upscale=s)
    sd = net.state_dict()
    assert list(sd.keys()) == keys
    assert [tuple(v.shape) for v in sd.values()] == shapes
    sy = synth.rrdbnet_state_dict(int(g['nb']), upscale=s)
    assert list(sy.keys()) == keys and [tuple(v.shape) for v in sy.values()] == shapes
    r = net.load_state_dict(sy, strict=True)
    assert not r.missing_keys and not r.unexpected_keys
    # what the plans derive from the module tree: the conv list in state-dict order, the up-convs
    assert [k for k, _, _ in net._conv_list()] == [k for k, *_ in synth.rrdbnet_keys(int(g['nb']), upscale=s)]
    n_up = {1: 0, 2: 1, 3: 1, 8: 3}[s]
    assert len(net._up_keys()) == n_up
    assert set(net._dgrad_special()) == (set() if s == 3 else set(net._up_keys()))
    assert net._fold_keys() == (tuple(net._up_keys()) if s == 3 else ())


def test_inference_copy_at_x3_has_the_references_keys(golden):
    from esrganplus_amd import architecture as arch
    g = golden('rrdbnet_scales')
    keys, shapes = _fixture_keys(g, 'ti3')
    sd = arch.RRDB_Net(3, 3, 64, int(g['nb']), upscale=3).state_dict()
    assert list(sd.keys()) == keys and [tuple(v.shape) for v in sd.values()] == shapes


def test_default_scale_is_unchanged():
    from esrganplus_amd import architecture as arch
    assert synth.rrdbnet_keys(2) == synth.rrdbnet_keys(2, upscale=4)
    a, b = synth.rrdbnet_state_dict(1, 3, 0.5), synth.rrdbnet_state_dict(1, 3, 0.5, upscale=4)
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    net = arch.RRDBNet(3, 3, 64, 1)
    assert net.upscale == 4 and net._tail_keys() == ['model.3', 'model.6', 'model.8', 'model.10']
    assert net._dgrad_special() == {'model.3': {'ups': True}, 'model.6': {'ups': True}}


@pytest.mark.parametrize('s', [0, 5, 6, 16])
@pytest.mark.parametrize('cls', ['RRDBNet', 'RRDB_Net'])
def test_other_scales_are_refused(cls, s):
    from esrganplus_amd import architecture as arch
    with pytest.raises(NotImplementedError, match=r'\(1, 2, 3, 4, 8\)'):
        getattr(arch, cls)(3, 3, 64, 1, upscale=s)


def test_upconv_block_takes_factor_3():
    from esrganplus_amd import block as B
    m = B.upconv_blcok(64, 64, 3, act_type='leakyrelu')
    assert m[0].scale_factor == 3 and tuple(m[1].weight.shape) == (64, 64, 3, 3)
    with pytest.raises(NotImplementedError):
        B.upconv_blcok(64, 64, 4)


def test_fold_identity_fp64():
    """nearest-x3 + zero-padded 3x3 conv == zero-padded 3x3 conv 64 -> 576 on the LR grid (folded weights, bias
    replicated) + the phase-major 3x shuffle; LeakyReLU commutes with the shuffle.  5 x 7: no multiple of anything.
    Tolerance: fp64 rounding of sums of 576 products of O(1) values (both sides round differently: the folded weights
    are sums formed first)."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 64, 5, 7, dtype=torch.float64, generator=g)
    w = torch.randn(64, 64, 3, 3, dtype=torch.float64, generator=g) / 24
    b = torch.randn(64, dtype=torch.float64, generator=g)
    ref = F.conv2d(F.interpolate(x, scale_factor=3, mode='nearest'), w, b, padding=1)
    wf, bf = SR.fold3(w, b)
    assert tuple(wf.shape) == (576, 64, 3, 3) and torch.equal(bf, b.repeat(9))
    got = SR.shuffle3(F.conv2d(x, wf, bf, padding=1))
    assert tuple(got.shape) == tuple(ref.shape) == (1, 64, 15, 21)
    err = (got - ref).abs().max().item()
    print('fold identity: max|diff| %.3e (|ref| max %.3f)' % (err, ref.abs().max().item()))
    assert err <= 64 * 9 * 2.0 ** -52 * max(1.0, ref.abs().max().item())
    assert torch.equal(SR.shuffle3(F.leaky_relu(F.conv2d(x, wf, bf, padding=1), 0.2)),
                       F.leaky_relu(SR.shuffle3(F.conv2d(x, wf, bf, padding=1)), 0.2))
    # the folded conv has 25 non-zero tap-phases of 81, and every source weight lands exactly once per phase
    nz = (wf.abs().reshape(9, 64, 64, 9).amax((1, 2)) > 0).sum().item()
    assert nz == 25
    assert torch.allclose(wf.reshape(9, 64, 64, 9).sum(3), w.reshape(64, 64, 9).sum(2).expand(9, 64, 64), atol=1e-13)
    # adjoints: <fold(w), G> == <w, unfold(G)>, unshuffle3 is shuffle3's inverse
    G = torch.randn(576, 64, 3, 3, dtype=torch.float64, generator=g)
    gb = torch.randn(576, dtype=torch.float64, generator=g)
    gw, gbs = SR.unfold3(G, gb)
    assert abs((wf * G).sum().item() - (w * gw).sum().item()) <= 1e-10
    assert abs((bf * gb).sum().item() - (b * gbs).sum().item()) <= 1e-11
    z = torch.randn(2, 576, 5, 7, dtype=torch.float64, generator=g)
    assert torch.equal(SR.unshuffle3(SR.shuffle3(z)), z)


@pytest.mark.parametrize('method', ['forward_tiled', 'forward_tiled_x8'])
def test_tiled_forms_refuse_a_net_that_is_not_x4(method):
    """ValueError from Python, before the no-CPU-fallback error a CPU tensor would otherwise meet."""
    from esrganplus_amd import architecture as arch
    net = arch.RRDBNet(3, 3, 64, 1, upscale=2)
    with pytest.raises(ValueError, match='x4-only'):
        getattr(net, method)(torch.zeros(1, 3, 8, 8))


def test_buffers_past_the_32_bit_offsets_are_refused_before_allocation(built):
    """The kernels address one channel-group plane (conv_mfma.hip: goff) and, in the fp16 weight-gradient kernel, one
    image (wgrad.hip: soff / poff) with 32-bit byte offsets: engine.G32 refuses a plane — for training plans an image —
    of 2^31 bytes or more with a ValueError, before anything is allocated (device 'meta' here: nothing could be)."""
    from esrganplus_amd import engine as E
    assert E.OFFSET_LIMIT == 2 ** 31
    # x8 from 1024 x 1024 LR: one plane of the HR buffers is (8192 + 38) x (8192 + 2) x 32 bytes = 2.16e9
    with pytest.raises(ValueError, match='32-bit offsets'):
        E.G32(1, 64, 8192, 8192, 'fp16', 'meta')
    # a training plan's 64-channel fp16 HR buffer at 4096 x 4096: 4 planes of 0.54e9 bytes per image
    with pytest.raises(ValueError, match='per image'):
        E.G32(1, 64, 4096, 4096, 'fp16', 'meta', image_limit=True)
    hp, wp = built.g32_dims(4096, 4096)
    assert hp * wp * 32 < 2 ** 31 <= 4 * hp * wp * 32
    # the issue's example — 16 x 128 x 128 LR at x8 in fp16, a 2 GiB buffer — is fine: the image offset is 64-bit
    b = E.G32(16, 64, 1024, 1024, 'fp16', 'meta', image_limit=True)
    assert b.bs < 2 ** 31 <= b.bs * 16
    assert E.TrainBuilder.image_limit and not E.Builder.image_limit
