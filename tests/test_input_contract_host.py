"""The input contract of the module layer, on the host: what an entry point cannot run it refuses with a ValueError
that names the expected and the given shape — before the device is touched and before a plan is built — instead of
pointing a layout op built for the first conv's channels, or a linear head sized for one input, at a tensor of another
shape.  Everything here runs on CPU tensors: a wrong shape must never reach a device, and a right one still ends at
the `no CPU fallback` error (tests/test_host.py::test_no_cpu_fallback).
"""
import types

import pytest
import torch


def _arch():
    from esrganplus_amd import architecture as arch, _lib
    return arch, _lib


_NETS = {}


def net_of(name):
    """one module per kind, shared by the tests (the discriminators' heads are a few MB each)"""
    arch, _ = _arch()
    if name not in _NETS:
        torch.manual_seed(0)
        _NETS[name] = {
            'd128': lambda: arch.Discriminator_VGG_128(3, 64),
            'd96': lambda: arch.Discriminator_VGG_96(3, 64),
            'd192': lambda: arch.Discriminator_VGG_192(3, 64),
            'd128_1ch': lambda: arch.Discriminator_VGG_128(1, 64),
            'd128_sn': lambda: arch.Discriminator_VGG_128_SN(),
            'vgg': lambda: arch.VGGFeatureExtractor(),
            'srresnet': lambda: arch.SRResNet(3, 3, 64, 1, upsample_mode='pixelshuffle'),
            'srresnet_1ch': lambda: arch.SRResNet(1, 1, 64, 1),
            'conv': lambda: arch.Conv2dHIP(5, 7, 3, padding=1),
            'conv_s2': lambda: arch.Conv2dHIP(5, 7, 4, stride=2, padding=1),
        }[name]()
    return _NETS[name]


# (net, the shape it takes, its first conv's channels)
GOOD = {'d128': (2, 3, 128, 128), 'd96': (2, 3, 96, 96), 'd192': (2, 3, 192, 192), 'd128_1ch': (2, 1, 128, 128),
        'd128_sn': (2, 3, 128, 128), 'vgg': (2, 3, 32, 48), 'srresnet': (2, 3, 9, 12), 'srresnet_1ch': (2, 1, 9, 12),
        'conv': (2, 5, 9, 12), 'conv_s2': (2, 5, 9, 12)}


def entries(net, pair_shape=None):
    """every entry point of a _SeqNet as (name, callable of one tensor); the pair forms get a second operand of the
    same shape (pair_shape: of that shape instead)"""
    def other(x):
        return torch.zeros(pair_shape if pair_shape is not None else tuple(x.shape))

    def shared(x):
        was = net.training
        net.train()
        try:
            return net.forward_shared(x.clone().requires_grad_(True), other(x))
        finally:
            net.train(was)

    out = [('forward', lambda x: net(x)),
           ('_run_forward', lambda x: net._run_forward(x, need_bwd=False)),
           ('_run_forward_bwd', lambda x: net._run_forward(x, need_bwd=True)),
           ('forward_pair', lambda x: net.forward_pair(x, other(x))),
           ('_pair_begin', lambda x: net._pair_begin(x))]
    if net._shared_ok:
        out.append(('forward_shared', shared))
    return out


def refused(call, x, *needles):
    with pytest.raises(ValueError) as ei:
        call(x)
    msg = str(ei.value)
    for n in needles + (str(tuple(x.shape)),):
        assert str(n) in msg, (n, msg)
    return msg


@pytest.mark.parametrize('name', sorted(GOOD))
def test_wrong_rank_channels_and_empty_maps_are_refused(name):
    net, good = net_of(name), GOOD[name]
    B, C_, H, W = good
    want = '[B, %d, H, W]' % C_
    for ename, call in entries(net):
        refused(call, torch.zeros(C_, H, W), want, '3-D')                          # not 4-D
        refused(call, torch.zeros(1, B, C_, H, W), want, '5-D')
        for c in (C_ + 1, C_ - 1, 2 * C_):                                          # another channel count
            if c > 0:
                refused(call, torch.zeros(B, c, H, W), 'expected %d input channels' % C_, 'got %d' % c)
        refused(call, torch.zeros(B, C_, 0, W), want)                               # empty spatial extent
        refused(call, torch.zeros(B, C_, H, 0), want)
    assert net._plans == {} and net._wp == {}, 'a refusal built a plan or packed weights'


@pytest.mark.parametrize('name,shape,layer', [
    ('d128', (2, 3, 16, 16), 'features.'),          # 16 -> 8 -> 4 -> 2 -> 1 -> 0 behind the fifth 4x4/s2 conv
    ('d192', (2, 3, 32, 16), 'features.'),
    ('d128_sn', (2, 3, 128, 16), 'conv9'),
    ('vgg', (2, 3, 8, 64), 'a pool'),               # 8 -> 4 -> 2 -> 1 -> 0 behind the fourth pool
    ('vgg', (2, 3, 1, 1), 'a pool'),
    ('conv_s2', (2, 5, 1, 9), 'conv'),              # (1 + 2 - 4) // 2 + 1 = 0
])
def test_maps_that_vanish_are_refused(name, shape, layer):
    net = net_of(name)
    for ename, call in entries(net):
        msg = refused(call, torch.zeros(shape), layer)
        assert 'behind' in msg and ('0 x' in msg or 'x 0' in msg), msg
    assert net._plans == {}


@pytest.mark.parametrize('name,size,feat,bad', [
    ('d128', 128, 8192, (192, 96, 64, 160)),         # 192: 100 x 18432 floats read from a 100 x 8192 weight
    ('d128_1ch', 128, 8192, (192, 96)),
    ('d128_sn', 128, 8192, (192, 96)),
    ('d96', 96, 4608, (128, 192, 64)),
    ('d192', 192, 4608, (128, 96, 256)),
])
def test_head_feature_count_is_checked(name, size, feat, bad):
    """the linear head reads w1 with the feature count of the plan's last map: any other crop is refused, and the
    message names the input size the net takes"""
    net = net_of(name)
    C_ = GOOD[name][1]
    assert net._head()['w1'].shape[1] == feat
    for ename, call in entries(net):
        for s in bad:
            msg = refused(call, torch.zeros(2, C_, s, s), '[B, %d, %d, %d]' % (C_, size, size), '%d features' % feat)
            side = s >> sum(1 for l in net._spec() if l.get('stride') == 2)
            assert '512 x %d x %d = %d features' % (side, side, 512 * side * side) in msg, msg
        # a crop that is right in one direction only
        refused(call, torch.zeros(2, C_, size, 2 * size), '%d features' % feat)
    assert net._plans == {}


@pytest.mark.parametrize('name', ['d128', 'd96', 'vgg', 'srresnet'])
def test_pair_operands_must_have_one_shape(name):
    net, good = net_of(name), GOOD[name]
    B, C_, H, W = good
    for other in ((B + 1, C_, H, W), (B, C_, H, W + 32), (B, C_, H + 32, W)):
        for ename, call in entries(net, pair_shape=other):
            if ename in ('forward_pair', 'forward_shared'):
                msg = refused(call, torch.zeros(good), 'expected')
                assert str(other) in msg, msg
        # _pair_finish: the late operand against what _pair_begin ran (the plan keeps the early operand)
        plan = types.SimpleNamespace(keep_x=(torch.zeros(other),))
        msg = refused(lambda x: net._pair_finish(plan, x), torch.zeros(good), 'expected %s' % (other,))
    plan = types.SimpleNamespace(keep_x=(torch.zeros(good),))
    refused(lambda x: net._pair_finish(plan, x), torch.zeros(B, C_ + 1, H, W), 'expected %s' % (good,))
    refused(lambda x: net._pair_finish(plan, x), torch.zeros(C_, H, W), 'expected %s' % (good,))
    assert net._plans == {}


@pytest.mark.parametrize('name', sorted(GOOD))
def test_right_shapes_still_end_at_no_cpu_fallback(name):
    """the checks come in front of the device check, not instead of it"""
    _, L = _arch()
    net, good = net_of(name), GOOD[name]
    for ename, call in entries(net):
        with pytest.raises(L.HipExtensionError):
            call(torch.zeros(good))
    plan = types.SimpleNamespace(keep_x=(torch.zeros(good),))
    with pytest.raises(L.HipExtensionError):
        net._pair_finish(plan, torch.zeros(good))
    assert net._plans == {}


def test_refused_input_leaves_the_spectral_norm_state_alone():
    """Discriminator_VGG_128_SN runs a power iteration per training forward: not for an input it refuses"""
    net = net_of('d128_sn').train()
    before = [m.weight_u.clone() for m in net._sn_layers()]
    for bad in (torch.zeros(2, 1, 128, 128), torch.zeros(2, 3, 96, 96), torch.zeros(3, 128, 128)):
        with pytest.raises(ValueError):
            net(bad)
        with pytest.raises(ValueError):
            net.forward_pair(bad, bad)
    assert all(torch.equal(a, m.weight_u) for a, m in zip(before, net._sn_layers()))


def test_srresnet_x3_checks_through_its_convs():
    """the x3 SRResNet walks per-conv modules: the first conv refuses what the planned form refuses"""
    arch, L = _arch()
    net = arch.SRResNet(3, 3, 64, 1, upscale=3, upsample_mode='pixelshuffle')
    with pytest.raises(ValueError) as ei:
        net(torch.zeros(2, 1, 9, 12))
    assert 'expected 3 input channels' in str(ei.value) and '(2, 1, 9, 12)' in str(ei.value)
    with pytest.raises(L.HipExtensionError):
        net(torch.zeros(2, 3, 9, 12))


# ---------------------------------------------------------------------------------------------------------------
# train steps
# ---------------------------------------------------------------------------------------------------------------

def test_train_steps_refuse_mismatched_channel_counts():
    arch, _ = _arch()
    from esrganplus_amd import train
    g1, g3, g4 = (arch.RRDBNet(3, c, 64, 0) for c in (1, 3, 4))
    d1, d3, vgg = net_of('d128_1ch'), net_of('d128'), net_of('vgg')
    for Step, kw in ((train.ESRGANPlusStep, {}), (train.SRGANStep, {}), (train.SRGANStep, dict(feature_weight=0))):
        for g, d, c in ((g1, d3, 1), (g4, d3, 4), (g3, d1, 3)):
            with pytest.raises(ValueError) as ei:
                Step(g, d, vgg, **kw)
            msg = str(ei.value)
            assert 'netD expects %d input channels' % d.in_nc in msg and 'out_nc = %d' % c in msg, msg
    # generator and discriminator agree on one channel, but a feature term reads 3
    for Step in (train.ESRGANPlusStep, train.SRGANStep):
        with pytest.raises(ValueError) as ei:
            Step(g1, d1, vgg)
        msg = str(ei.value)
        assert 'expects 3 input channels' in msg and 'out_nc = 1' in msg, msg
    # ... and without the feature term there is nothing to refuse; matching 3-channel networks pass as before
    train._check_channels('SRGANStep', g1, d1, None)
    train._check_channels('ESRGANPlusStep', g3, d3, vgg)
    # a wrapped generator is asked through .module, as the steps reach its plans
    with pytest.raises(ValueError):
        train._check_channels('ESRGANPlusStep', types.SimpleNamespace(module=g4), d3, vgg)


# ---------------------------------------------------------------------------------------------------------------
# tiled and x8 forms
# ---------------------------------------------------------------------------------------------------------------

def _forms(net, x):
    return [('forward_x8', lambda: net.forward_x8(x)),
            ('forward_tiled', lambda: net.forward_tiled(x, tile=8, pad=3)),
            ('forward_tiled_x8', lambda: net.forward_tiled_x8(x, tile=8, pad=3)),
            ('forward_tiled_many', lambda: net.forward_tiled_many([x[0]], tile=8, pad=3))]


@pytest.mark.parametrize('in_nc,out_nc', [(9, 3), (3, 9), (17, 20)])
def test_tiled_and_x8_forms_refuse_more_than_8_channels(in_nc, out_nc):
    arch, _ = _arch()
    net = arch.RRDBNet(in_nc, out_nc, 64, 0).eval()
    for what, call in _forms(net, torch.zeros(1, in_nc, 9, 12)):
        with pytest.raises(ValueError) as ei:
            call()
        msg = str(ei.value)
        assert what in msg and 'in_nc <= 8 and out_nc <= 8' in msg, msg
        assert 'in_nc=%d' % in_nc in msg and 'out_nc=%d' % out_nc in msg, msg
    assert net._plans == {} and net._wp == {}


def test_tiled_and_x8_forms_take_8_channels():
    arch, L = _arch()
    net = arch.RRDBNet(8, 8, 64, 0).eval()
    for what, call in _forms(net, torch.zeros(1, 8, 9, 12)):
        with pytest.raises((L.HipExtensionError, ValueError)) as ei:       # (forward_tiled_many: a ValueError)
            call()
        assert 'no CPU fallback' in str(ei.value), (what, ei.value)
