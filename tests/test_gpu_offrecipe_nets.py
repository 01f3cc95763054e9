"""The module layer off the recipe's 3 -> 3 channels: generators, discriminators, SRResNet, Conv2dHIP and the PSNR step
with in_nc / out_nc of 1, 4, 8 and 9 and with nb = 0, against the in-repo oracle (oracle/ref_torch.py, driven by the
state dict) run in float64 under autograd on the CPU.  Every case goes through the code path and the bound of a
3-channel control.  Weights are drawn as synth._conv draws them, U(+-1/sqrt(fan_in)) from per-key streams, so the
3 -> 3 state dicts are the ones synth gives bit for bit (pinned below, without a GPU).

LR inputs are (2, C, 17, 33): both the 16-row and the 32-column tile edge are crossed.  Bounds are the 3-channel
tests': forward 1e-4 and gradients 2e-3 max(1, |ref|) (test_gpu_backward.py), fp16 forward 5e-2 (test_gpu_forward.py),
fp16 gradients 6e-2 relative norm against the fp32 run (test_backward_fp16_close_to_fp32), discriminators 2e-4 /
2e-3 max(1, |ref|) / 1e-4 (test_discriminator_golden).  Each case prints its worst error and the reference's largest
magnitude; the worst measured on an MI355X stands in each test's docstring.
"""
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from esrganplus_amd import synth

LR = (17, 33)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


# ----------------------------------------------------------------------------------------------------------------
# weights (test side; synth.py's convention and streams)
# ----------------------------------------------------------------------------------------------------------------

def rrdbnet_sd(in_nc=3, out_nc=3, nb=1, seed=0):
    sd, keys = OrderedDict(), synth.rrdbnet_keys(nb)
    for i, (key, cout, cin, k, bias) in enumerate(keys):
        cin = in_nc if i == 0 else cin
        cout = out_nc if i == len(keys) - 1 else cout
        synth._conv(sd, seed, key, cout, cin, k, bias)
    return sd


def srresnet_sd(in_nc=3, out_nc=3, nb=1, seed=0, upsample_mode='pixelshuffle'):
    sd, keys = OrderedDict(), synth.srresnet_keys(nb, upsample_mode)
    for i, (key, cout, cin, k) in enumerate(keys):
        synth._conv(sd, seed, key, out_nc if i == len(keys) - 1 else cout, in_nc if i == 0 else cin, k, True)
    return sd


def discriminator_sd(in_nc=3, seed=0, size=128):
    sd = synth.discriminator_state_dict(seed, size)
    first = OrderedDict()
    synth._conv(first, seed, 'features.0', 64, in_nc, 3, True, gain=np.sqrt(3.0))
    sd.update(first)
    return sd


def test_helper_defaults_are_the_3_channel_draws():
    for ours, theirs in ((rrdbnet_sd(nb=2, seed=7), synth.rrdbnet_state_dict(nb=2, seed=7)),
                         (srresnet_sd(nb=2, seed=7), synth.srresnet_state_dict(nb=2, seed=7)),
                         (srresnet_sd(nb=1, seed=7, upsample_mode='upconv'), synth.srresnet_state_dict(1, 7, 'upconv')),
                         (discriminator_sd(seed=7, size=96), synth.discriminator_state_dict(7, 96))):
        assert list(ours) == list(theirs)
        for k in ours:
            assert torch.equal(ours[k], theirs[k]), k
    sd = rrdbnet_sd(9, 2, 1, seed=7)
    assert sd['model.0.weight'].shape == (64, 9, 3, 3) and sd['model.10.weight'].shape == (2, 64, 3, 3)
    assert sd['model.10.bias'].shape == (2,) and sd['model.0.weight'].abs().max() <= 1 / 9.0
    assert torch.equal(sd['model.8.weight'], synth.rrdbnet_state_dict(nb=1, seed=7)['model.8.weight'])
    assert discriminator_sd(1, 7)['features.0.weight'].shape == (64, 1, 3, 3)


def f64(sd, grad=False):
    return {k: (v.double().requires_grad_(grad) if v.is_floating_point() else v.clone()) for k, v in sd.items()}


def worst(name, pairs, bound_of):
    """prints every (what, got, ref) comparison and asserts |got - ref| max <= bound_of(|ref| max)"""
    bad = []
    for what, got, ref in pairs:
        got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
        assert got.shape == ref.shape, (name, what, got.shape, ref.shape)
        e, m = (got - ref).abs().max().item(), ref.abs().max().item()
        print('%s %-36s max|diff| %.3e  max|ref| %.3e  bound %.3e' % (name, what, e, m, bound_of(m)))
        if not e <= bound_of(m):
            bad.append((what, e, m))
    assert not bad, (name, bad)


# ----------------------------------------------------------------------------------------------------------------
# activation ties
#
# The derivative of LeakyReLU / ReLU jumps at zero, so the gradient of a network is not a continuous function of its
# pre-activations: an implementation whose fp32 pre-activation differs from the float64 one in the last bits takes the
# other slope wherever that pre-activation is within rounding of zero, and every gradient downstream of that pixel
# moves by a finite amount — 1e-3 of the scale at these shapes, which hold 3e6 activations of which a handful lie within
# 1e-7 of zero.  fp32 torch on the CPU itself differs from float64 torch by 1.7e-3 in dL/dx of the (1, 1) generator
# for this reason and by 2e-7 where no tie is hit.  The reference is therefore a set: the exact float64 gradients for
# EVERY assignment of the one-sided derivatives at the ties, a tie being a pre-activation within 16 fp32 ulps of its
# layer's largest magnitude (the rounding of a sum of up to 8192 fp32 products) of zero.  `tie_reference` starts from
# the plain assignment and, only if the result is outside its bound there, tries the ties nearest to zero one by one,
# keeping a flip that brings the reference closer; the final comparison is against the exact float64 gradients of that
# assignment, with the unchanged bound.  A wrong kernel is not excused: a flip moves the gradients only in the
# receptive field of one pixel, by an amount the oracle computes, and at most MAX_TIES candidates are tried.
# ----------------------------------------------------------------------------------------------------------------

TIE_ULPS, MAX_TIES = 16, 12


class TieAct:
    """act(x) = x for x > 0, slope * x otherwise, with the branch inverted at the listed (call, flat index) ties"""

    def __init__(self):
        self.ties = []
        self.begin()

    def begin(self, flips=(), record=False):
        self.calls, self.record, self.flips = 0, record, {}
        if record:
            self.ties = []
        for i, j in flips:
            self.flips.setdefault(i, []).append(j)

    def __call__(self, x, slope):
        i, xd = self.calls, x.detach()
        self.calls += 1
        mask = xd > 0
        if self.record:
            tau = TIE_ULPS * 2.0 ** -24 * xd.abs().max().item()
            flat = xd.flatten().abs()
            self.ties += [(flat[j].item() / tau, i, int(j)) for j in (flat < tau).nonzero().flatten()]
        if i in self.flips:
            m = mask.flatten().clone()
            m[self.flips[i]] ^= True
            mask = m.view_as(mask)
        return torch.where(mask, x, x * slope)


class oracle_acts:
    """inside: the oracle's LeakyReLU (ref_torch._lrelu) and the SRResNet restatement's torch.relu are `tie`"""

    def __init__(self, tie, flips=(), record=False):
        self.tie, self.args = tie, (flips, record)

    def __enter__(self):
        from oracle import ref_torch as RT
        self.saved = (RT._lrelu, torch.relu)
        self.tie.begin(*self.args)
        RT._lrelu = lambda x: self.tie(x, RT.NEG_SLOPE)
        torch.relu = lambda x: self.tie(x, 0.0)

    def __exit__(self, *exc):
        from oracle import ref_torch as RT
        RT._lrelu, torch.relu = self.saved


def tie_reference(name, oracle, got, bound_of):
    """oracle(flips) -> {what: float64 reference} (flips = (): the plain assignment, which also records the ties in
    oracle.tie); got: {what: result}.  Returns the reference of the assignment described above."""
    def misfit(ref):
        r = [(got[k].detach().double().cpu() - ref[k]) / bound_of(ref[k].abs().max().item()) for k in got]
        return max(t.abs().max().item() for t in r), sum((t * t).sum().item() for t in r)
    ref, chosen = oracle(()), []
    ties = sorted(oracle.tie.ties)
    worst_, l2 = misfit(ref)
    for _, i, j in ties[:MAX_TIES]:
        if worst_ <= 1.0:
            break
        trial = oracle(chosen + [(i, j)])
        w_, l_ = misfit(trial)
        if l_ < l2:
            chosen, ref, worst_, l2 = chosen + [(i, j)], trial, w_, l_
    print('%s: %d activation ties within %d ulps of zero, reference takes the other slope at %d of them'
          % (name, len(ties), TIE_ULPS, len(chosen)))
    return ref


# ----------------------------------------------------------------------------------------------------------------
# generators
# ----------------------------------------------------------------------------------------------------------------

GEN_CASES = [('RRDBNet', 3, 3, 1),          # the control: the recipe's channels through the same code and bound
             ('RRDBNet', 1, 1, 1), ('RRDBNet', 4, 3, 1), ('RRDBNet', 8, 8, 1), ('RRDBNet', 9, 3, 1),
             ('RRDBNet', 3, 1, 0), ('RRDB_Net', 1, 3, 1)]
_GEN = {}


def gen_case(case):
    """state dict, inputs and the float64 oracle results of one generator case (computed once)"""
    from oracle import ref_torch as RT
    if case in _GEN:
        return _GEN[case]
    cls, in_nc, out_nc, nb = case
    variant = 'codes' if cls == 'RRDBNet' else 'test_image'
    seed = 100 + 10 * in_nc + out_nc
    sd = rrdbnet_sd(in_nc, out_nc, nb, seed)
    x = synth.image_batch(seed, 2, in_nc, *LR, name='off.x')
    gy = synth.normal_like(seed, 'off.gy', (2, out_nc, 4 * LR[0], 4 * LR[1]))
    z = [synth.normal_like(seed, 'off.z.%d' % i, s) for i, s in enumerate(RT.noise_shapes(x.shape, nb, variant))]
    with torch.no_grad():
        y_eval = RT.rrdbnet_forward(x.double(), f64(sd), nb, None, variant)
    tie, out = TieAct(), {}

    def oracle(flips):
        """float64 train forward + backward: {'dL/dx', 'd <key>'}; the plain assignment also leaves y_train"""
        sdr, xr = f64(sd, True), x.double().requires_grad_(True)
        with oracle_acts(tie, flips, record=not flips):
            y = RT.rrdbnet_forward(xr, sdr, nb, [t.double() for t in z], variant)
            (y * gy.double()).sum().backward()
        if not flips:
            out['y_train'] = y.detach()
        return dict([('dL/dx', xr.grad)] + [('d ' + k, sdr[k].grad) for k in grad_keys(nb)])
    oracle.tie = tie
    _GEN[case] = dict(sd=sd, x=x, gy=gy, z=z, variant=variant, y_eval=y_eval, oracle=oracle, out=out)
    return _GEN[case]


def grad_keys(nb):
    dense = 'model.1.sub.0.RDB2.conv2.0.weight' if nb else 'model.1.sub.0.weight'       # nb = 0: LR_conv
    return ('model.0.weight', 'model.10.weight', 'model.10.bias', dense)


def make_net(dev, case, prec='fp32'):
    from esrganplus_amd import architecture as arch
    cls, in_nc, out_nc, nb = case
    net = getattr(arch, cls)(in_nc, out_nc, 64, nb).to(dev).set_precision(prec)
    net.load_state_dict(gen_case(case)['sd'], strict=True)
    return net


@pytest.mark.gpu
@pytest.mark.parametrize('case', GEN_CASES, ids=['%s-%d-%d-nb%d' % c for c in GEN_CASES])
def test_generator_fp32_matches_fp64_oracle(dev, case):
    """eval forward and train forward with explicit z within 1e-4; dL/dx and the gradients of model.0.weight, the last
    conv's weight and bias and one dense-block weight (nb = 0: LR_conv's) within 2e-3 max(1, |ref|), against the
    float64 gradients of one assignment of the activation ties (see `tie_reference`).
    Worst measured on an MI355X: forwards 9.9e-8 (|ref| 0.08); gradients 6.4e-4 in dL/dx of (8, 8) and 8.9e-4 in its
    model.0.weight (|ref| 0.39 / 4.8: ties left as they were, inside the bound); where no tie is hit 8.7e-7 / 4.8e-6.
    The plain assignment missed the bound in dL/dx of (1, 1) and (9, 3) by 2.4e-3 / 2.5e-3 against 2e-3; with the
    other slope at two / one of their 15 / 9 ties they are at 1.5e-4 / 1.6e-5."""
    r = gen_case(case)
    net = make_net(dev, case)
    with torch.no_grad():
        ye = net.eval()(r['x'].to(dev))
    net.train()
    x = r['x'].to(dev).requires_grad_(True)
    y = net(x, z=[t.to(dev) for t in r['z']])
    (y * r['gy'].to(dev)).sum().backward()
    name = '%s(%d,%d,nb=%d)' % case
    params = dict(net.named_parameters())
    assert x.grad is not None and all(params[k].grad is not None for k in grad_keys(case[3]))
    got = dict([('dL/dx', x.grad)] + [('d ' + k, params[k].grad) for k in grad_keys(case[3])])
    bound = lambda m: 2e-3 * max(1.0, m)
    ref = tie_reference(name, r['oracle'], got, bound)
    worst(name, [('eval forward', ye, r['y_eval']), ('train forward', y, r['out']['y_train'])], lambda m: 1e-4)
    worst(name, [(k, got[k], ref[k]) for k in got], bound)


FP16_CASES = [GEN_CASES[0], GEN_CASES[1], GEN_CASES[2]]


@pytest.mark.gpu
@pytest.mark.parametrize('case', FP16_CASES, ids=['%s-%d-%d-nb%d' % c for c in FP16_CASES])
def test_generator_fp16_tracks_fp32_on_the_fused_chain(dev, case):
    """fp16 eval forward within 5e-2 of the oracle; every parameter gradient and dL/dx of the fp16 pass within 6e-2
    relative norm of the fp32 pass's; the fp16 pass runs the dense blocks as the fused training chain.
    Worst measured on an MI355X: forward 6.3e-5; gradients 3.5e-2 (3, 3), 4.9e-2 (1, 1), 5.8e-2 (4, 3)."""
    from esrganplus_amd import engine as E, _lib as L
    r = gen_case(case)
    res = {}
    for prec in ('fp32', 'fp16'):
        net = make_net(dev, case, prec).eval()
        x = r['x'].to(dev).requires_grad_(True)
        y = net(x)
        (y * r['gy'].to(dev)).sum().backward()
        res[prec] = dict(y=y.detach(), gx=x.grad, g={k: p.grad.clone() for k, p in net.named_parameters()})
        if prec == 'fp16':
            assert E.use_train_chain(L.ESR_F16, 2, LR[0], LR[1], False)
            plans = [tp for key, pool in net._plans.items() if isinstance(key, tuple) and key[0] == 'train' for tp in pool]
            assert len(plans) == 1 and plans[0].bwd_chain_ops and plans[0].fwd.chain_ops, 'not the fused training chain'
    name = '%s(%d,%d,nb=%d) fp16' % case
    worst(name, [('eval forward', res['fp16']['y'], r['y_eval'])], lambda m: 5e-2)
    rels = [(k, ((a - res['fp16']['g'][k]).norm() / a.norm().clamp_min(1e-6)).item()) for k, a in res['fp32']['g'].items()]
    rels.append(('dL/dx', ((res['fp32']['gx'] - res['fp16']['gx']).norm() / res['fp32']['gx'].norm()).item()))
    k, e = max(rels, key=lambda t: t[1])
    print('%s gradients vs fp32: worst relative norm %.3e (%s), bound 6e-2' % (name, e, k))
    assert e <= 6e-2, (k, e)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize('case', [GEN_CASES[1], GEN_CASES[3]], ids=['1-1', '8-8'])
def test_inference_forms_are_bit_identical_to_their_references(dev, case):
    """forward_x8 and forward_tiled (tile 8, pad 3) on 1 and on 8 channels (the most the ends take), forward_tiled_x8
    and forward_tiled_many on 1 channel, against the pure-torch restatements over the net's own forward (bit for
    bit; that forward within 1e-4 of the oracle: 7.5e-8 measured)"""
    from esrganplus_amd import functional as F
    r = gen_case(case)
    net = make_net(dev, case).eval()
    x = r['x'].to(dev)
    with torch.no_grad():
        assert _same_bits(net.forward_x8(x), F.x8_reference(net, x))
        assert _same_bits(net.forward_tiled(x, tile=8, pad=3), F.tiled_reference(net, x, 8, 3))
        if case[1] == 1:
            assert _same_bits(net.forward_tiled_x8(x, tile=8, pad=3), F.tiled_x8_reference(net, x, 8, 3))
            xs = [x[0], x[1:2, :, :9, :20].contiguous()]
            ys, refs = net.forward_tiled_many(xs, tile=8, pad=3), F.tiled_many_reference(net, xs, 8, 3)
            assert len(ys) == 2 and all(_same_bits(a, b) for a, b in zip(ys, refs))
        # ... and the whole-image forward they restate is the oracle's
        worst('%s(%d,%d,nb=%d)' % case, [('forward', net(x), r['y_eval'])], lambda m: 1e-4)


# ----------------------------------------------------------------------------------------------------------------
# discriminators
# ----------------------------------------------------------------------------------------------------------------

D_CASES = [(128, 3), (128, 1), (96, 4)]            # (size, in_nc); the first is the control


@pytest.mark.gpu
@pytest.mark.parametrize('size,in_nc', D_CASES)
def test_discriminator_train_mode_matches_fp64_oracle(dev, size, in_nc):
    """B = 2 in train mode (batch statistics): logits within 2e-4, running statistics within 1e-4 and
    num_batches_tracked = 1, the input gradient within 2e-4, the gradients of the first conv, one BatchNorm and the
    head within 2e-3 max(1, |ref|) (test_discriminator_golden's bounds; gradients against one assignment of the
    activation ties, see `tie_reference`).
    Worst measured on an MI355X: logits 1.7e-6, running statistics 3.9e-7, dL/dx 1.5e-4 on one channel and 1.7e-7 on
    3 and 4; parameter gradients 7.4e-5 (features.0.weight on one channel, |ref| 0.19).  The plain assignment missed the input gradient's bound in
    all three cases (2.9e-4, 7.2e-4, 2.8e-4 against 2e-4): B = 2 leaves 4 x 4 and 3 x 3 maps of batch statistics behind
    the last convs, where one flipped LeakyReLU moves every pixel under it; one, one and three of the 22, 22 and 10
    ties took the other slope."""
    from esrganplus_amd import architecture as arch
    from oracle import ref_torch as RT
    seed = 200 + size + in_nc
    sd = discriminator_sd(in_nc, seed, size)
    x = synth.image_batch(seed, 2, in_nc, size, size, name='offd.x')
    gy = synth.normal_like(seed, 'offd.gy', (2, 1))
    stats = {k: v.double() for k, v in sd.items() if 'running' in k}
    keys = ('features.0.weight', 'features.0.bias', 'features.3.weight', 'features.3.bias', 'features.27.weight',
            'classifier.0.weight', 'classifier.0.bias', 'classifier.2.weight')
    tie, out = TieAct(), {}

    def oracle(flips):
        sdr, xr = f64(sd, True), x.double().requires_grad_(True)
        sdr.update({k: v.clone() for k, v in stats.items()})           # buffers: updated in place, no gradient
        with oracle_acts(tie, flips, record=not flips):
            yo = RT.discriminator_forward(xr, sdr, training=True, size=size)
            (yo * gy.double()).sum().backward()
        if not flips:
            out.update(yo=yo.detach(), sdr=sdr)
        return dict([('dL/dx', xr.grad)] + [('d ' + k, sdr[k].grad) for k in keys])
    oracle.tie = tie
    net = getattr(arch, 'Discriminator_VGG_%d' % size)(in_nc, 64).to(dev).train()
    net.load_state_dict(sd, strict=True)
    xg = x.to(dev).requires_grad_(True)
    y = net(xg)
    (y * gy.to(dev)).sum().backward()
    name = 'Discriminator_VGG_%d(%d)' % (size, in_nc)
    params, bufs = dict(net.named_parameters()), dict(net.named_buffers())
    got = dict([('dL/dx', xg.grad)] + [('d ' + k, params[k].grad) for k in keys])
    # (one misfit scale for the search: the input gradient's bound is absolute, the parameters' relative above 1)
    ref = tie_reference(name, oracle, got, lambda m: 2e-4)
    yo, sdr = out['yo'], out['sdr']
    worst(name, [('logits', y, yo), ('dL/dx', got['dL/dx'], ref['dL/dx'])], lambda m: 2e-4)
    worst(name, [('d ' + k, got['d ' + k], ref['d ' + k]) for k in keys], lambda m: 2e-3 * max(1.0, m))
    for k in ('features.3', 'features.15', 'features.27'):
        for s in ('.running_mean', '.running_var'):
            assert not torch.equal(sdr[k + s], stats[k + s]), 'the oracle did not update ' + k + s
    worst(name, [(k + s, bufs[k + s], sdr[k + s]) for k in ('features.3', 'features.15', 'features.27')
                 for s in ('.running_mean', '.running_var')], lambda m: 1e-4)
    assert int(bufs['features.3.num_batches_tracked']) == 1 == int(sdr['features.3.num_batches_tracked'])


def _ragan(pa, pb):
    bce = TF.binary_cross_entropy_with_logits
    return (bce(pb - pa.mean(), torch.ones_like(pb)) + bce(pa - pb.mean(), torch.zeros_like(pa))) / 2


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['d_step', 'g_step'])
def test_one_channel_forward_pair_matches_two_calls(dev, mode):
    """forward_pair on Discriminator_VGG_128(1, 64) against two calls, fp32, within
    test_discriminator_forward_pair_matches_two_calls' 2e-4 (running statistics 2e-5).  Worst measured on an
    MI355X: 9.3e-5 (d_step), 0 (g_step)."""
    from esrganplus_amd import architecture as arch
    tol = 2e-4
    sd = discriminator_sd(1, 5)
    a0 = synth.image_batch(61, 2, 1, 128, 128, name='offpair.a').to(dev)
    b0 = synth.image_batch(62, 2, 1, 128, 128, name='offpair.b').to(dev)
    res = {}
    for how in ('two', 'pair'):
        net = arch.Discriminator_VGG_128(1, 64).to(dev).train()
        net.load_state_dict(sd)
        a, b = a0.clone(), b0.clone()
        if mode == 'g_step':
            for p in net.parameters():
                p.requires_grad = False
            a.requires_grad_(True)
        if how == 'two':
            ya = net(a)
            yb = net(b).detach() if mode == 'g_step' else net(b)
        else:
            ya, yb = net.forward_pair(a, b)
        _ragan(ya, yb).backward()
        bn = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
        res[how] = dict(ya=ya.detach(), yb=yb.detach(), ga=a.grad,
                        gp=[p.grad for p in net.parameters()] if mode == 'd_step' else [],
                        rm=[m.running_mean.clone() for m in bn], rv=[m.running_var.clone() for m in bn],
                        nbt=[int(m.num_batches_tracked) for m in bn])
    two, pair = res['two'], res['pair']
    assert pair['nbt'] == two['nbt'] == [2] * len(two['nbt'])
    rel = lambda x, y: ((x - y).abs().max() / y.abs().max().clamp_min(1e-12)).item()
    errs = [rel(pair['ya'], two['ya']), rel(pair['yb'], two['yb'])]
    assert max(errs) <= tol, errs
    for x, y in zip(pair['rm'] + pair['rv'], two['rm'] + two['rv']):
        assert rel(x, y) <= max(tol * 0.1, 1e-5)
    if mode == 'g_step':
        errs.append(rel(pair['ga'], two['ga']))
        assert errs[-1] <= tol
    else:
        assert pair['ga'] is None
        gmax = max(y.abs().max().item() for y in two['gp'])
        for x, y in zip(pair['gp'], two['gp']):
            e = (x - y).abs().max().item() / max(y.abs().max().item(), 1e-3 * gmax)
            errs.append(e)
            assert e <= tol
    print('forward_pair 1 channel %s: worst relative difference %.3e, bound %.1e' % (mode, max(errs), tol))


# ----------------------------------------------------------------------------------------------------------------
# SRResNet and Conv2dHIP
# ----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('in_nc,out_nc', [(3, 3), (1, 1)])
@pytest.mark.parametrize('mode', ['pixelshuffle', 'upconv'])
def test_srresnet_matches_fp64(dev, mode, in_nc, out_nc):
    """SRResNet(1, 1, 64, 1) (and the 3-channel control) against tests/test_gpu_srresnet.py's restatement in float64,
    with test_srresnet_is_one_launch_plan's bounds: output 1e-4, input and parameter gradients 2e-3, relative
    (gradients against one assignment of the ReLU ties, see `tie_reference`).
    Worst measured on an MI355X, relative: forward 1.4e-6, gradients 3.9e-6.  The plain assignment missed the bound in
    both upconv cases (a ReLU tie behind model.6 on 3 channels: 3.4e-3 in its bias gradient; behind model.8 on one:
    7.8e-3); the other slope at two of 6 / one of 7 ties."""
    from esrganplus_amd import architecture as arch
    from tests.test_gpu_srresnet import _torch_srresnet
    nb, seed = 1, 300 + in_nc
    sd = srresnet_sd(in_nc, out_nc, nb, seed, mode)
    x = synth.image_batch(seed, 2, in_nc, *LR, name='offsr.x')
    gy = synth.normal_like(seed, 'offsr.gy', (2, out_nc, 4 * LR[0], 4 * LR[1]))
    tie, out = TieAct(), {}

    def oracle(flips):
        sdr, xr = f64(sd, True), x.double().requires_grad_(True)
        with oracle_acts(tie, flips, record=not flips):
            yo = _torch_srresnet(xr, sdr, nb, mode, 1.0)
            (yo * gy.double()).sum().backward()
        if not flips:
            out['yo'] = yo.detach()
        return dict([('dL/dx', xr.grad)] + [('d ' + k, v.grad) for k, v in sdr.items()])
    oracle.tie = tie
    net = arch.SRResNet(in_nc, out_nc, 64, nb, upscale=4, upsample_mode=mode).to(dev)
    net.load_state_dict(sd, strict=True)
    xg = x.to(dev).requires_grad_(True)
    y = net(xg)
    (y * gy.to(dev)).sum().backward()
    name = 'SRResNet(%d,%d) %s' % (in_nc, out_nc, mode)
    params = dict(net.named_parameters())
    got = dict([('dL/dx', xg.grad)] + [('d ' + k, params[k].grad) for k in sd])
    ref = tie_reference(name, oracle, got, lambda m: 2e-3 * m)
    worst(name, [('forward', y, out['yo'])], lambda m: 1e-4 * m)
    worst(name, [(k, got[k], ref[k]) for k in got], lambda m: 2e-3 * m)


@pytest.mark.gpu
@pytest.mark.parametrize('prec', ['fp32', 'fp16'])
@pytest.mark.parametrize('cin,cout,ks', [(1, 5, 3), (5, 1, 3), (1, 5, 4), (5, 1, 4), (5, 7, 3)])
def test_conv2dhip_narrow_channels_match_fp64(dev, cin, cout, ks, prec):
    """Conv2dHIP forward and backward against float64 conv2d on the stored values (fp16: x, w and the upstream gradient
    rounded to fp16), within the conv files' bounds relative to the reference's largest magnitude: forward 4e-6 /
    6e-4, input gradient 4e-6 / 1.5e-3, weight and bias gradients 2e-6.  (5, 7) is the control.
    Worst measured on an MI355X: forward 2.3e-7 / 3.6e-4, input gradient 2.5e-7 / 4.0e-4, weight and bias gradients
    7.7e-7 (db of (5, 1, k4) fp32)."""
    from esrganplus_amd import architecture as arch
    st = 2 if ks == 4 else 1
    q = (lambda t: t.half().float()) if prec == 'fp16' else (lambda t: t)
    key = 'offconv.%d.%d.%d' % (cin, cout, ks)
    H, W = (26, 40) if st == 2 else (13, 40)
    x = q(synth.normal_like(1, key + '.x', (2, cin, H, W)))
    w = q(synth.normal_like(1, key + '.w', (cout, cin, ks, ks)) / np.sqrt(cin * ks * ks))
    b = synth.normal_like(1, key + '.b', (cout,)) * 0.5
    gy = q(synth.normal_like(1, key + '.gy', (2, cout, H // st, W // st)))
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    yo = TF.conv2d(xr, wr, br, stride=st, padding=(ks - 1) // 2)
    (yo * gy.double()).sum().backward()
    m = arch.Conv2dHIP(cin, cout, ks, stride=st, padding=(ks - 1) // 2).to(dev).set_precision(prec)
    with torch.no_grad():
        m.weight.copy_(w)
        m.bias.copy_(b)
    xg = x.to(dev).requires_grad_(True)
    y = m(xg)
    (y * gy.to(dev)).sum().backward()
    name = 'Conv2dHIP(%d,%d,k%d) %s' % (cin, cout, ks, prec)
    f, d = {'fp32': (4e-6, 4e-6), 'fp16': (6e-4, 1.5e-3)}[prec]
    worst(name, [('forward', y, yo)], lambda s: f * s)
    worst(name, [('dL/dx', xg.grad, xr.grad)], lambda s: d * s)
    worst(name, [('dW', m.weight.grad, wr.grad), ('db', m.bias.grad, br.grad)], lambda s: 2e-6 * s)


# ----------------------------------------------------------------------------------------------------------------
# PSNR step
# ----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('in_nc,out_nc', [(3, 3), (1, 1)])
def test_psnr_step_two_iterations_match_oracle_and_adam(dev, in_nc, out_nc):
    """PSNRStep on RRDBNet(1, 1, 64, 1) (and the 3-channel control), two iterations with explicit z, against the oracle
    under autograd plus torch.optim.Adam in float64, with test_three_iterations_match_the_reference's bounds: l_pix
    within 5e-4 max(1, |ref|), fake_H within 2e-3 of the reference's maximum, after iteration 1 every parameter
    gradient within 1e-2 of that tensor's maximum, after iteration 2 the deltas of three tensors within
    mean|d - ref| / mean|ref| <= 0.08.  Worst measured on an MI355X on one channel: l_pix 1e-7, fake_H 2e-6 of its
    maximum, gradients 2.6e-5 of theirs, deltas 2.8e-5."""
    from esrganplus_amd import architecture as arch, train
    from oracle import ref_torch as RT
    nb, seed, lr_G = 1, 400 + in_nc, 2e-4
    sd = rrdbnet_sd(in_nc, out_nc, nb, seed)
    netG = arch.RRDBNet(in_nc, out_nc, 64, nb).to(dev).train()
    netG.load_state_dict(sd, strict=True)
    st = train.PSNRStep(netG, lr_G=lr_G)
    sdr = f64(sd, True)
    opt = torch.optim.Adam(list(sdr.values()), lr=lr_G, betas=(0.9, 0.999))
    pg = dict(netG.named_parameters())
    name = 'PSNRStep(%d,%d)' % (in_nc, out_nc)
    for it in (1, 2):
        lr = synth.image_batch(seed + it, 2, in_nc, *LR, name='offstep.lr')
        hr = synth.image_batch(seed + it, 2, out_nc, 4 * LR[0], 4 * LR[1], name='offstep.hr')
        z = [synth.normal_like(seed + it, 'offstep.z.%d' % i, s) for i, s in enumerate(RT.noise_shapes(lr.shape, nb))]
        opt.zero_grad()
        fake = RT.rrdbnet_forward(lr.double(), sdr, nb, [t.double() for t in z])
        l_ref = (fake - hr.double()).abs().mean()
        l_ref.backward()
        got = st.step(lr.to(dev), hr.to(dev), z=[t.to(dev) for t in z])['l_pix']
        print('%s iteration %d  l_pix hip %.6f  ref %.6f' % (name, it, float(got), float(l_ref.detach())))
        assert abs(float(got) - float(l_ref.detach())) <= 5e-4 * max(1.0, abs(float(l_ref.detach())))
        worst(name, [('fake_H %d' % it, st.fake_H, fake)], lambda m: 2e-3 * m)
        if it == 1:
            worst(name, [('d ' + k, pg[k].grad, v.grad) for k, v in sdr.items()], lambda m: 1e-2 * m)
        opt.step()
    st.finish()
    for k in ('model.0.weight', 'model.10.weight', 'model.1.sub.0.RDB1.conv1.0.weight'):
        d, ref = pg[k].detach().cpu().double() - sd[k].double(), sdr[k].detach() - sd[k].double()
        err = ((d - ref).abs().mean() / ref.abs().mean()).item()
        print('%s delta of %-40s mean|d - ref| / mean|ref| = %.3e' % (name, k, err))
        assert err <= 0.08, (k, err)
