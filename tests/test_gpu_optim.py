"""Fused Adam (adam_kernel) and the dynamic loss scaler (amp_check / amp_count / amp_update kernels, csrc/nn_kernels.hip)
through esrganplus_amd.optim, against the fp64 restatement tests/fp64_refs.adam_ref (pinned to torch.optim.Adam in
float64 by tests/test_fp64_refs.py): parameters AND both moment buffers after every step, at tensor sizes around the
4096-element block table's partial blocks, with weight decay, non-default betas / eps, zero and underflowing gradients,
and the host paths that shift the flat offsets.  The scaler's values are exact.

Error bounds (U = 2^-24, t = steps applied so far), from adam_kernel's operation count:

* g = grad * gs (+ wd * p): the scale's division by the loss scale and its product with grad one rounding each, wd * p
  and the sum one each: 4 U relative to gmag = |grad * gs| + wd |p|;
* m = b1 * m + omb1 * g: fl(b1), omb1 = fl(1 - b1), two products, one sum: 5 more -> c'_m = 9 per step, relative to
  the recursion of m on gmag (``mag``: it is >= |m|, and equal to it unless gradients of both signs cancel);
* v = b2 * v + omb2 * g * g: 8 U from g^2, fl(b2), omb2, three products, one sum -> c'_v = 14 per step, relative to
  ``vmag`` (v on gmag^2; equal to v when wd = 0);
  -> |m - ref| <= c'_m t U mag + X + 2^-126,  |v - ref| <= c'_v t U vmag + Y + 2^-126.  The floor is the fp32
  denormal threshold (the 1e-20 block: g^2 = 1e-40); X, Y feed the parameter's own error back through wd * p:
  X_t = b1 X_{t-1} + (1 - b1) wd Bp_{t-1},  Y_t = b2 Y_{t-1} + (1 - b2) (2 |g| + wd Bp_{t-1}) wd Bp_{t-1};
* upd = (lr / bc1) * m / (sqrt(v) * rsqrt(bc2) + eps): fl(lr), fl(bc1), the quotient: 3;  fl(bc2), rsqrtf (1 ulp = 2 U),
  sqrtf, the product, fl(eps) + the sum: 6;  step * m and the division: 2 -> c = 11, relative to |upd|;
* p - upd: half an ulp of the result, <= U |p|.
  -> per step Bp grows by U |p| + c U |upd| + what the moments' errors move upd by:
     (lr / bc1) tol_m / den' + |upd| dden / den',  dden = min(tol_v / (2 sqrt(v)), sqrt(tol_v)) / sqrt(bc2),
     den' = den - dden.
  With the moments exact this is the "t (ulp(p) / 2 + c lr U)" of a plain count; the two extra terms are the
  correction that count needs, because the moments' own errors grow like c' t U and pass into every later update.
  Where tol_v is no longer small against v (grad * gs and wd * p cancel in g: dden >= den / 2) a first-order term means
  nothing, and the update's error is bounded by Adam's own ceiling instead: by Cauchy-Schwarz over the steps
  |m| <= sqrt(sum_k w1_k^2 / w2_k) sqrt(v) with w1_k = (1 - b1) b1^(t-k), w2_k = (1 - b2) b2^(t-k), for the kernel's
  moments as for the reference's, so the two updates differ by at most 2 lr K_t, K_t = sqrt(sum_k w1_k^2 / w2_k) *
  sqrt(bc2) / bc1 (a 0.1 % allowance covers the kernel's roundings of that inequality).
"""
import numpy as np
import pytest
import torch

from tests import fp64_refs as R

pytestmark = pytest.mark.gpu

U = R.U
C_UPD, C_M, C_V = 11, 9, 14
TINY = 2.0 ** -126
SCALE = 1024.0
SHAPES = [(1,), (255,), (256,), (257,), (4095,), (4096,), (4097,), (2 * 4096 + 3,), (64, 3, 3, 3)]
ZERO_T, TINY_T = 3, 6           # the tensor whose gradient is zero throughout / holds a block of 1e-20 magnitudes


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _init(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) for s in shapes], g


def _grads(shapes, g, it, scale=SCALE):
    """float32 gradients of step `it`, already multiplied by the loss scale (a power of two: exact)."""
    out = [torch.randn(s, generator=g) * (0.1 + it) for s in shapes]
    if len(shapes) == len(SHAPES):
        out[ZERO_T].zero_()
        out[TINY_T].view(-1)[:300] *= 1e-20
    return [t * scale for t in out]


class _Tracker:
    """Compares a FusedAdam's live parameters and state_dict() moments with an adam_ref after every step and keeps the
    running bounds of the module docstring.  ``keys``: the live parameters' indices in state_dict()['state']."""

    def __init__(self, ref, keys):
        self.ref, self.keys = ref, keys
        self.Bp = [np.zeros_like(q) for q in ref.p]
        self.X = [np.zeros_like(q) for q in ref.p]
        self.Y = [np.zeros_like(q) for q in ref.p]
        self.worst = dict(p=0.0, m=0.0, v=0.0)

    def check(self, params, sd, label):
        ref, t = self.ref, self.ref.t
        b1, b2 = ref.betas
        for i, (p, k) in enumerate(zip(params, self.keys)):
            wb = ref.wd * self.Bp[i]
            self.X[i] = b1 * self.X[i] + (1 - b1) * wb
            self.Y[i] = b2 * self.Y[i] + (1 - b2) * (2 * np.abs(ref.g[i]) + wb) * wb
            tol_m = C_M * t * U * ref.mag[i] + self.X[i] + TINY
            tol_v = C_V * t * U * ref.vmag[i] + self.Y[i] + TINY
            dden = np.minimum(tol_v / (2 * np.sqrt(np.maximum(ref.v[i], 1e-300))), np.sqrt(tol_v)) / np.sqrt(ref.bc2)
            ok = dden < 0.5 * ref.den[i]
            den = np.where(ok, ref.den[i] - dden, ref.den[i])
            first = C_UPD * U * np.abs(ref.upd[i]) + ref.lr / ref.bc1 * tol_m / den + np.abs(ref.upd[i]) * dden / den
            K = np.sqrt(sum((1 - b1) ** 2 * b1 ** (2 * j) / ((1 - b2) * b2 ** j) for j in range(t)) * ref.bc2) / ref.bc1
            self.Bp[i] = self.Bp[i] + U * np.abs(ref.p[i]) + np.minimum(np.where(ok, first, np.inf), 2.002 * ref.lr * K) + 2.0 ** -149
            st = sd['state'][k]
            assert float(st['step']) == t, (label, k, float(st['step']), t)
            for name, got, want, tol in (('p', p, ref.p[i], self.Bp[i]), ('m', st['exp_avg'], ref.m[i], tol_m),
                                         ('v', st['exp_avg_sq'], ref.v[i], tol_v)):
                got = R.f64(got)
                assert got.shape == want.shape and np.isfinite(got).all(), (label, name, i)
                r = float((np.abs(got - want) / tol).max())
                self.worst[name] = max(self.worst[name], r)
                assert r <= 1.0, '%s: %s of tensor %d at step %d is %.2f x its bound' % (label, name, i, t, r)

    def report(self, label):
        print('adam %s: measured / bound  p %.3f  exp_avg %.3f  exp_avg_sq %.3f' %
              (label, self.worst['p'], self.worst['m'], self.worst['v']))


def _tile(params, grads, dev):
    """The gradients as views tiling one flat buffer in parameter order (what the fused backward emits)."""
    buf = torch.cat([g.reshape(-1) for g in grads]).to(dev)
    off = 0
    for p, g in zip(params, grads):
        p.grad = buf[off:off + g.numel()].view_as(g)
        off += g.numel()
    return buf


@pytest.mark.parametrize('wd', [0.0, 1e-2])
@pytest.mark.parametrize('eps', [1e-8, 1e-3])
@pytest.mark.parametrize('betas', [(0.9, 0.999), (0.8, 0.99)])
def test_fused_adam_against_fp64_every_step(dev, betas, eps, wd):
    """12 steps on one group of tensors of 1, 255, 256, 257, 4095, 4096, 4097, 2 * 4096 + 3 and 64x3x3x3 elements
    (one-element tensors, partial last blocks, exact block multiples), lr changed after step 5, grad_scale = 1 / 1024
    on gradients pre-multiplied by 1024.  One tensor's gradient is zero for the whole run (it may move by weight decay
    only: not at all with wd = 0, and never to NaN), one holds 300 values of 1e-20 magnitude (g * g underflows: the
    update is governed by eps).  Parameters and both moments against adam_ref after EVERY step; bounds: module
    docstring."""
    from esrganplus_amd.optim import FusedAdam
    init, g = _init(SHAPES, 7)
    ps = [torch.nn.Parameter(t.to(dev)) for t in init]
    opt = FusedAdam(ps, lr=1e-3, betas=betas, eps=eps, weight_decay=wd)
    ref = R.adam_ref(init, lr=1e-3, betas=betas, eps=eps, weight_decay=wd)
    tr = _Tracker(ref, list(range(len(ps))))
    label = 'betas=%s eps=%g wd=%g' % (betas, eps, wd)
    for it in range(12):
        grads = _grads(SHAPES, g, it)
        _tile(ps, grads, dev)
        opt.step(grad_scale=1.0 / SCALE)
        ref.step(grads, grad_scale=1.0 / SCALE)
        tr.check(ps, opt.state_dict(), label)
        if wd == 0.0:
            assert torch.equal(ps[ZERO_T].detach().cpu(), init[ZERO_T])
            sd = opt.state_dict()['state'][ZERO_T]
            assert not sd['exp_avg'].any() and not sd['exp_avg_sq'].any()
        if it == 4:
            opt.param_groups[0]['lr'] = ref.lr = 5e-4
    assert wd == 0.0 or not torch.equal(ps[ZERO_T].detach().cpu(), init[ZERO_T])
    tr.report(label)


HOST_SHAPES = [(257,), (4097,), (5, 3), (4096,), (1,)]


def _host_case(dev, seed=11, **kw):
    init, g = _init(HOST_SHAPES, seed)
    ps = [torch.nn.Parameter(t.to(dev)) for t in init]
    return init, g, ps


def test_fused_adam_frozen_parameter_in_the_middle(dev):
    """requires_grad=False in the middle of the list: the flat offsets of its neighbours close up, their moments land
    in their own state_dict() slots (indices 0, 1, 3, 4), the frozen tensor keeps its bits and has no state."""
    from esrganplus_amd.optim import FusedAdam
    init, g, ps = _host_case(dev)
    ps[2].requires_grad_(False)
    live = [0, 1, 3, 4]
    opt = FusedAdam(ps, lr=2e-3, weight_decay=1e-2)
    ref = R.adam_ref([init[i] for i in live], lr=2e-3, weight_decay=1e-2)
    tr = _Tracker(ref, live)
    for it in range(4):
        grads = _grads(HOST_SHAPES, g, it)
        for i in live:
            ps[i].grad = grads[i].to(dev)
        opt.step(grad_scale=1.0 / SCALE)
        ref.step([grads[i] for i in live], grad_scale=1.0 / SCALE)
        sd = opt.state_dict()
        assert sorted(sd['state']) == live
        tr.check([ps[i] for i in live], sd, 'frozen')
        assert torch.equal(ps[2].detach().cpu(), init[2])
    tr.report('frozen parameter')


def test_fused_adam_two_parameter_groups(dev):
    """Two groups with their own lr and weight_decay: each is one launch with its own tables and moments; the
    state_dict() indices run on through the groups."""
    from esrganplus_amd.optim import FusedAdam
    init, g, ps = _host_case(dev, seed=12)
    opt = FusedAdam([dict(params=ps[:2], lr=1e-3, weight_decay=0.0), dict(params=ps[2:], lr=3e-3, weight_decay=1e-2)],
                    betas=(0.8, 0.99))
    refs = [R.adam_ref(init[:2], lr=1e-3, betas=(0.8, 0.99)), R.adam_ref(init[2:], lr=3e-3, betas=(0.8, 0.99), weight_decay=1e-2)]
    trs = [_Tracker(refs[0], [0, 1]), _Tracker(refs[1], [2, 3, 4])]
    for it in range(4):
        grads = _grads(HOST_SHAPES, g, it)
        for p, gr in zip(ps, grads):
            p.grad = gr.to(dev)
        opt.step(grad_scale=1.0 / SCALE)
        refs[0].step(grads[:2], grad_scale=1.0 / SCALE)
        refs[1].step(grads[2:], grad_scale=1.0 / SCALE)
        sd = opt.state_dict()
        trs[0].check(ps[:2], sd, 'group 0')
        trs[1].check(ps[2:], sd, 'group 1')
    trs[0].report('group 0')
    trs[1].report('group 1')


def test_fused_adam_flat_grad_argument_and_scattered_gradients(dev):
    """step(flat_grad=buf) with .grad unset, and scattered .grad tensors (staged into one buffer), both against
    adam_ref and bit for bit against the zero-copy tiling views."""
    from esrganplus_amd.optim import FusedAdam
    runs = {}
    for how in ('tiled', 'flat_grad', 'scattered'):
        init, g, ps = _host_case(dev, seed=13)
        opt = FusedAdam(ps, lr=1e-3, eps=1e-3, weight_decay=1e-2)
        ref = R.adam_ref(init, lr=1e-3, eps=1e-3, weight_decay=1e-2)
        tr = _Tracker(ref, list(range(len(ps))))
        for it in range(4):
            grads = _grads(HOST_SHAPES, g, it)
            if how == 'tiled':
                _tile(ps, grads, dev)
                opt.step(grad_scale=1.0 / SCALE)
            elif how == 'flat_grad':
                assert all(p.grad is None for p in ps)
                opt.step(grad_scale=1.0 / SCALE, flat_grad=torch.cat([t.reshape(-1) for t in grads]).to(dev))
            else:
                for p, gr in zip(ps, grads):
                    p.grad = gr.to(dev)
                opt.step(grad_scale=1.0 / SCALE)
            ref.step(grads, grad_scale=1.0 / SCALE)
            tr.check(ps, opt.state_dict(), how)
        tr.report(how)
        sd = opt.state_dict()['state']
        runs[how] = [p.detach().clone() for p in ps] + [sd[k][n] for k in sorted(sd) for n in ('exp_avg', 'exp_avg_sq')]
    for how in ('flat_grad', 'scattered'):
        assert all(torch.equal(a, b) for a, b in zip(runs['tiled'], runs[how])), how


@pytest.mark.parametrize('missing', [0, 2])
def test_fused_adam_refuses_a_live_parameter_without_gradient(dev, missing):
    """One live parameter with grad=None while the others have one: HipExtensionError, and nothing changes —
    parameters, moments and the step count are bit for bit those of before."""
    from esrganplus_amd import _lib as L
    from esrganplus_amd.optim import FusedAdam
    init, g, ps = _host_case(dev, seed=14)
    opt = FusedAdam(ps, lr=1e-3)
    for it in range(2):
        for p, gr in zip(ps, _grads(HOST_SHAPES, g, it)):
            p.grad = gr.to(dev)
        opt.step(grad_scale=1.0 / SCALE)
    before_p = [p.detach().clone() for p in ps]
    before = opt.state_dict()['state']
    for p, gr in zip(ps, _grads(HOST_SHAPES, g, 2)):
        p.grad = gr.to(dev)
    ps[missing].grad = None
    with pytest.raises(L.HipExtensionError):
        opt.step(grad_scale=1.0 / SCALE)
    torch.cuda.synchronize()
    after = opt.state_dict()['state']
    assert all(torch.equal(a, b) for a, b in zip(before_p, [p.detach() for p in ps]))
    for k in before:
        assert float(after[k]['step']) == 2.0
        assert torch.equal(before[k]['exp_avg'], after[k]['exp_avg']) and torch.equal(before[k]['exp_avg_sq'], after[k]['exp_avg_sq'])


def test_fused_adam_device_step_counter_under_the_loss_scaler(dev):
    """Two steps skipped for an inf, then five applied, under a DynamicLossScaler: the device counter ages the bias
    correction by APPLIED steps only, so parameters and moments equal adam_ref run for five steps, and
    state_dict() reports step 5.  The gradients carry the scaler's current scale (a power of two: exact)."""
    from esrganplus_amd.optim import FusedAdam, DynamicLossScaler
    init, g, ps = _host_case(dev, seed=15)
    opt = FusedAdam(ps, lr=1e-3, betas=(0.8, 0.99), weight_decay=1e-2)
    sc = DynamicLossScaler(dev, init_scale=4096.0, interval=1000)
    ref = R.adam_ref(init, lr=1e-3, betas=(0.8, 0.99), weight_decay=1e-2)
    tr = _Tracker(ref, list(range(len(ps))))
    for it in range(7):
        scale = float(sc.state[0])
        assert scale == 4096.0 * 0.5 ** min(it, 2)
        grads = _grads(HOST_SHAPES, g, it, scale=1.0)
        for p, gr in zip(ps, grads):
            p.grad = (gr * scale).to(dev)
        if it < 2:
            ps[1 + it].grad.view(-1)[-1] = float('inf') if it == 0 else float('-inf')
        opt.step(scaler=sc)
        sc.update()
        if it < 2:
            assert all(torch.equal(p.detach().cpu(), t) for p, t in zip(ps, init))
            assert float(opt._g[0]['applied']) == 0.0 and not opt._g[0]['exp_avg'].any() and not opt._g[0]['exp_avg_sq'].any()
        else:
            ref.step(grads)
            tr.check(ps, opt.state_dict(), 'scaler')
    assert ref.t == 5 and all(float(s['step']) == 5.0 for s in opt.state_dict()['state'].values())
    tr.report('device step counter')


# ---- loss scaler: every value is exact ----------------------------------------------------------------------------
BIG = 2048 * 4096 + 4099        # amp_check_kernel's grid is capped at 2048 workgroups of 4096 elements: one element past a
#                                 whole second pass of the grid-stride loop, plus a ragged tail


def _flags(sc):
    return sc.state[4:8].tolist()


def test_scaler_check_on_a_buffer_past_the_grid_cap(dev):
    """check() over 2048 * 4096 + 4099 floats.  All finite, with FLT_MAX, -FLT_MAX, a denormal and -0.0 among them:
    no flag.  Then one inf / -inf / nan at element 0, at the last element of the first grid pass, at the first of the
    second pass and at the very last element: the flag of the slot asked for is 1, the other three stay 0."""
    from esrganplus_amd.optim import DynamicLossScaler
    flt_max = float(np.finfo(np.float32).max)
    host = torch.randn(BIG, generator=torch.Generator().manual_seed(20))
    host[5], host[2048 * 4096 + 7], host[-2], host[123457], host[-1] = flt_max, -flt_max, 1e-45, -0.0, flt_max
    assert host[-2].item() != 0.0 and torch.isfinite(host).all()
    buf = host.to(dev)
    sc = DynamicLossScaler(dev)
    for slot in range(4):
        sc.check(buf, slot=slot)
    assert _flags(sc) == [0.0, 0.0, 0.0, 0.0]
    k = 0
    for pos in (0, 2048 * 4096 - 1, 2048 * 4096, BIG - 1):
        for bad in (float('inf'), float('-inf'), float('nan')):
            slot = k % 4
            k += 1
            keep = buf[pos].item()
            buf[pos] = bad
            sc.check(buf, slot=slot)
            assert _flags(sc) == [1.0 if s == slot else 0.0 for s in range(4)], (pos, bad, slot, _flags(sc))
            buf[pos] = keep
            sc.state[4:8] = 0.0
            sc.check(buf, slot=slot)
            assert _flags(sc) == [0.0, 0.0, 0.0, 0.0], (pos, bad)
    assert float(sc.state[0]) == 1024.0 and sc.state[1:4].tolist() == [0.0, 0.0, 0.0]


def test_scaler_slots_and_the_fifth_optimizer(dev):
    """Four optimizers on one scaler take slots 0-3 in the order of their first step; a fifth is refused.  An overflow
    in slot 2's gradients skips that optimizer's step alone: its parameters and moments keep their bits, the other
    three move."""
    from esrganplus_amd import _lib as L
    from esrganplus_amd.optim import FusedAdam, DynamicLossScaler
    g = torch.Generator().manual_seed(21)
    sc = DynamicLossScaler(dev, init_scale=64.0, interval=1000)
    ps = [[torch.nn.Parameter(torch.randn(s, generator=g).to(dev)) for s in [(300,), (4097,)]] for _ in range(5)]
    opts = [FusedAdam(p, lr=1e-2) for p in ps]

    def give(o):
        for p in ps[o]:
            p.grad = (torch.randn(p.shape, generator=g) * 64.0).to(dev)

    for o in range(4):
        give(o)
        opts[o].step(scaler=sc)
        assert sc.slot_of((id(opts[o]), 0)) == o
    give(4)
    with pytest.raises(L.HipExtensionError):
        opts[4].step(scaler=sc)
    assert _flags(sc) == [0.0, 0.0, 0.0, 0.0]
    sc.update()
    snap = lambda o: [p.detach().clone() for p in ps[o]] + [opts[o]._g[0]['exp_avg'].clone(), opts[o]._g[0]['exp_avg_sq'].clone()]
    before = [snap(o) for o in range(4)]
    for o in range(4):
        give(o)
    ps[2][1].grad[4096] = float('nan')
    for o in range(4):
        opts[o].step(scaler=sc)
    assert _flags(sc) == [0.0, 0.0, 1.0, 0.0]
    after = [snap(o) for o in range(4)]
    for o in range(4):
        same = [torch.equal(a, b) for a, b in zip(before[o], after[o])]
        assert all(same) if o == 2 else not any(same), (o, same)
    assert [float(opts[o].state_dict()['state'][0]['step']) for o in range(4)] == [2.0, 2.0, 1.0, 2.0]
    sc.update()
    assert float(sc.state[0]) == 32.0 and _flags(sc) == [0.0, 0.0, 0.0, 0.0]


def test_scaler_update_sequence_and_count(dev):
    """update(): interval - 1 clean steps leave the scale and count up; an overflow (in any slot) multiplies the scale
    by backoff, zeroes the good-step count and clears the flags; then `interval` clean steps multiply it by growth
    exactly once and the count is back at 0.  count(): step_count advances only while the slot's flag is clear."""
    from esrganplus_amd.optim import DynamicLossScaler
    interval = 4
    sc = DynamicLossScaler(dev, init_scale=256.0, growth=2.0, backoff=0.5, interval=interval)
    read = lambda: (float(sc.state[0]), float(sc.state[2]), _flags(sc))
    for k in range(interval - 1):
        sc.update()
        assert read() == (256.0, float(k + 1), [0.0] * 4)
    bad = torch.tensor([1.0, float('inf')], device=dev)
    sc.check(bad, slot=3)
    assert read() == (256.0, float(interval - 1), [0.0, 0.0, 0.0, 1.0])
    sc.update()
    assert read() == (128.0, 0.0, [0.0] * 4)
    for k in range(interval):
        assert read() == (128.0, float(k), [0.0] * 4)
        sc.update()
    assert read() == (256.0, 0.0, [0.0] * 4)
    sc.update()
    assert read() == (256.0, 1.0, [0.0] * 4)
    # count
    steps = torch.tensor([3.0], device=dev)
    sc.count(steps, slot=1)
    assert steps.item() == 4.0
    sc.check(bad, slot=1)
    sc.count(steps, slot=1)
    assert steps.item() == 4.0              # this slot overflowed: not counted
    sc.count(steps, slot=0)
    assert steps.item() == 5.0              # another slot's flag does not stop this one
    sc.update()
    sc.count(steps, slot=1)
    assert steps.item() == 6.0 and read() == (128.0, 0.0, [0.0] * 4)
