"""RRDBNet / RRDB_Net at upscale 1, 2, 3 and 8 on the GPU: the fold / unfold and 3x shuffle kernels of the x3 up-conv
against their fp64 restatements (tests/scales_refs.py), forward and training passes against the reference's own
(tests/golden/rrdbnet_scales*.npz, tools/gen_scales_golden.py), forward_x8, PSNRStep and ESRGANPlusStep at x2, and
tools/sr_infer.py --scale."""
import ctypes as C
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from esrganplus_amd import synth
from tests import scales_refs as SR
from tests.conftest import checks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = (1, 2, 3, 8)
U = 2.0 ** -24          # fp32 unit roundoff
SENT = 7.0


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _mods():
    from esrganplus_amd import engine as E, _lib as L
    return E, L


def _run(kind, field, st):
    E, L = _mods()
    lst = L.OpList()
    lst.add(kind, field, st)
    lst.run(E.current_stream())
    torch.cuda.synchronize()


def _fold_op(mode, w, b, wf, bf):
    _, L = _mods()
    f = L.esr_fold3()
    f.mode, f.cout, f.cin = mode, w.shape[0], w.shape[1]
    f.w, f.bias, f.wf, f.bf = w.data_ptr(), b.data_ptr(), wf.data_ptr(), bf.data_ptr()
    return f


# ---- fold / unfold ----------------------------------------------------------------------------------------------------
def test_fold_against_the_fp64_sum(dev):
    """Every folded weight is the fp32 sum of 1 to 4 sources: three adds at most, so the error is within
    3 u sum|sources| <= 4 2^-24 sum|sources|; the folded bias is the bias, nine times."""
    _, L = _mods()
    w = synth.normal_like(1, 'fold.w', (64, 64, 3, 3))
    b = synth.normal_like(1, 'fold.b', (64,))
    wd, bd = w.to(dev), b.to(dev)
    wf = torch.full((576, 64, 3, 3), SENT, device=dev)
    bf = torch.full((576 + 8,), SENT, device=dev)
    _run(L.OP_FOLD3, 'fold3', _fold_op(L.FOLD3_FOLD, wd, bd, wf, bf))
    ref, _ = SR.fold3(w.double())
    bound, _ = SR.fold3(w.double().abs())
    err = (wf.cpu().double() - ref).abs()
    print('fold: max err %.3e, max err / (4 u sum|src|) %.3f' % (err.max().item(), (err / (4 * U * bound).clamp_min(1e-300)).max().item()))
    assert (err <= 4 * U * bound).all()
    assert torch.equal(bf[:576].cpu(), b.repeat(9)) and (bf[576:] == SENT).all()
    assert torch.equal(wd.cpu(), w) and torch.equal(bd.cpu(), b)


def test_unfold_is_the_adjoint_of_fold(dev):
    """<fold(w), G> = <w, unfold(G)> on the kernels' fp32 results, inner products in fp64.  A folded weight carries at
    most 3 roundings, an unfolded one 8 (nine terms), and sum fold(|w|) |G| = sum |w| unfold(|G|) = S: the two sides
    differ by at most 11 u S.  And unfold directly against its fp64 restatement, within 8 u unfold(|G|) per element."""
    _, L = _mods()
    w = synth.normal_like(2, 'unfold.w', (64, 64, 3, 3))
    b = synth.normal_like(2, 'unfold.b', (64,))
    G = synth.normal_like(2, 'unfold.G', (576, 64, 3, 3))
    gb = synth.normal_like(2, 'unfold.gb', (576,))
    wd, bd, Gd, gbd = w.to(dev), b.to(dev), G.to(dev), gb.to(dev)
    wf, bf = torch.empty(576, 64, 3, 3, device=dev), torch.empty(576, device=dev)
    gw, gbs = torch.full((64, 64, 3, 3), SENT, device=dev), torch.full((64 + 8,), SENT, device=dev)
    _run(L.OP_FOLD3, 'fold3', _fold_op(L.FOLD3_FOLD, wd, bd, wf, bf))
    _run(L.OP_FOLD3, 'fold3', _fold_op(L.FOLD3_UNFOLD, gw, gbs, Gd, gbd))
    assert (gbs[64:] == SENT).all() and torch.equal(Gd.cpu(), G)
    lhs = (wf.cpu().double() * G.double()).sum().item()
    rhs = (w.double() * gw.cpu().double()).sum().item()
    S = (w.double().abs() * SR.unfold3(G.double().abs())[0]).sum().item()
    print('adjoint: <fold w, G> %.9e  <w, unfold G> %.9e  |diff| %.3e  bound %.3e' % (lhs, rhs, abs(lhs - rhs), 11 * U * S))
    assert abs(lhs - rhs) <= 11 * U * S
    ref, rb = SR.unfold3(G.double(), gb.double())
    ab, abb = SR.unfold3(G.double().abs(), gb.double().abs())
    assert ((gw.cpu().double() - ref).abs() <= 8 * U * ab).all()
    assert ((gbs[:64].cpu().double() - rb).abs() <= 8 * U * abb).all()


# ---- shuffle3 / unshuffle3 -------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _interior(buf, h, w):
    """image pixels of a G32 buffer as NCHW (every channel lane), and everything else"""
    t = buf.t
    inner = t[:, :, 1:h + 1, 1:w + 1, :].permute(0, 1, 4, 2, 3).reshape(buf.B, buf.ng * buf.cpg, h, w)
    rest = torch.ones(t.shape, dtype=torch.bool, device=t.device)
    rest[:, :, 1:h + 1, 1:w + 1, :] = False
    return inner, t[rest]


@pytest.mark.parametrize('prec', ['fp16', 'fp32'])
@pytest.mark.parametrize('h,w', [(5, 7), (1, 1)])
def test_shuffle3_pair_is_a_bit_exact_permutation(dev, prec, h, w):
    """y[b][c][3h+i][3w+j] = z[b][(3i + j) 64 + c][h][w], bit for bit, against the torch index form; nothing outside the
    destination's image pixels changes (the ring the next conv reads as zeros, the rows and columns past the image);
    unshuffle3 is the exact way back.  B = 2, C = 64; 5 x 7 and the 1 x 1 corner."""
    E, L = _mods()
    B = 2
    zb, yb = E.G32(B, 576, h, w, prec, dev), E.G32(B, 64, 3 * h, 3 * w, prec, dev)
    z = synth.normal_like(3, 'shuf.z', (B, 576, h, w)).to(dev).to(zb.tdtype)
    zb.t.fill_(SENT)
    zb.t[:, :, 1:h + 1, 1:w + 1, :] = z.reshape(B, zb.ng, zb.cpg, h, w).permute(0, 1, 3, 4, 2)
    yb.t.fill_(SENT)
    pl = L.esr_pool()
    pl.dtype, pl.mode, pl.B, pl.C, pl.H, pl.W = zb.esr_dtype, L.POOL_SHUFFLE3, B, 64, h, w
    pl.x, pl.y = zb.view(0, 576), yb.view(0, 64)
    _run(L.OP_POOL, 'pool', pl)
    got, rest = _interior(yb, 3 * h, 3 * w)
    assert torch.equal(_bits(got), _bits(SR.shuffle3(z)))
    assert (rest == SENT).all()
    zi, zrest = _interior(zb, h, w)
    assert torch.equal(_bits(zi), _bits(z)) and (zrest == SENT).all()         # the source is untouched
    # the way back, into a fresh buffer
    gxb = E.G32(B, 576, h, w, prec, dev)
    gxb.t.fill_(SENT)
    pl = L.esr_pool()
    pl.dtype, pl.mode, pl.B, pl.C, pl.H, pl.W = zb.esr_dtype, L.POOL_UNSHUFFLE3, B, 64, h, w
    pl.x, pl.g, pl.gx = zb.view(0, 576), yb.view(0, 64), gxb.view(0, 576)
    _run(L.OP_POOL, 'pool', pl)
    back, brest = _interior(gxb, h, w)
    assert torch.equal(_bits(back), _bits(z)) and (brest == SENT).all()
    assert torch.equal(_bits(back), _bits(SR.unshuffle3(SR.shuffle3(z))))


def test_shuffle3_refuses_missing_operands(dev):
    E, L = _mods()
    zb = E.G32(1, 576, 2, 2, 'fp32', dev)
    pl = L.esr_pool()
    pl.dtype, pl.mode, pl.B, pl.C, pl.H, pl.W = zb.esr_dtype, L.POOL_SHUFFLE3, 1, 64, 2, 2
    pl.x = zb.view(0, 576)
    assert L.lib().esr_maxpool2(C.byref(pl), C.c_void_p(E.current_stream())) == -1          # no destination
    pl.y = zb.view(0, 64)
    pl.x = zb.view(0, 64)                                                                   # 64 channels are not 9 x 64
    assert L.lib().esr_maxpool2(C.byref(pl), C.c_void_p(E.current_stream())) == -1


# ---- forward against the reference ------------------------------------------------------------------------------------
def _net(dev, s, variant='codes', nb=1, seed=0):
    from esrganplus_amd import architecture as arch
    cls = arch.RRDBNet if variant == 'codes' else arch.RRDB_Net
    net = cls(3, 3, 64, nb, upscale=s).to(dev)
    net.load_state_dict(synth.rrdbnet_state_dict(nb, seed, upscale=s), strict=True)
    return net


def _eval_input(g, tag):
    sd_seed, x_seed, _ = [int(v) for v in g['seeds']]
    shape = [int(v) for v in g['eval_shape']]
    gain = float(g[tag + '_eval_gain']) if tag + '_eval_gain' in g else 1.0
    return synth.image_batch(x_seed, *shape, name='scales.x.eval') * gain


@pytest.mark.parametrize('tag,s,variant', [('x1', 1, 'codes'), ('x2', 2, 'codes'), ('x3', 3, 'codes'), ('x8', 8, 'codes'),
                                           ('ti3', 3, 'test_image')])
def test_eval_forward_matches_the_reference(dev, golden, tag, s, variant):
    """fp32 against the imported reference: max-abs <= 1e-3 (the project's gate) on an output whose peak is > 0.1; fp16
    against the module's own fp32 output with the 5e-2 of the x4 fp16 forward tests (tests/test_gpu_forward.py)."""
    g = golden('rrdbnet_scales')
    x = _eval_input(g, tag).to(dev)
    ref = g[tag + '_y_eval']
    assert np.abs(ref).max() > 0.1
    net = _net(dev, s, variant).eval()
    with torch.no_grad():
        y = net(x)
    assert tuple(y.shape) == tuple(ref.shape) == (1, 3, s * x.shape[2], s * x.shape[3])
    err = np.abs(y.cpu().numpy() - ref).max()
    print('%s fp32 eval: max|diff| %.3e, |ref| max %.3f' % (tag, err, np.abs(ref).max()))
    assert err <= 1e-3
    with torch.no_grad():
        y16 = net.set_precision('fp16')(x)
    e16 = (y16 - y).abs().max().item()
    print('%s fp16 vs fp32: max|diff| %.3e' % (tag, e16))
    assert e16 <= 5e-2


def _train_case(dev, s, g, monkeypatch=None):
    from oracle import ref_torch as RT
    z_seed = int(np.load(os.path.join(ROOT, 'tests', 'golden', 'rrdbnet_scales.npz'))['seeds'][2])
    # the image seed is the case's own: tools/gen_scales_golden.py takes the first whose LeakyReLU inputs all stay clear of
    # 0 by more than fp32 rounding, where the slope taken, and every gradient behind it, would depend on the summation order
    x_seed, shape = int(g['x_seed']), tuple(int(v) for v in g['shape'])
    net = _net(dev, s).train()
    x = synth.image_batch(x_seed, *shape, name='scales.x.train').to(dev).requires_grad_(True)
    gy = synth.normal_like(x_seed, 'scales.gy.x%d' % s, (shape[0], 3, s * shape[2], s * shape[3])).to(dev)
    z = [synth.normal_like(z_seed, 'scales.z.%d' % i, sh).to(dev) for i, sh in enumerate(RT.noise_shapes(shape, 1, 'codes'))]
    y = net(x, z=z)
    (y * gy).sum().backward()
    return net, x, y


def _check_train_case(net, x, y, g, what):
    """The tolerances of tests/test_gpu_backward.py::test_rrdbnet_param_grads_fp32 for the same quantities."""
    assert np.abs(y.detach().cpu().numpy() - g['y']).max() <= 1e-4
    gxr = g['gx']
    egx = np.abs(x.grad.cpu().numpy() - gxr).max()
    print('%s dL/dx max|diff| %.3e (|ref| max %.3f)' % (what, egx, np.abs(gxr).max()))
    assert egx <= 2e-3 * max(1.0, np.abs(gxr).max())
    params = dict(net.named_parameters())
    tail = [k for k in params if 'RDB' not in k]
    assert sorted('g_' + k for k in tail) == sorted(k for k in g if k.startswith('g_'))
    for k in tail:
        ref = g['g_' + k]
        err = np.abs(params[k].grad.cpu().numpy() - ref).max()
        print('%s %-24s max|diff| %.3e (|ref| max %.3f)' % (what, k, err, np.abs(ref).max()))
        assert err <= 2e-3 * max(1.0, np.abs(ref).max()), (k, err)
    chk = np.stack([checks(p.grad) for p in params.values()])
    rel = np.abs(chk - g['gchk']) / np.maximum(1.0, np.abs(g['gchk'][:, 1:2]))
    assert rel.max() <= 2e-3, (np.unravel_index(rel.argmax(), rel.shape), rel.max())


@pytest.mark.parametrize('s', SCALES)
def test_train_case_matches_the_reference(dev, golden, s):
    """Train mode with the fixture's noise: output, input gradient, the full gradients of every conv outside the dense
    blocks (model.0, LR_conv, the up-convs, HR_conv0, HR_conv1) and the checksums of every parameter's gradient."""
    g = golden('rrdbnet_scales_x%d_train' % s)
    net, x, y = _train_case(dev, s, g)
    if s != 3:
        assert net._weights(dev).subpix == frozenset(net._up_keys())        # the sub-pixel form by default
    _check_train_case(net, x, y, g, 'x%d' % s)


def test_gather_form_at_x2_agrees(dev, golden, monkeypatch):
    """ESR_SUBPIX=0: the up-conv in its gather form (upsample = 1, ks = 3), to the same bounds."""
    _, L = _mods()
    monkeypatch.setenv('ESR_SUBPIX', '0')
    g = golden('rrdbnet_scales_x2_train')
    net, x, y = _train_case(dev, 2, g)
    assert net._weights(dev).subpix == frozenset()
    plan = next(v for k, v in net._plans.items() if k[0] == 'train')[0]
    ups = [o.u.conv for o in plan.fwd.ops.ops if o.kind == L.OP_CONV and o.u.conv.upsample]
    assert [(c.upsample, c.ks) for c in ups] == [(1, 3)]
    _check_train_case(net, x, y, g, 'x2 gather')


def test_fp16_train_case_tracks_fp32_at_x3(dev):
    """The folded up-conv through the fp16 kernels (576-channel conv, weight gradient and input-gradient conv): every
    gradient within the 6e-2 relative l2 of tests/test_gpu_backward.py::test_backward_fp16_close_to_fp32."""
    x = synth.image_batch(3, 2, 3, 12, 12, name='s3.x').to(dev)
    gy = synth.normal_like(3, 's3.gy', (2, 3, 36, 36)).to(dev)
    grads = {}
    for prec in ('fp32', 'fp16'):
        net = _net(dev, 3, seed=3).eval().set_precision(prec)
        (net(x) * gy).sum().backward()
        grads[prec] = {k: p.grad.clone() for k, p in net.named_parameters()}
        net.zero_grad()
        (net(x) * gy).sum().backward()                       # a second pass: the folded gradient scratch starts from zero
        for k, p in net.named_parameters():
            assert (p.grad - grads[prec][k]).abs().max().item() <= 1e-4 * max(1.0, grads[prec][k].abs().max().item()), k
    for k in grads['fp32']:
        a, b = grads['fp32'][k], grads['fp16'][k]
        rel = ((a - b).norm() / a.norm().clamp_min(1e-6)).item()
        assert rel <= 6e-2, (k, rel)


def test_x3_weights_refold_after_an_update(dev):
    """The folded tensor is derived: after load_state_dict and after an in-place optimizer step the forward uses the new
    up-conv weights."""
    net = _net(dev, 3, seed=1).eval()
    x = synth.image_batch(4, 1, 3, 6, 9, name='refold.x').to(dev)
    with torch.no_grad():
        y0 = net(x)
        net.load_state_dict(synth.rrdbnet_state_dict(1, 2, upscale=3))
        y1 = net(x)
        fresh = _net(dev, 3, seed=2).eval()
        assert torch.equal(y1, fresh(x)) and not torch.equal(y0, y1)
        net.model[3].weight.mul_(0.5)
        fresh.model[3].weight.mul_(0.5)
        fresh.invalidate()
        assert torch.equal(net(x), fresh(x)) and not torch.equal(net(x), y1)


# ---- x4 is untouched ----------------------------------------------------------------------------------------------------
def test_default_x4_plans_are_the_same_ops(dev):
    """The launch lists of a default net, by kind and geometry, as they were before the tail took a scale: forward =
    import, fea_conv, the chain, LR_conv, two sub-pixel up-convs, HR_conv0, HR_conv1; the backward's tail = per conv a
    weight gradient and an input-gradient conv, the up-convs' adjoint as the 4x4 / stride-2 conv."""
    _, L = _mods()
    from esrganplus_amd import architecture as arch
    net = arch.RRDBNet(3, 3, 64, 1).to(dev).eval()
    net.load_state_dict(synth.rrdbnet_state_dict(1, 0))
    x = synth.image_batch(1, 1, 3, 8, 12, name='x4.ops').to(dev)
    with torch.no_grad():
        assert tuple(net(x).shape) == (1, 3, 32, 48)
    (plan,) = net._plans.values()
    assert [o.kind for o in plan.ops.ops] == [L.OP_LAYOUT, L.OP_CONV, L.OP_RDB_CHAIN] + [L.OP_CONV] * 5
    convs = [o.u.conv for o in plan.ops.ops if o.kind == L.OP_CONV]
    assert [(c.ks, c.upsample, c.H, c.W) for c in convs] == [(3, 0, 8, 12), (3, 0, 8, 12), (2, 3, 16, 24), (2, 3, 32, 48),
                                                             (3, 0, 32, 48), (3, 0, 32, 48)]
    net(x.requires_grad_(True)).sum().backward()
    tp = next(v for k, v in net._plans.items() if k[0] == 'train')[0]
    tail = tp.bwd.ops[:11]
    assert [o.kind for o in tail] == [L.OP_LAYOUT] + [L.OP_WGRAD, L.OP_CONV] * 5
    assert [(o.u.wgrad.upsample, o.u.wgrad.H, o.u.wgrad.cout) for o in tail[1::2]] == [(0, 32, 3), (0, 32, 64), (1, 32, 64),
                                                                                     (1, 16, 64), (0, 8, 64)]
    assert [(o.u.conv.ks, o.u.conv.stride, o.u.conv.H) for o in tail[2::2]] == [(3, 1, 32), (3, 1, 32), (4, 2, 16), (4, 2, 8),
                                                                               (3, 1, 8)]
    assert tp.scratch_grads == []


# ---- forward_x8 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('s,shape', [(2, (1, 3, 12, 12)), (3, (2, 3, 8, 12)), (8, (1, 3, 6, 6)), (1, (1, 3, 9, 5))])
def test_forward_x8_equals_the_reference_form(dev, s, shape):
    """Bit-identical to functional.x8_reference over the ordinary forward, as the x4 test requires; the module's mode and
    every requires_grad stay as they were."""
    from esrganplus_amd import functional as Fn
    net = _net(dev, s, seed=5).train()
    net.model[0].weight.requires_grad_(False)
    x = synth.image_batch(6, *shape, name='x8s.x').to(dev)
    y = net.forward_x8(x)
    assert net.training and not net.model[0].weight.requires_grad and net.model[0].bias.requires_grad
    assert not y.requires_grad and tuple(y.shape) == (shape[0], 3, s * shape[2], s * shape[3])
    ref_net = _net(dev, s, seed=5).eval()
    with torch.no_grad():
        ref = Fn.x8_reference(ref_net, x)
    assert torch.equal(y, ref)


# ---- the steps ----------------------------------------------------------------------------------------------------------
PSNR_CASES = {'l1_wd0': ('l1', 0.0), 'l2_wd0': ('l2', 0.0), 'l2_wd1e-2': ('l2', 1e-2)}


@pytest.mark.parametrize('case', list(PSNR_CASES))
def test_psnr_step_three_iterations_at_x2(dev, golden, case):
    """tests/test_gpu_psnr_step.py::test_three_iterations_match_the_reference at scale 2 (HR = 2 x LR), the production
    form, with its tolerances: learning rates rtol 1e-12; l_pix within 5e-4 max(1, |ref|); checks(fake_H) within 2e-3;
    gradients after iteration 1 within 1e-2 of each tensor's maximum; after iteration 3 the parameters' checks within
    2e-3 and the stored deltas within mean|d - ref| / mean|ref| <= 0.08."""
    from esrganplus_amd import architecture as arch, train
    from oracle import ref_torch as RT
    g = golden('psnr_steps3_x2')
    assert int(g['scale']) == 2 and [int(v) for v in g['hr_shape'][2:]] == [2 * int(v) for v in g['lr_shape'][2:]]
    crit, wd = PSNR_CASES[case]
    sd = synth.rrdbnet_state_dict(nb=2, seed=int(g['sd_seed']), upscale=2)
    assert list(sd.keys()) == [str(k) for k in g['param_keys']]
    netG = arch.RRDBNet(3, 3, 64, 2, upscale=2).to(dev).train()
    netG.load_state_dict(sd, strict=True)
    st = train.PSNRStep(netG, lr_G=float(g['lr_G']), weight_decay_G=wd, pixel_criterion=crit)
    assert st._manual_ok()
    sched = torch.optim.lr_scheduler.MultiStepLR(st.optimizer_G, [int(v) for v in g['lr_steps']], float(g['lr_gamma']))
    pg = dict(netG.named_parameters())
    (s_lr, s_hr, s_z), (n_lr, n_hr, n_z) = [int(v) for v in g['seeds']], [str(v) for v in g['names']]
    full_grads = [k[len(case) + 6:] for k in g if k.startswith(case + '.grad_model')]
    full_deltas = [k[len(case) + 7:] for k in g if k.startswith(case + '.delta_')]
    assert len(full_grads) == 2 and len(full_deltas) == 3
    for it in range(1, 4):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            sched.step()
        assert np.allclose(st.optimizer_G.param_groups[0]['lr'], g['%s.lr_%d' % (case, it)], rtol=1e-12), it
        lr = synth.image_batch(s_lr + it, *[int(v) for v in g['lr_shape']], name=n_lr).to(dev)
        hr = synth.image_batch(s_hr + it, *[int(v) for v in g['hr_shape']], name=n_hr).to(dev)
        z = [synth.normal_like(s_z + it, '%s.%d' % (n_z, i), sh).to(dev) for i, sh in enumerate(RT.noise_shapes(lr.shape, 2, 'codes'))]
        got = float(st.step(lr, hr, z=z)['l_pix'])
        ref = float(g['%s.l_pix_%d' % (case, it)])
        print('%s iteration %d  l_pix hip %.6f  ref %.6f' % (case, it, got, ref))
        assert abs(got - ref) <= 5e-4 * max(1.0, abs(ref)), (it, got, ref)
        assert tuple(st.fake_H.shape) == tuple(hr.shape)
        ref = g['%s.fake_H_chk_%d' % (case, it)]
        assert np.abs(checks(st.fake_H.detach()) - ref).max() <= 2e-3 * np.abs(ref).max(), it
        if it == 1:
            for row, k in zip(g[case + '.grad_chk'], sd.keys()):
                assert np.abs(checks(pg[k].grad) - row).max() <= 1e-2 * np.abs(row).max(), k
            for k in full_grads:
                ref = g['%s.grad_%s' % (case, k)]
                assert np.abs(pg[k].grad.cpu().numpy() - ref).max() <= 1e-2 * np.abs(ref).max(), k
    st.finish()
    chk = np.stack([checks(pg[k]) for k in sd.keys()])
    assert np.abs(chk - g[case + '.G_chk']).max() <= 2e-3 * np.abs(g[case + '.G_chk']).max()
    for k in full_deltas:
        d = (pg[k].detach().cpu() - sd[k]).numpy()
        ref = g['%s.delta_%s' % (case, k)]
        err = np.abs(d - ref).mean() / np.abs(ref).mean()
        print('%s delta of %-40s mean|d - ref| / mean|ref| = %.3e' % (case, k, err))
        assert err <= 0.08, (k, err)
    with torch.no_grad():
        assert tuple(st.test(lr).shape) == tuple(hr.shape)


def test_esrgan_plus_step_at_x2_against_torch_autograd(dev):
    """One ESRGANPlusStep (the hand-written step) with an x2 generator — LR 64 x 64 -> HR 128 x 128 for
    Discriminator_VGG_128 — against the reference's call pattern (SRRaGAN_model.py:113-168) restated with stock torch
    pieces over copies of the same modules: torch.optim.Adam, nn.L1Loss, BCEWithLogitsLoss, loss.backward().  The bounds
    of tests/test_gpu_train_step.py for the same comparison: logs within 2e-4 max(1, |ref|), fake_H within 1e-4, the
    weights' checks after Adam within 2e-3, the sign of the first update of model.0.weight agreeing on >= 97 %."""
    from esrganplus_amd import architecture as arch, train
    from oracle import ref_torch as RT
    sdG, sdD = synth.rrdbnet_state_dict(nb=1, seed=30, upscale=2), synth.discriminator_state_dict(seed=31)

    def nets():
        netG = arch.RRDBNet(3, 3, 64, 1, upscale=2).to(dev).train()
        netD = arch.Discriminator_VGG_128(3, 64).to(dev).train()
        netF = arch.VGGFeatureExtractor(34, False, True, dev).to(dev).eval()
        netG.load_state_dict(sdG, strict=True)
        netD.load_state_dict(sdD, strict=True)
        netF.load_state_dict(synth.vgg19_state_dict(6, 34), strict=False)
        return netG, netD, netF
    var_L = synth.image_batch(30, 2, 3, 64, 64, name='step2.lr').to(dev)
    var_H = synth.image_batch(30, 2, 3, 128, 128, name='step2.hr').to(dev)
    z = [synth.normal_like(9, 'step2.z.%d' % i, s).to(dev) for i, s in enumerate(RT.noise_shapes(var_L.shape, 1, 'codes'))]
    # ---- the hand-written step
    netG, netD, netF = nets()
    st = train.ESRGANPlusStep(netG, netD, netF)
    assert st._manual_ok()
    log = st.step(var_L, var_H, z=z)
    fake_step = st.fake_H.detach().clone()
    st.finish()
    # ---- torch autograd over the same modules
    rG, rD, rF = nets()
    cri, bce = torch.nn.L1Loss(), torch.nn.BCEWithLogitsLoss()
    gan = lambda t, real: bce(t, torch.ones_like(t) if real else torch.zeros_like(t))
    oG = torch.optim.Adam(rG.parameters(), lr=1e-4, betas=(0.9, 0.999))
    oD = torch.optim.Adam(rD.parameters(), lr=1e-4, betas=(0.9, 0.999))
    for p in rD.parameters():
        p.requires_grad = False
    fake_H = rG(var_L, z=z)
    assert tuple(fake_H.shape) == tuple(var_H.shape)
    l_g_pix = 1e-2 * cri(fake_H, var_H)
    l_g_fea = cri(rF(fake_H), rF(var_H).detach())
    pred_g_fake, pred_d_real = rD(fake_H), rD(var_H).detach()
    l_g_gan = 5e-3 * (gan(pred_d_real - torch.mean(pred_g_fake), False) + gan(pred_g_fake - torch.mean(pred_d_real), True)) / 2
    (l_g_pix + l_g_fea + l_g_gan).backward()
    oG.step()
    for p in rD.parameters():
        p.requires_grad = True
    oD.zero_grad()
    pred_d_real, pred_d_fake = rD(var_H), rD(fake_H.detach())
    l_d_real, l_d_fake = gan(pred_d_real - torch.mean(pred_d_fake), True), gan(pred_d_fake - torch.mean(pred_d_real), False)
    ((l_d_real + l_d_fake) / 2).backward()
    oD.step()
    ref = dict(l_g_pix=l_g_pix.item(), l_g_fea=l_g_fea.item(), l_g_gan=l_g_gan.item(), l_d_real=l_d_real.item(),
               l_d_fake=l_d_fake.item(), D_real=pred_d_real.mean().item(), D_fake=pred_d_fake.mean().item())
    for k, v in ref.items():
        print('%-9s step %.6e  autograd %.6e' % (k, float(log[k]), v))
        assert abs(float(log[k]) - v) <= 2e-4 * max(1.0, abs(v)), k
    assert (fake_step - fake_H.detach()).abs().max().item() <= 1e-4
    for a, b in ((netG, rG), (netD, rD)):
        pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
        ca, cb = np.stack([checks(pa[k]) for k in pa]), np.stack([checks(pb[k]) for k in pa])
        assert np.abs(ca - cb).max() <= 2e-3 * np.abs(cb).max()
    da = (dict(netG.named_parameters())['model.0.weight'].detach().cpu() - sdG['model.0.weight']).numpy()
    db = (dict(rG.named_parameters())['model.0.weight'].detach().cpu() - sdG['model.0.weight']).numpy()
    assert np.mean(np.sign(da) == np.sign(db)) >= 0.97


# ---- the inference script ---------------------------------------------------------------------------------------------
def test_sr_infer_scale_2(dev, tmp_path, golden):
    """tools/sr_infer.py --scale 2 on one bundled LR image with synthetic weights: the output is 2 x the input and equals
    the module's own forward; --tile with it exits with the library's message."""
    from PIL import Image
    from esrganplus_amd import architecture as arch
    g = golden('sr_infer')
    name = 'butterfly'
    lr = g['lr_' + name]
    in_dir, out_dir = tmp_path / 'LR', tmp_path / 'results'
    in_dir.mkdir()
    Image.fromarray(lr).save(str(in_dir / (name + '.png')))
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'sr_infer.py'), 'synthetic', str(in_dir), str(out_dir), 'fp32']
    r = subprocess.run(cmd + ['--scale', '2'], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.array(Image.open(str(out_dir / (name + '_rlt.png'))).convert('RGB'))
    assert got.shape == (2 * lr.shape[0], 2 * lr.shape[1], 3)
    net = arch.RRDB_Net(3, 3, 64, 23, upscale=2)
    net.load_state_dict(synth.rrdbnet_state_dict(23, 0, upscale=2), strict=True)
    net = net.eval().to(dev)
    x = torch.from_numpy(np.transpose(lr.astype(np.float64) / 255, (2, 0, 1))).float().unsqueeze(0).to(dev)
    with torch.no_grad():
        y = net(x).squeeze().cpu().clamp_(0, 1).numpy()
    want = (np.transpose(y, (1, 2, 0)) * 255.0).round().astype(np.uint8)
    assert len(np.unique(want)) > 16 and np.array_equal(got, want)
    r = subprocess.run(cmd + ['--scale=2', '--tile', '64'], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and 'x4-only' in r.stderr
