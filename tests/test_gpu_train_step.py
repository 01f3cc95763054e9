"""One full ESRGAN+ optimisation step on the HIP path vs the golden captured from the reference's
``SRRaGANModel.optimize_parameters`` (nb=2, batch 4; oracle/gen_golden.py: gen_train_step)."""
import os

import numpy as np
import pytest
import torch

from esrganplus_amd import synth
from tests.conftest import GOLDEN, checks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def test_optimize_parameters_step_matches_reference():
    assert torch.cuda.is_available()
    dev = torch.device('cuda:0')
    from esrganplus_amd import architecture as arch, train
    from oracle import ref_torch as RT
    g = dict(np.load(os.path.join(GOLDEN, 'train_step.npz')))
    sdG, sdD = synth.rrdbnet_state_dict(nb=2, seed=30), synth.discriminator_state_dict(seed=31)
    netG = arch.RRDBNet(3, 3, 64, 2).to(dev).train()
    netD = arch.Discriminator_VGG_128(3, 64).to(dev).train()
    netF = arch.VGGFeatureExtractor(34, False, True, dev).to(dev).eval()
    netG.load_state_dict(sdG, strict=True)
    netD.load_state_dict(sdD, strict=True)
    netF.load_state_dict(synth.vgg19_state_dict(6, 34), strict=False)
    lr = synth.image_batch(30, 4, 3, 32, 32, name='step.lr').to(dev)
    hr = synth.image_batch(30, 4, 3, 128, 128, name='step.hr').to(dev)
    z = [synth.normal_like(9, 'step.z.%d' % i, s).to(dev) for i, s in enumerate(RT.noise_shapes(lr.shape, 2, 'codes'))]
    st = train.ESRGANPlusStep(netG, netD, netF)
    log = st.step(lr, hr, z=z)
    for k in ('l_g_pix', 'l_g_fea', 'l_g_gan', 'l_d_real', 'l_d_fake', 'D_real', 'D_fake'):
        ref = float(g['log_' + k])
        print('%-9s hip %.6e  ref %.6e' % (k, log[k], ref))
        assert abs(log[k] - ref) <= 2e-4 * max(1.0, abs(ref)), k
    assert np.abs(st.fake_H.detach().cpu().numpy()[:, :, ::4, ::4] - g['fake_H_sub4']).max() <= 1e-4
    # Adam's first step moves every weight by ~lr*sign(grad): compare the updated weights
    pg = dict(netG.named_parameters())
    chk = np.stack([checks(pg[k]) for k in sdG.keys()])
    assert np.abs(chk - g['G_new_chk']).max() <= 2e-3 * np.abs(g['G_new_chk']).max()
    d = (pg['model.0.weight'].detach().cpu() - sdG['model.0.weight']).numpy()
    ref = g['G_delta_model.0.weight']
    agree = np.mean(np.sign(d) == np.sign(ref))
    print('sign agreement of the first Adam update on model.0.weight: %.4f' % agree)
    assert agree >= 0.97 and np.abs(d - ref).mean() <= 0.1 * np.abs(ref).mean()
    pd = dict(netD.named_parameters())
    dd = (pd['classifier.2.weight'].detach().cpu() - sdD['classifier.2.weight']).numpy()
    assert np.mean(np.sign(dd) == np.sign(g['D_delta_classifier.2.weight'])) >= 0.97


@pytest.mark.parametrize('knobs', [{}, {'PIPELINED': '1'}, {'ESR_TRAIN_NETF_SIDE': '0', 'ESR_TRAIN_DSTEP': 'first'}, {'ESR_TRAIN_MANUAL': '0'},
                                   {'ESR_TRAIN_DSPLIT': '0'}, {'ESR_TRAIN_DSPLIT': '1', 'ESR_TRAIN_DSTEP': 'mid', 'PIPELINED': '1'},
                                   {'ESR_FUSE_BN': '0', 'ESR_S2_SPLIT': '0'},      # two-stage netD forward over the unfused BatchNorm launches
                                   {'ESR_TRAIN_MANUAL': '0', 'ESR_SHARED_D': '0', 'ESR_TRAIN_OVERLAP': '0', 'ESR_FLAT_GRADS': '0',
                                    'ESR_FUSE_BN': '0', 'ESR_S2_SPLIT': '0'}])
def test_three_training_iterations_match_the_reference(monkeypatch, knobs):
    """Three iterations of the reference's loop body (codes/train.py:97-106) — MultiStepLR([1, 2]) stepped BEFORE the
    optimizers, fresh data and noise per step — against the imported SRRaGANModel (tests/golden/train_steps3.npz,
    oracle/gen_golden.py: gen_train_steps3): the seven logged losses per step, the learning rates, the weights after
    the third Adam step (moments + bias correction over steps), and the discriminator's BatchNorm buffers after its 12
    training forwards.  Runs the production step (hand-written forward / backward over the launch lists, shared netD forward, stream overlap,
    flat gradient store, fused BatchNorm passes, split-K deep convs), the same through autograd, and the plain one
    (every knob off)."""
    pipelined = knobs.get('PIPELINED') == '1'      # step(sync_log=False) + finish(): the D-side tail stays on the side stream
    for k, v in knobs.items():
        if k != 'PIPELINED':
            monkeypatch.setenv(k, v)
    from esrganplus_amd import architecture as arch, train
    from oracle import ref_torch as RT
    monkeypatch.setattr(arch._RRDBNetBase, 'flat_param_grads', knobs.get('ESR_FLAT_GRADS', '1') != '0')
    assert torch.cuda.is_available()
    dev = torch.device('cuda:0')
    g = dict(np.load(os.path.join(GOLDEN, 'train_steps3.npz')))
    sdG, sdD = synth.rrdbnet_state_dict(nb=2, seed=32), synth.discriminator_state_dict(seed=33)
    netG = arch.RRDBNet(3, 3, 64, 2).to(dev).train()
    netD = arch.Discriminator_VGG_128(3, 64).to(dev).train()
    netF = arch.VGGFeatureExtractor(34, False, True, dev).to(dev).eval()
    netG.load_state_dict(sdG, strict=True)
    netD.load_state_dict(sdD, strict=True)
    netF.load_state_dict(synth.vgg19_state_dict(6, 34), strict=False)
    st = train.ESRGANPlusStep(netG, netD, netF)
    scheds = [torch.optim.lr_scheduler.MultiStepLR(o, [1, 2], 0.5) for o in (st.optimizer_G, st.optimizer_D)]
    import warnings
    keys = ('l_g_pix', 'l_g_fea', 'l_g_gan', 'l_d_real', 'l_d_fake', 'D_real', 'D_fake')
    logs = []
    for it in range(1, 4):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            for sch in scheds:
                sch.step()                              # the reference's order: scheduler first (train.py:102)
        lrs = np.array([st.optimizer_G.param_groups[0]['lr'], st.optimizer_D.param_groups[0]['lr']])
        assert np.allclose(lrs, g['lr_%d' % it], rtol=1e-12), (it, lrs)
        lr = synth.image_batch(70 + it, 4, 3, 32, 32, name='steps3.lr').to(dev)
        hr = synth.image_batch(80 + it, 4, 3, 128, 128, name='steps3.hr').to(dev)
        z = [synth.normal_like(90 + it, 'steps3.z.%d' % i, s).to(dev)
             for i, s in enumerate(RT.noise_shapes(lr.shape, 2, 'codes'))]
        if pipelined:                                   # three steps back to back, nothing read in between
            logs.append(dict(st.step(lr, hr, z=z, sync_log=False)))
        else:
            logs.append(st.step(lr, hr, z=z))
        assert np.abs(checks(st.fake_H.detach()) - g['fake_H_chk_%d' % it]).max() <= 2e-3 * np.abs(g['fake_H_chk_%d' % it]).max()
    st.finish()
    for it in range(1, 4):
        got = np.array([float(logs[it - 1][k]) for k in keys])
        ref = g['log_%d' % it]
        print('step %d  hip %s\n        ref %s' % (it, got, ref))
        # (steps 2 and 3 run on weights that already differ in the last bits: 5e-4 of the value, 2e-4 absolute)
        assert np.all(np.abs(got - ref) <= 5e-4 * np.maximum(1.0, np.abs(ref))), (it, got - ref)
    pg, pd = dict(netG.named_parameters()), dict(netD.named_parameters())
    chk = np.stack([checks(pg[k]) for k in sdG.keys()])
    assert np.abs(chk - g['G_chk']).max() <= 2e-3 * np.abs(g['G_chk']).max()
    chk = np.stack([checks(pd[k]) for k in pd.keys()])
    assert np.abs(chk - g['D_chk']).max() <= 2e-3 * np.abs(g['D_chk']).max()
    for net, sd, k in ((pg, sdG, 'G_delta_model.0.weight'), (pg, sdG, 'G_delta_model.1.sub.1.RDB2.conv3.0.bias'),
                       (pd, sdD, 'D_delta_classifier.2.weight'), (pd, sdD, 'D_delta_features.3.weight')):
        name = k.split('_delta_')[1]
        d = (net[name].detach().cpu() - sd[name]).numpy()
        ref = g[k]
        # three Adam steps of ~lr each: the accumulated update must agree (a wrong bias correction, a scheduler
        # stepped after the optimizer or a stale moment changes it by tens of percent)
        err = np.abs(d - ref).mean() / np.abs(ref).mean()
        print('%-45s mean|delta - ref| / mean|ref| = %.3e' % (k, err))
        assert err <= 0.08, (k, err)
    bufs = dict(netD.named_buffers())
    for k in ('features.3', 'features.15', 'features.27'):
        # (after three optimizer steps the weights differ from the reference's in the last bits and the deep layers'
        # statistics with them: 1e-3; the ORDER of the four updates per step is pinned at 1e-5 by
        # test_discriminator_forward_shared_matches_four_calls)
        em = np.abs(bufs[k + '.running_mean'].cpu().numpy() - g['rm_' + k]).max() / max(1.0, np.abs(g['rm_' + k]).max())
        ev = np.abs(bufs[k + '.running_var'].cpu().numpy() - g['rv_' + k]).max() / max(1.0, np.abs(g['rv_' + k]).max())
        print('%s running_mean err %.2e running_var err %.2e' % (k, em, ev))
        assert em <= 1e-3 and ev <= 1e-3, (k, em, ev)
    nbt = np.array([int(bufs[k]) for k in bufs if k.endswith('num_batches_tracked')])
    assert (nbt == g['nbt']).all() and (nbt == 12).all()


@pytest.mark.parametrize('flat', [True, False])
def test_fused_adam_matches_torch_adam(dev, flat):
    """optim.FusedAdam (one HIP launch) vs torch.optim.Adam over 4 steps, with a loss-scale folded in;
    gradients either as views tiling one flat buffer (the fused backward's layout) or scattered."""
    from esrganplus_amd.optim import FusedAdam
    shapes = [(64, 3, 3, 3), (64,), (32, 64, 3, 3), (32,), (5000,), (1,), (100, 8192)]
    torch.manual_seed(0)
    ps = [torch.randn(s, device=dev) for s in shapes]
    pa = [torch.nn.Parameter(p.clone()) for p in ps]
    pb = [torch.nn.Parameter(p.clone()) for p in ps]
    oa = FusedAdam(pa, lr=1e-3, betas=(0.9, 0.999), weight_decay=0.0)
    ob = torch.optim.Adam(pb, lr=1e-3, betas=(0.9, 0.999))
    scale = 1024.0
    for it in range(4):
        gs = [torch.randn(s, device=dev) * (0.1 + it) for s in shapes]
        if flat:
            buf = torch.cat([g.reshape(-1) for g in gs]) * scale
            off = 0
            for p, g in zip(pa, gs):
                p.grad = buf[off:off + g.numel()].view_as(g)
                off += g.numel()
        else:
            for p, g in zip(pa, gs):
                p.grad = g * scale
        for p, g in zip(pb, gs):
            p.grad = g.clone()
        oa.step(grad_scale=1.0 / scale)
        ob.step()
        if it == 1:                      # scheduler-style lr change must be honoured
            for o in (oa, ob):
                o.param_groups[0]['lr'] = 5e-4
    for a, b in zip(pa, pb):
        assert (a - b).abs().max().item() <= 2e-6 * max(1.0, b.abs().max().item())


def test_graph_replay_matches_per_op_launches(dev, monkeypatch):
    """ESR_GRAPH=1: forward/backward launch lists replayed as captured hipGraphs (static I/O buffers,
    Philox seed read from device memory) must reproduce the per-op path (bit for bit where the arithmetic is deterministic)."""
    from esrganplus_amd import architecture as arch

    def run(graph):
        monkeypatch.setenv('ESR_GRAPH', '1' if graph else '0')
        torch.manual_seed(123)
        netG = arch.RRDBNet(3, 3, 64, 2).to(dev).train().set_precision('fp16')
        netG.load_state_dict(synth.rrdbnet_state_dict(nb=2, seed=30))
        netD = arch.Discriminator_VGG_128(3, 64).to(dev).train().set_precision('fp16')
        netD.load_state_dict(synth.discriminator_state_dict(seed=31))
        x = synth.image_batch(7, 2, 3, 32, 32, name='g.x').to(dev)
        outs = []
        for _ in range(2):                                # second pass = graph REPLAY
            netG.zero_grad(set_to_none=True)
            netD.zero_grad(set_to_none=True)
            y = netG(x)
            d = netD(y)
            (y.mean() + d.mean()).backward()
            outs.append((y.detach().clone(), d.detach().clone(),
                         netG.model[0].weight.grad.clone(), netD.features[0].weight.grad.clone()))
        return outs

    a, b = run(False), run(True)
    for ta, tb in zip(a, b):
        assert torch.equal(ta[0], tb[0])                  # generator forward: deterministic, bit-exact
        for u, v in zip(ta[1:], tb[1:]):                  # BN sums / weight gradients use float atomics
            assert (u.float() - v.float()).abs().max().item() <= 2e-3 * max(1e-6, v.float().abs().max().item())


def test_fused_adam_state_dict_interchanges_with_torch_adam(dev, tmp_path):
    """`.state` resume files (base_model.py:66-85): FusedAdam -> state_dict -> torch.optim.Adam and back
    must continue the very same trajectory."""
    from esrganplus_amd.optim import FusedAdam
    from esrganplus_amd import checkpoint as ck
    torch.manual_seed(1)
    shapes = [(16, 3, 3, 3), (16,), (700,)]
    init = [torch.randn(s, device=dev) for s in shapes]
    grads = [[torch.randn(s, device=dev) for s in shapes] for _ in range(4)]

    def mk(cls):
        ps = [torch.nn.Parameter(t.clone()) for t in init]
        return ps, cls(ps, lr=1e-3, betas=(0.9, 0.999))

    def step(ps, opt, gs):
        for p, g in zip(ps, gs):
            p.grad = g.clone()
        opt.step()

    pf, of = mk(FusedAdam)
    sched = torch.optim.lr_scheduler.MultiStepLR(of, [1, 3], 0.5)
    for k in range(2):
        step(pf, of, grads[k])
        sched.step()
    ck.save_training_state(str(tmp_path / 's.state'), 0, 2, [of], [sched])
    rs = torch.load(str(tmp_path / 's.state'), weights_only=False)
    # resume into torch's Adam and into a fresh FusedAdam: both must match continuing the original
    pt, ot = mk(torch.optim.Adam)
    pn, on = mk(FusedAdam)
    for ps in (pt, pn):
        for p, q in zip(ps, pf):
            p.data.copy_(q.data)
    st, sn = torch.optim.lr_scheduler.MultiStepLR(ot, [1, 3], 0.5), torch.optim.lr_scheduler.MultiStepLR(on, [1, 3], 0.5)
    ck.resume_training(rs, [ot], [st])
    ck.resume_training(rs, [on], [sn])
    for k in range(2, 4):
        for ps, o, s in ((pf, of, sched), (pt, ot, st), (pn, on, sn)):
            step(ps, o, grads[k])
            s.step()
    for a, b, c in zip(pf, pt, pn):
        assert (a - b).abs().max().item() <= 2e-6 and (a - c).abs().max().item() <= 1e-7


def _step_nets(dev, prec):
    from esrganplus_amd import architecture as arch
    sdG, sdD = synth.rrdbnet_state_dict(nb=2, seed=30), synth.discriminator_state_dict(seed=31)
    netG = arch.RRDBNet(3, 3, 64, 2).to(dev).train().set_precision(prec)
    netD = arch.Discriminator_VGG_128(3, 64).to(dev).train().set_precision(prec)
    netF = arch.VGGFeatureExtractor(34, False, True, dev).to(dev).eval().set_precision(prec)
    netG.load_state_dict(sdG, strict=True)
    netD.load_state_dict(sdD, strict=True)
    netF.load_state_dict(synth.vgg19_state_dict(6, 34), strict=False)
    return netG, netD, netF, sdG, sdD


@pytest.mark.parametrize('scale', [1024.0, 'dynamic'])
def test_optimize_parameters_step_fp16_loss_scaled(dev, scale):
    """BASELINE configs[2] as stated — the same golden `optimize_parameters` step in fp16 storage with loss
    scaling (static 1024, and the dynamic scaler): losses within 2e-2 relative of the reference's fp32 values,
    the first Adam update agrees in sign with the reference's on >= 95 % of a weight tensor, everything finite."""
    from esrganplus_amd import train
    from oracle import ref_torch as RT
    g = dict(np.load(os.path.join(GOLDEN, 'train_step.npz')))
    netG, netD, netF, sdG, sdD = _step_nets(dev, 'fp16')
    lr = synth.image_batch(30, 4, 3, 32, 32, name='step.lr').to(dev)
    hr = synth.image_batch(30, 4, 3, 128, 128, name='step.hr').to(dev)
    z = [synth.normal_like(9, 'step.z.%d' % i, s).to(dev) for i, s in enumerate(RT.noise_shapes(lr.shape, 2, 'codes'))]
    st = train.ESRGANPlusStep(netG, netD, netF, loss_scale=scale)
    log = st.step(lr, hr, z=z)
    for k in ('l_g_pix', 'l_g_fea', 'l_g_gan', 'l_d_real', 'l_d_fake'):
        ref = float(g['log_' + k])
        print('%-9s hip fp16 %.6e  ref %.6e' % (k, log[k], ref))
        assert np.isfinite(log[k]) and abs(log[k] - ref) <= 2e-2 * max(1e-3, abs(ref)), k
    pg = dict(netG.named_parameters())
    for k, v in pg.items():
        assert torch.isfinite(v).all(), k
    d = (pg['model.0.weight'].detach().cpu() - sdG['model.0.weight']).numpy()
    agree = np.mean(np.sign(d) == np.sign(g['G_delta_model.0.weight']))
    print('sign agreement of the first Adam update (fp16, scale %s): %.4f' % (scale, agree))
    assert agree >= 0.95
    pd = dict(netD.named_parameters())
    dd = (pd['classifier.2.weight'].detach().cpu() - sdD['classifier.2.weight']).numpy()
    assert np.mean(np.sign(dd) == np.sign(g['D_delta_classifier.2.weight'])) >= 0.95
    if scale == 'dynamic':
        assert float(st.scaler.state[0]) == 1024.0 and float(st.scaler.state[1]) == 0.0 and float(st.scaler.state[2]) == 1.0


def test_dynamic_loss_scaler_skips_overflow_step(dev):
    """An inf in the gradients must leave weights AND Adam moments untouched and halve the scale; the next clean
    step updates normally; after `interval` clean steps the scale doubles.  All decided on the device."""
    from esrganplus_amd.optim import FusedAdam, DynamicLossScaler
    torch.manual_seed(1)
    ps = [torch.nn.Parameter(torch.randn(s, device=dev)) for s in [(64, 3, 3, 3), (64,), (5000,)]]
    ref = [p.detach().clone() for p in ps]
    opt = FusedAdam(ps, lr=1e-2)
    sc = DynamicLossScaler(dev, init_scale=256.0, interval=2)
    for p in ps:
        p.grad = torch.randn_like(p) * 256.0
    ps[2].grad[17] = float('inf')
    opt.step(scaler=sc)
    sc.update()
    for p, r in zip(ps, ref):
        assert torch.equal(p.detach(), r)
    assert float(sc.state[0]) == 128.0 and float(opt._g[0]['exp_avg'].abs().max()) == 0.0
    for it in range(2):
        for p in ps:
            p.grad = torch.randn_like(p) * 128.0
        opt.step(scaler=sc)
        sc.update()
    assert all(not torch.equal(p.detach(), r) for p, r in zip(ps, ref))
    assert float(sc.state[0]) == 256.0 and all(torch.isfinite(p).all() for p in ps)


def test_dynamic_loss_scaler_is_per_optimizer_and_keeps_bias_correction(dev):
    """torch.amp.GradScaler semantics: an overflow in ONE optimizer's gradients skips only that
    optimizer's step, and a skipped step does not advance Adam's step count — after the skip the first applied
    update equals torch.optim.Adam's FIRST step (bias correction with t = 1, not t = 2)."""
    from esrganplus_amd.optim import FusedAdam, DynamicLossScaler
    torch.manual_seed(2)
    shapes = [(32, 3, 3, 3), (700,)]
    pa = [torch.nn.Parameter(torch.randn(s, device=dev)) for s in shapes]
    pb = [torch.nn.Parameter(torch.randn(s, device=dev)) for s in shapes]
    ra, rb = [p.detach().clone() for p in pa], [p.detach().clone() for p in pb]
    oa, ob = FusedAdam(pa, lr=1e-2), FusedAdam(pb, lr=1e-2)
    sc = DynamicLossScaler(dev, init_scale=64.0, interval=1000)
    ga = [torch.randn_like(p) for p in pa]
    gb = [torch.randn_like(p) for p in pb]
    for p, g in zip(pa, ga):
        p.grad = g * 64.0
    pa[1].grad[3] = float('nan')
    for p, g in zip(pb, gb):
        p.grad = g * 64.0
    oa.step(scaler=sc)
    ob.step(scaler=sc)
    sc.update()
    assert all(torch.equal(p.detach(), r) for p, r in zip(pa, ra))            # A skipped
    assert all(not torch.equal(p.detach(), r) for p, r in zip(pb, rb))        # B stepped in the same iteration
    assert float(sc.state[0]) == 32.0
    # A's first APPLIED step (second attempt) == torch Adam's first step on the same gradients
    pt = [torch.nn.Parameter(r.clone()) for r in ra]
    ot = torch.optim.Adam(pt, lr=1e-2)
    g2 = [torch.randn_like(p) for p in pa]
    for p, q, g in zip(pa, pt, g2):
        p.grad = g * 32.0
        q.grad = g.clone()
    oa.step(scaler=sc)
    sc.update()
    ot.step()
    for p, q in zip(pa, pt):
        assert (p - q).abs().max().item() <= 2e-6 * max(1.0, q.abs().max().item())
    assert float(oa.state_dict()['state'][0]['step']) == 1.0 and float(ob.state_dict()['state'][0]['step']) == 1.0


@pytest.mark.parametrize('size', [192, 256])
def test_generator_training_tiles_192_256_vs_oracle(dev, size):
    """BASELINE configs[4] tile sizes (mixed 128/192/256 LR tiles; nb=2 here): noise-on generator forward +
    backward with an L1 loss on ONE 192^2 / 256^2 tile, fp32, against the oracle under autograd with the same
    Philox z — output 1e-4, parameter gradients 1e-2 relative (LeakyReLU mask flips, see test_gpu_rdb_chain)."""
    import torch.nn.functional as F
    from esrganplus_amd import architecture as arch, ops
    from oracle import ref_torch as RT
    nb = 2
    sd = synth.rrdbnet_state_dict(nb=nb, seed=52)
    net = arch.RRDBNet(3, 3, 64, nb).to(dev).train()
    net.load_state_dict(sd, strict=True)
    lr = synth.image_batch(52, 1, 3, size, size, name='gt.lr').to(dev)
    hr = synth.image_batch(53, 1, 3, 4 * size, 4 * size, name='gt.hr').to(dev)
    torch.manual_seed(7)
    y = net(lr)
    loss = F.l1_loss(y, hr)
    loss.backward()
    torch.manual_seed(7)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    z = [ops.philox_normal(s, seed, i, dev).cpu() for i, s in enumerate(RT.noise_shapes(lr.shape, nb, 'codes'))]
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    sdr = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    yr = RT.rrdbnet_forward(lr.cpu(), sdr, nb, z, 'codes')
    lr_ref = F.l1_loss(yr, hr.cpu())
    lr_ref.backward()
    assert (y.detach().cpu() - yr.detach()).abs().max().item() <= 1e-4
    assert abs(float(loss.detach()) - float(lr_ref.detach())) <= 1e-5
    for k, p in net.named_parameters():
        ref = sdr[k].grad
        err = (p.grad.cpu() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6)
        assert err <= 1e-2, (k, err)


def test_eval_after_fused_adam_uses_updated_weights(dev):
    """optim.FusedAdam writes the parameters through raw pointers (no version bump): eval() right after a training
    step must re-pack, i.e. validation runs the model that `state_dict()` would save."""
    from esrganplus_amd import architecture as arch
    from esrganplus_amd.optim import FusedAdam
    for prec in ('fp32', 'fp16'):
        net = arch.RRDBNet(3, 3, 64, 1).to(dev).train().set_precision(prec)
        net.load_state_dict(synth.rrdbnet_state_dict(nb=1, seed=8))
        opt = FusedAdam(net.parameters(), lr=1e-2)
        x = synth.image_batch(8, 2, 3, 24, 40, name='stale.x').to(dev)
        net(x).mean().backward()
        opt.step()
        net.eval()
        with torch.no_grad():
            y = net(x)
            fresh = arch.RRDBNet(3, 3, 64, 1).to(dev).eval().set_precision(prec)
            fresh.load_state_dict(net.state_dict())
            y2 = fresh(x)
        assert torch.equal(y, y2), prec


@pytest.mark.parametrize('prec', ['fp16', 'fp32'])
def test_weight_gradients_are_bit_identical_run_to_run(dev, prec):
    """Deterministic two-stage wgrad reduction (esr_wgrad.partial; fp16 kernels and the fp32 parity kernel): G and D
    gradients of two identical backward passes are equal bit for bit (the atomics form, ESR_WGRAD_DET=0, is not)."""
    from esrganplus_amd import architecture as arch
    sd = synth.rrdbnet_state_dict(nb=2, seed=13)
    x = synth.image_batch(13, 4, 3, 32, 32, name='det.x').to(dev)
    gy = synth.normal_like(13, 'det.gy', (4, 3, 128, 128)).to(dev)
    runs = []
    for _ in range(2):
        net = arch.RRDBNet(3, 3, 64, 2).to(dev).eval().set_precision(prec)
        net.load_state_dict(sd)
        (net(x) * gy).sum().backward()
        runs.append(torch.cat([p.grad.reshape(-1) for p in net.parameters()]).clone())
    assert torch.equal(runs[0], runs[1])
    assert torch.isfinite(runs[0]).all() and runs[0].abs().sum() > 0
    dsd = synth.discriminator_state_dict(seed=14)
    xd = synth.image_batch(14, 4, 3, 128, 128, name='det.xd').to(dev)
    gd = synth.normal_like(14, 'det.gd', (4, 1)).to(dev)
    runs = []
    for _ in range(2):
        netD = arch.Discriminator_VGG_128(3, 64).to(dev).train().set_precision(prec)
        netD.load_state_dict(dsd)
        (netD(xd) * gd).sum().backward()
        runs.append(torch.cat([p.grad.reshape(-1) for p in netD.parameters()]).clone())
    assert torch.equal(runs[0], runs[1])


def test_pipelined_steps_equal_synchronised_steps_bit_for_bit():
    """step(sync_log=False) leaves the discriminator-side tail (end of the D step, D's Adam, weight packs) on the side
    stream and enqueues the D step behind the G backward; step() orders everything on the current stream.  Same
    kernels, same order per stream, deterministic reductions: after 12 steps from the same start the two loops must hold
    the same weights, moments and BatchNorm buffers BIT FOR BIT — a missing wait between the streams shows up here."""
    from esrganplus_amd import architecture as arch, train
    dev = torch.device('cuda:0')
    sdG, sdD = synth.rrdbnet_state_dict(nb=2, seed=41), synth.discriminator_state_dict(seed=42)

    def run(pipelined):
        torch.manual_seed(1234)
        netG = arch.RRDBNet(3, 3, 64, 2).to(dev).train().set_precision('fp16')
        netD = arch.Discriminator_VGG_128(3, 64).to(dev).train().set_precision('fp16')
        netF = arch.VGGFeatureExtractor(34, False, True, dev).to(dev).eval().set_precision('fp16')
        netG.load_state_dict(sdG, strict=True)
        netD.load_state_dict(sdD, strict=True)
        netF.load_state_dict(synth.vgg19_state_dict(6, 34), strict=False)
        st = train.ESRGANPlusStep(netG, netD, netF, loss_scale=1024.0)
        for it in range(12):
            lr = synth.image_batch(500 + it, 4, 3, 32, 32, name='pipe.lr').to(dev)
            hr = synth.image_batch(600 + it, 4, 3, 128, 128, name='pipe.hr').to(dev)
            st.step(lr, hr, sync_log=not pipelined)
        st.finish()
        torch.cuda.synchronize()
        out = {'G.' + k: v.detach().clone() for k, v in netG.state_dict().items()}
        out.update({'D.' + k: v.detach().clone() for k, v in netD.state_dict().items()})
        return out

    a, b = run(False), run(True)
    assert a.keys() == b.keys()
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    assert not bad, bad[:8]


def test_networks_join_a_pipelined_steps_tail_at_their_public_entry_points(monkeypatch):
    """after step(sync_log=False) the D step's end, D's Adam and the weight packs are still on the side
    stream.  Without finish(), a validation forward / a checkpoint taken on the CURRENT stream right after the call must
    still see the finished update: the networks' forward / state_dict order that tail in front of their caller's stream
    (block._PlannedModule._join_pending).  Also: a misspelt schedule knob is refused instead of silently dropping the D step."""
    from esrganplus_amd import architecture as arch, train
    dev = torch.device('cuda:0')
    sdG, sdD = synth.rrdbnet_state_dict(nb=1, seed=51), synth.discriminator_state_dict(seed=52)

    def run(explicit_finish):
        torch.manual_seed(4321)                       # (the Philox seeds of the noise layers are drawn from torch's generator)
        netG = arch.RRDBNet(3, 3, 64, 1).to(dev).train().set_precision('fp16')
        netD = arch.Discriminator_VGG_128(3, 64).to(dev).train().set_precision('fp16')
        netF = arch.VGGFeatureExtractor(34, False, True, dev).to(dev).eval().set_precision('fp16')
        netG.load_state_dict(sdG, strict=True)
        netD.load_state_dict(sdD, strict=True)
        netF.load_state_dict(synth.vgg19_state_dict(6, 34), strict=False)
        st = train.ESRGANPlusStep(netG, netD, netF, loss_scale=1024.0)
        for it in range(3):
            lr = synth.image_batch(700 + it, 4, 3, 32, 32, name='join.lr').to(dev)
            hr = synth.image_batch(800 + it, 4, 3, 128, 128, name='join.hr').to(dev)
            st.step(lr, hr, sync_log=False)
        assert netD.__dict__.get('_pending_ev') is not None and netG.__dict__.get('_pending_ev') is not None
        if explicit_finish:
            st.finish()
            torch.cuda.synchronize()
        # no finish(): the reads below are on the current stream, the tail is on the side stream
        sd = {k: v.detach().clone() for k, v in netD.state_dict().items()}
        if not explicit_finish:
            # the event stays for callers on OTHER streams; this stream has joined it once
            pend = netD.__dict__.get('_pending_ev')
            cur = torch.cuda.current_stream()
            assert isinstance(pend, tuple) and (cur.device.index, cur.cuda_stream) in pend[1]
            other = torch.cuda.Stream()
            with torch.cuda.stream(other):              # NOT ordered behind the current stream: only the join orders it
                sd2 = {k: v.detach().clone() for k, v in netD.state_dict().items()}
            other.synchronize()
            assert (other.device.index, other.cuda_stream) in pend[1]
            assert all(torch.equal(sd[k], sd2[k]) for k in sd)
        netD.eval()
        with torch.no_grad():
            y = netD(hr).clone()
        opt = st.state_dict()['optimizers'][1]['state']
        m = {k: v['exp_avg'].detach().clone() for k, v in opt.items()}
        torch.cuda.synchronize()
        return sd, y, m

    (sa, ya, ma), (sb, yb, mb) = run(True), run(False)
    assert all(torch.equal(sa[k], sb[k]) for k in sa) and torch.equal(ya, yb)
    assert ma.keys() == mb.keys() and all(torch.equal(ma[k], mb[k]) for k in ma)
    monkeypatch.setenv('ESR_TRAIN_DSTEP', 'lsat')
    with pytest.raises(ValueError):
        train.ESRGANPlusStep(arch.RRDBNet(3, 3, 64, 1), arch.Discriminator_VGG_128(3, 64),
                             arch.VGGFeatureExtractor(34, False, True, torch.device('cpu')))


@pytest.mark.parametrize('prec', ['fp32', 'fp16'])
def test_optimize_parameters_step_at_full_depth_matches_reference(dev, prec):
    """VERDICT r04 missing #4: ONE `optimize_parameters` step (SRRaGAN_model.py:113-186) of the imported SRRaGANModel at
    the benchmarked depth, nb = 23 (batch 4 of 32x32 LR, explicit z), through the production step.  fp32: the seven
    logged losses, fake_H, the weights after the first Adam step of both networks.  fp16 (storage, loss scale 1024 —
    BASELINE configs[2]'s arithmetic): limits DERIVED from the fp16-storage emulation of the reference's step committed
    with the golden (oracle/gen_golden.py: gen_train_step_full): 2 x its distance from the fp32 losses, with a floor of
    1e-3 of the value (an emulation's error on a mean can be small by cancellation), sign agreement of the first Adam
    update no worse than the emulation's minus 2 %."""
    from esrganplus_amd import architecture as arch, train
    from oracle import ref_torch as RT
    g = dict(np.load(os.path.join(GOLDEN, 'train_step_full.npz')))
    nb = 23
    sdG, sdD = synth.rrdbnet_state_dict(nb=nb, seed=60, gain=0.5), synth.discriminator_state_dict(seed=61)
    netG = arch.RRDBNet(3, 3, 64, nb).to(dev).train().set_precision(prec)
    netD = arch.Discriminator_VGG_128(3, 64).to(dev).train().set_precision(prec)
    netF = arch.VGGFeatureExtractor(34, False, True, dev).to(dev).eval().set_precision(prec)
    netG.load_state_dict(sdG, strict=True)
    netD.load_state_dict(sdD, strict=True)
    netF.load_state_dict(synth.vgg19_state_dict(6, 34), strict=False)
    lr = synth.image_batch(62, 4, 3, 32, 32, name='stepfull.lr').to(dev)
    hr = synth.image_batch(62, 4, 3, 128, 128, name='stepfull.hr').to(dev)
    z = [synth.normal_like(63, 'stepfull.z.%d' % i, s).to(dev) for i, s in enumerate(RT.noise_shapes(lr.shape, nb, 'codes'))]
    st = train.ESRGANPlusStep(netG, netD, netF, loss_scale=1.0 if prec == 'fp32' else 1024.0)
    assert st._manual_ok()                                   # the production (hand-written, two-stream) form of the step
    log = st.step(lr, hr, z=z)
    keys = [str(k) for k in g['keys']]
    got = np.array([log[k] for k in keys])
    ref, emu = g['log'], g['log_fp16emu_err'].copy()
    # (D_real / D_fake are both means of four logits of one network, l_d_real / l_d_fake both BCE means over them: one
    # error scale per pair — the emulation's error on ONE of them is a single draw, 4e-5 on D_real next to 9e-4 on D_fake)
    for a, b in (('D_real', 'D_fake'), ('l_d_real', 'l_d_fake')):
        ia, ib = keys.index(a), keys.index(b)
        emu[ia] = emu[ib] = max(emu[ia], emu[ib])
    lim = 3e-4 * np.maximum(1.0, np.abs(ref)) if prec == 'fp32' else np.maximum(2 * emu, 1e-3 * np.abs(ref))
    for k, a, b, l in zip(keys, got, ref, lim):
        print('%-9s hip %s %.6e  ref %.6e  |diff| %.2e  limit %.2e' % (k, prec, a, b, abs(a - b), l))
    assert np.all(np.isfinite(got)) and np.all(np.abs(got - ref) <= lim), (got - ref, lim)
    fh = st.fake_H.detach().float().cpu().numpy()[:, :, ::4, ::4]
    rng = g['fake_H_sub4'].max() - g['fake_H_sub4'].min()
    efh = np.abs(fh - g['fake_H_sub4']).max() / rng
    print('fake_H max|diff| / range %.2e (fp16-storage emulation: %.2e)' % (efh, float(g['fake_H_fp16emu_err'])))
    assert efh <= (1e-4 if prec == 'fp32' else 2 * float(g['fake_H_fp16emu_err']))
    pg, pd = dict(netG.named_parameters()), dict(netD.named_parameters())
    if prec == 'fp32':
        chk = np.stack([checks(pg[k]) for k in sdG.keys()])
        assert np.abs(chk - g['G_new_chk']).max() <= 2e-3 * np.abs(g['G_new_chk']).max()
        chk = np.stack([checks(pd[k]) for k in pd.keys()])
        assert np.abs(chk - g['D_new_chk']).max() <= 2e-3 * np.abs(g['D_new_chk']).max()
    for i, k in enumerate(str(k) for k in g['probes']):
        d = (pg[k].detach().cpu() - sdG[k]).numpy()
        agree = np.mean(np.sign(d) == np.sign(g['G_delta_' + k]))
        floor = 0.97 if prec == 'fp32' else float(g['G_sign_agree_fp16emu'][i]) - 0.02
        print('G %-40s sign agreement of the first Adam update %.4f (floor %.4f)' % (k, agree, floor))
        assert agree >= floor, (k, agree)
    for i, k in enumerate(('classifier.2.weight', 'features.0.weight', 'features.26.weight')):
        d = (pd[k].detach().cpu() - sdD[k]).numpy()[:8]
        agree = np.mean(np.sign(d) == np.sign(g['D_delta_' + k]))
        floor = 0.95 if prec == 'fp32' else float(g['D_sign_agree_fp16emu'][i]) - 0.03
        print('D %-40s sign agreement %.4f (floor %.4f)' % (k, agree, floor))
        assert agree >= floor, (k, agree)


@pytest.mark.parametrize('scale', [1024.0, 'dynamic'])
def test_resumed_training_continues_bit_for_bit(dev, tmp_path, scale):
    """codes/train.py:162-165 + the resume branch (27-28, 86-91) on the fp16 production step: 3 steps, `save_step`
    ({iter}_G.pth / _D.pth / .state in the reference's layouts + the loss scaler), a FRESH set of networks, optimizers
    and schedulers, `resume_step`, 3 more steps — against 6 uninterrupted steps: every weight, BatchNorm buffer and Adam
    moment bit-identical (fixed noise seeds per step; pipelined calls, so the checkpoint is taken behind work in flight)."""
    from esrganplus_amd import architecture as arch, train, checkpoint as ck
    sdG, sdD = synth.rrdbnet_state_dict(nb=2, seed=81), synth.discriminator_state_dict(seed=82)

    def make():
        netG = arch.RRDBNet(3, 3, 64, 2).to(dev).train().set_precision('fp16')
        netD = arch.Discriminator_VGG_128(3, 64).to(dev).train().set_precision('fp16')
        netF = arch.VGGFeatureExtractor(34, False, True, dev).to(dev).eval().set_precision('fp16')
        netF.load_state_dict(synth.vgg19_state_dict(6, 34), strict=False)
        st = train.ESRGANPlusStep(netG, netD, netF, loss_scale=scale)
        scheds = [torch.optim.lr_scheduler.MultiStepLR(o, [2, 4], 0.5) for o in (st.optimizer_G, st.optimizer_D)]
        return netG, netD, st, scheds

    def steps(st, scheds, lo, hi):
        import warnings
        for it in range(lo, hi):
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                for sch in scheds:
                    sch.step()                              # train.py:102: the schedulers first
            torch.manual_seed(9000 + it)                    # the Philox seeds of the noise layers come from torch's generator
            lr = synth.image_batch(900 + it, 4, 3, 32, 32, name='resume.lr').to(dev)
            hr = synth.image_batch(950 + it, 4, 3, 128, 128, name='resume.hr').to(dev)
            st.step(lr, hr, sync_log=False)

    def snapshot(netG, netD, st):
        st.finish()
        torch.cuda.synchronize()
        out = {'G.' + k: v.detach().clone() for k, v in netG.state_dict().items()}
        out.update({'D.' + k: v.detach().clone() for k, v in netD.state_dict().items()})
        for tag, opt in (('oG', st.optimizer_G), ('oD', st.optimizer_D)):
            for i, e in opt.state_dict()['state'].items():
                out['%s.%s.m' % (tag, i)], out['%s.%s.v' % (tag, i)], out['%s.%s.t' % (tag, i)] = e['exp_avg'], e['exp_avg_sq'], e['step']
        return out

    netG, netD, st, scheds = make()
    netG.load_state_dict(sdG, strict=True)
    netD.load_state_dict(sdD, strict=True)
    steps(st, scheds, 0, 6)
    want = snapshot(netG, netD, st)

    netG, netD, st, scheds = make()
    netG.load_state_dict(sdG, strict=True)
    netD.load_state_dict(sdD, strict=True)
    steps(st, scheds, 0, 3)
    paths = ck.save_step(st, str(tmp_path), epoch=0, iter_step=3, schedulers=scheds)     # no finish() by the caller
    assert [os.path.basename(p) for p in paths] == ['3_G.pth', '3_D.pth', '3.state']
    state = torch.load(paths[2], map_location='cpu')
    assert set(state) >= {'epoch', 'iter', 'schedulers', 'optimizers'} and len(state['optimizers']) == 2
    del netG, netD, st, scheds
    netG, netD, st, scheds = make()                         # default-initialised networks: everything comes from the files
    assert ck.resume_step(st, str(tmp_path), 3, schedulers=scheds) == (0, 3)
    steps(st, scheds, 3, 6)
    got = snapshot(netG, netD, st)
    assert want.keys() == got.keys()
    bad = [k for k in want if not torch.equal(want[k].cpu(), got[k].cpu())]
    assert not bad, bad[:8]


def test_validation_between_pipelined_steps_does_not_disturb_training(dev):
    """codes/train.py:121-159: every `val_freq` iterations the loop runs `model.test()` — netG.eval(), a no_grad forward,
    netG.train() (SRRaGAN_model.py:188-192) — between two optimisation steps.  In a pipelined loop that forward lands
    between a step whose D-side tail is still in flight and the next one, and the train <-> eval flips re-pack weights:
    the trajectory must be the one without validation (bit for bit), and what validation sees must be the eval forward of
    the weights after exactly that many steps."""
    from esrganplus_amd import architecture as arch, train
    sdG, sdD = synth.rrdbnet_state_dict(nb=2, seed=85), synth.discriminator_state_dict(seed=86)
    val_lr = synth.image_batch(990, 1, 3, 40, 24, name='val.lr').to(dev)

    def run(validate_at):
        netG = arch.RRDBNet(3, 3, 64, 2).to(dev).train().set_precision('fp16')
        netD = arch.Discriminator_VGG_128(3, 64).to(dev).train().set_precision('fp16')
        netF = arch.VGGFeatureExtractor(34, False, True, dev).to(dev).eval().set_precision('fp16')
        netG.load_state_dict(sdG, strict=True)
        netD.load_state_dict(sdD, strict=True)
        netF.load_state_dict(synth.vgg19_state_dict(6, 34), strict=False)
        st = train.ESRGANPlusStep(netG, netD, netF, loss_scale=1024.0)
        seen = {}
        for it in range(4):
            torch.manual_seed(7000 + it)
            lr = synth.image_batch(970 + it, 4, 3, 32, 32, name='valrun.lr').to(dev)
            hr = synth.image_batch(980 + it, 4, 3, 128, 128, name='valrun.hr').to(dev)
            st.step(lr, hr, sync_log=False)
            if it + 1 in validate_at:
                netG.eval()
                with torch.no_grad():
                    seen[it + 1] = (netG(val_lr).clone(), {k: v.detach().clone() for k, v in netG.state_dict().items()})
                netG.train()
        st.finish()
        torch.cuda.synchronize()
        out = {'G.' + k: v.detach().clone() for k, v in netG.state_dict().items()}
        out.update({'D.' + k: v.detach().clone() for k, v in netD.state_dict().items()})
        return out, seen

    plain, _ = run(())
    withval, seen = run((2, 3))
    bad = [k for k in plain if not torch.equal(plain[k], withval[k])]
    assert not bad, bad[:8]
    for n, (y, sd) in seen.items():
        ref = arch.RRDBNet(3, 3, 64, 2).to(dev).eval().set_precision('fp16')
        ref.load_state_dict(sd, strict=True)
        with torch.no_grad():
            assert torch.equal(ref(val_lr), y), n


def test_reference_call_pattern_over_the_drop_in_modules_matches_the_golden(dev):
    """INTEGRATION.md section 1 taken literally: the call pattern of `SRRaGANModel.optimize_parameters`
    (SRRaGAN_model.py:113-168) restated call by call with stock torch pieces — torch.optim.Adam, nn.L1Loss, BCEWithLogitsLoss, requires_grad toggles on netD, FOUR separate netD calls,
    two netF calls, loss.backward() — with nothing of this repository but the three drop-in modules.  Against the golden
    step of the imported reference (train_step.npz): losses, fake_H, the weights after Adam, and BatchNorm's
    `num_batches_tracked` = 4."""
    from esrganplus_amd import architecture as arch
    from oracle import ref_torch as RT
    g = dict(np.load(os.path.join(GOLDEN, 'train_step.npz')))
    sdG, sdD = synth.rrdbnet_state_dict(nb=2, seed=30), synth.discriminator_state_dict(seed=31)
    netG = arch.RRDBNet(3, 3, 64, 2).to(dev).train()
    netD = arch.Discriminator_VGG_128(3, 64).to(dev).train()
    netF = arch.VGGFeatureExtractor(34, False, True, dev).to(dev).eval()
    netG.load_state_dict(sdG, strict=True)
    netD.load_state_dict(sdD, strict=True)
    netF.load_state_dict(synth.vgg19_state_dict(6, 34), strict=False)
    var_L = synth.image_batch(30, 4, 3, 32, 32, name='step.lr').to(dev)
    var_H = synth.image_batch(30, 4, 3, 128, 128, name='step.hr').to(dev)
    var_ref = var_H
    z = [synth.normal_like(9, 'step.z.%d' % i, s).to(dev) for i, s in enumerate(RT.noise_shapes(var_L.shape, 2, 'codes'))]
    cri_pix, cri_fea, bce = torch.nn.L1Loss(), torch.nn.L1Loss(), torch.nn.BCEWithLogitsLoss()
    gan = lambda x, real: bce(x, torch.ones_like(x) if real else torch.zeros_like(x))      # loss.py:6-38, 'vanilla'
    optimizer_G = torch.optim.Adam([p for p in netG.parameters() if p.requires_grad], lr=1e-4, betas=(0.9, 0.999))
    optimizer_D = torch.optim.Adam(netD.parameters(), lr=1e-4, betas=(0.9, 0.999))
    # ---- G (SRRaGAN_model.py:114-141)
    for p in netD.parameters():
        p.requires_grad = False
    optimizer_G.zero_grad()
    fake_H = netG(var_L, z=z)                       # (z: the golden's injected normal_() draws)
    l_g_pix = 1e-2 * cri_pix(fake_H, var_H)
    real_fea = netF(var_H).detach()
    fake_fea = netF(fake_H)
    l_g_fea = 1.0 * cri_fea(fake_fea, real_fea)
    pred_g_fake = netD(fake_H)
    pred_d_real = netD(var_ref).detach()
    l_g_gan = 5e-3 * (gan(pred_d_real - torch.mean(pred_g_fake), False) + gan(pred_g_fake - torch.mean(pred_d_real), True)) / 2
    (l_g_pix + l_g_fea + l_g_gan).backward()
    optimizer_G.step()
    # ---- D (143-168)
    for p in netD.parameters():
        p.requires_grad = True
    optimizer_D.zero_grad()
    pred_d_real = netD(var_ref)
    pred_d_fake = netD(fake_H.detach())
    l_d_real = gan(pred_d_real - torch.mean(pred_d_fake), True)
    l_d_fake = gan(pred_d_fake - torch.mean(pred_d_real), False)
    ((l_d_real + l_d_fake) / 2).backward()
    optimizer_D.step()
    log = dict(l_g_pix=l_g_pix.item(), l_g_fea=l_g_fea.item(), l_g_gan=l_g_gan.item(), l_d_real=l_d_real.item(),
               l_d_fake=l_d_fake.item(), D_real=torch.mean(pred_d_real.detach()).item(), D_fake=torch.mean(pred_d_fake.detach()).item())
    for k, v in log.items():
        ref = float(g['log_' + k])
        print('%-9s drop-in %.6e  ref %.6e' % (k, v, ref))
        assert abs(v - ref) <= 2e-4 * max(1.0, abs(ref)), k
    assert np.abs(fake_H.detach().cpu().numpy()[:, :, ::4, ::4] - g['fake_H_sub4']).max() <= 1e-4
    pg, pd = dict(netG.named_parameters()), dict(netD.named_parameters())
    chk = np.stack([checks(pg[k]) for k in sdG.keys()])
    assert np.abs(chk - g['G_new_chk']).max() <= 2e-3 * np.abs(g['G_new_chk']).max()
    chk = np.stack([checks(pd[k]) for k in pd.keys()])
    assert np.abs(chk - g['D_new_chk']).max() <= 2e-3 * np.abs(g['D_new_chk']).max()
    d = (pg['model.0.weight'].detach().cpu() - sdG['model.0.weight']).numpy()
    assert np.mean(np.sign(d) == np.sign(g['G_delta_model.0.weight'])) >= 0.97
    nbt = [int(v) for k, v in netD.named_buffers() if k.endswith('num_batches_tracked')]
    assert nbt and all(n == 4 for n in nbt), nbt
