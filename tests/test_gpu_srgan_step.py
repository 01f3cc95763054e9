"""train.SRGANStep — ``SRGANModel.optimize_parameters`` (codes/models/SRGAN_model.py:113-178) — against the reference's
own model run on the CPU (tests/golden/srgan_step.npz, srgan_steps4.npz, srgan_step_srresnet.npz;
tools/gen_srgan_step_golden.py): both GAN types in both forms, the update schedule, the order of netD's BatchNorm buffer
updates, fp16 storage, the pipelined form, checkpoints, a step without pixel / feature terms, one-rank RCCL, and
``ESRGANPlusStep`` left as it was."""
import os
import socket
import sys
import warnings

import numpy as np
import pytest
import torch

from esrganplus_amd import synth
from tests.conftest import GOLDEN, checks

pytestmark = pytest.mark.gpu

LOG_KEYS = ('l_g_pix', 'l_g_fea', 'l_g_gan', 'l_d_real', 'l_d_fake', 'D_real', 'D_fake')
G_KEYS = LOG_KEYS[:3]
FULL_BUFS = ('features.3', 'features.15', 'features.27')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _nets(dev, prec, seedG=30, seedD=31, netF=True, load=True):
    from esrganplus_amd import architecture as arch
    sdG, sdD = synth.rrdbnet_state_dict(nb=2, seed=seedG), synth.discriminator_state_dict(seed=seedD)
    netG = arch.RRDBNet(3, 3, 64, 2).to(dev).train().set_precision(prec)
    netD = arch.Discriminator_VGG_128(3, 64).to(dev).train().set_precision(prec)
    F_ = None
    if netF:
        F_ = arch.VGGFeatureExtractor(34, False, True, dev).to(dev).eval().set_precision(prec)
        F_.load_state_dict(synth.vgg19_state_dict(6, 34), strict=False)
    if load:
        netG.load_state_dict(sdG, strict=True)
        netD.load_state_dict(sdD, strict=True)
    return netG, netD, F_, sdG, sdD


def _data(dev, seed_lr, seed_hr, seed_z, name, nb=2):
    from oracle import ref_torch as RT
    lr = synth.image_batch(seed_lr, 4, 3, 32, 32, name=name + '.lr').to(dev)
    hr = synth.image_batch(seed_hr, 4, 3, 128, 128, name=name + '.hr').to(dev)
    z = None
    if seed_z is not None:
        z = [synth.normal_like(seed_z, '%s.z.%d' % (name, i), s).to(dev)
             for i, s in enumerate(RT.noise_shapes(lr.shape, nb, 'codes'))]
    return lr, hr, z


def _bn_buffers(netD):
    return [(k, v) for k, v in netD.named_buffers() if k.endswith('running_mean') or k.endswith('running_var')]


def _nbt(netD):
    return np.array([int(v) for k, v in netD.named_buffers() if k.endswith('num_batches_tracked')])


def _check_buffers(netD, g, pre, elem_tol, relative=False):
    """netD's BatchNorm buffers: the checksums of every running statistic within the fixture's D_buf_tol (what
    `elem_tol` per element, the bound of test_discriminator_golden, allows on a sum / abs-sum / L2 norm of C elements;
    the generator asserts that a wrong call order misses it by a factor >= 10), three layers element by element."""
    chk = np.stack([checks(v) for _, v in _bn_buffers(netD)])
    tol = g[pre + 'D_buf_tol'] * (elem_tol / 1e-4)
    r = (np.abs(chk - g[pre + 'D_buf_chk']) / tol).max()
    print('D_buf_chk: worst error / tolerance = %.3f' % r)
    assert r <= 1.0
    bufs = dict(netD.named_buffers())
    for k in FULL_BUFS:
        for what, key in (('running_mean', 'rm_'), ('running_var', 'rv_')):
            ref = g[pre + key + k]
            err = np.abs(bufs[k + '.' + what].cpu().numpy() - ref).max()
            # (one step: absolute, as test_discriminator_golden; several: relative to max(1, |ref|), as the three-iteration test)
            assert err <= elem_tol * (max(1.0, np.abs(ref).max()) if relative else 1.0), (k, what, err)


def _check_one_step(st, log, netG, netD, sdG, sdD, g, pre):
    """The assertions and tolerances of test_optimize_parameters_step_l2_matches_reference, plus the buffers."""
    assert tuple(log) == LOG_KEYS
    for k in LOG_KEYS:
        ref = float(g[pre + 'log_' + k])
        print('%-9s hip %.6e  ref %.6e' % (k, log[k], ref))
        assert abs(log[k] - ref) <= 2e-4 * max(1.0, abs(ref)), k
    assert np.abs(st.fake_H.detach().cpu().numpy()[:, :, ::4, ::4] - g[pre + 'fake_H_sub4']).max() <= 1e-4
    pg = dict(netG.named_parameters())
    chk = np.stack([checks(pg[k]) for k in sdG.keys()])
    assert np.abs(chk - g[pre + 'G_new_chk']).max() <= 2e-3 * np.abs(g[pre + 'G_new_chk']).max()
    d = (pg['model.0.weight'].detach().cpu() - sdG['model.0.weight']).numpy()
    ref = g[pre + 'G_delta_model.0.weight']
    agree = np.mean(np.sign(d) == np.sign(ref))
    print('sign agreement of the first Adam update on model.0.weight: %.4f' % agree)
    assert agree >= 0.97 and np.abs(d - ref).mean() <= 0.1 * np.abs(ref).mean()
    pd = dict(netD.named_parameters())
    dd = (pd['classifier.2.weight'].detach().cpu() - sdD['classifier.2.weight']).numpy()
    assert np.mean(np.sign(dd) == np.sign(g[pre + 'D_delta_classifier.2.weight'])) >= 0.97
    _check_buffers(netD, g, pre, 1e-4)
    assert np.array_equal(_nbt(netD), g[pre + 'num_batches_tracked']) and (_nbt(netD) == 3).all()


@pytest.mark.parametrize('form', ['manual', 'manual_one_stream', 'autograd'])
@pytest.mark.parametrize('gan_type', ['vanilla', 'lsgan'])
def test_srgan_step_matches_reference(monkeypatch, dev, gan_type, form):
    """One step of the reference's SRGANModel per GAN type: hand-driven (with the side stream, and as a plain sequence
    on one stream, ESR_TRAIN_OVERLAP=0) and through autograd (ESR_TRAIN_MANUAL=0).
    l_d_fake is 0.641 under 'vanilla' and 0.0134 under 'lsgan', l_g_gan 3.74e-3 against 6.14e-3: the wrong type, or the
    relativistic term in its place (l_g_gan 4.2e-3, train_step_l2.npz), misses the 2e-4 tolerance by orders of
    magnitude.  netD's buffers pin the call order fake, real, fake (three updates per layer)."""
    from esrganplus_amd import train
    monkeypatch.setenv('ESR_TRAIN_MANUAL', '0' if form == 'autograd' else '1')
    monkeypatch.setenv('ESR_TRAIN_OVERLAP', '0' if form == 'manual_one_stream' else '1')
    g = dict(np.load(os.path.join(GOLDEN, 'srgan_step.npz')))
    netG, netD, netF, sdG, sdD = _nets(dev, 'fp32')
    lr, hr, z = _data(dev, 30, 30, 9, 'step')
    st = train.SRGANStep(netG, netD, netF, pixel_criterion='l2', feature_criterion='l2', gan_type=gan_type)
    assert st._manual_ok() == (form != 'autograd') and st.overlap == (0 if form == 'manual_one_stream' else 1)
    log = st.step(lr, hr, z=z)
    assert st.iteration == 1
    _check_one_step(st, log, netG, netD, sdG, sdD, g, gan_type + '.')


def test_srgan_step_srresnet_generator(dev):
    """``which_model_G: sr_resnet`` (the generator of train_SRGAN.json): the autograd form, same tolerances."""
    from esrganplus_amd import architecture as arch, train
    g = dict(np.load(os.path.join(GOLDEN, 'srgan_step_srresnet.npz')))
    _, netD, netF, _, _ = _nets(dev, 'fp32', load=False)
    sdG = synth.srresnet_state_dict(nb=2, seed=34, upsample_mode='pixelshuffle')
    sdD = synth.discriminator_state_dict(seed=35)
    netG = arch.SRResNet(3, 3, 64, 2, upscale=4, norm_type=None, act_type='relu', mode='CNA',
                         upsample_mode='pixelshuffle').to(dev).train()
    netG.load_state_dict(sdG, strict=True)
    netD.load_state_dict(sdD, strict=True)
    lr, hr, _ = _data(dev, 36, 36, None, 'srgan_srresnet')
    st = train.SRGANStep(netG, netD, netF, pixel_criterion='l2', feature_criterion='l2')
    assert not st._manual_ok()
    log = st.step(lr, hr)
    _check_one_step(st, log, netG, netD, sdG, sdD, g, '')


@pytest.mark.parametrize('manual', ['1', '0'])
def test_four_iterations_with_update_ratio_match_the_reference(monkeypatch, dev, manual):
    """Four iterations of the reference's loop body (scheduler before optimizer, MultiStepLR([2], 0.5)) with
    D_update_ratio 2 and D_init_iters 1, at the tolerances of test_three_training_iterations_match_the_reference: G moves
    at iterations 2 and 4 only — at 1 and 3 every G parameter and Adam(G)'s step count stay bit-identical —, the log has
    no l_g_* key before the first G update and keeps iteration 2's through iteration 3, and netD's buffers count 2 + 3 +
    2 + 3 calls."""
    from esrganplus_amd import train
    monkeypatch.setenv('ESR_TRAIN_MANUAL', manual)
    g = dict(np.load(os.path.join(GOLDEN, 'srgan_steps4.npz')))
    netG, netD, netF, sdG, sdD = _nets(dev, 'fp32', 32, 33)
    st = train.SRGANStep(netG, netD, netF, pixel_criterion='l2', feature_criterion='l2', D_update_ratio=2, D_init_iters=1)
    scheds = [torch.optim.lr_scheduler.MultiStepLR(o, [2], 0.5) for o in (st.optimizer_G, st.optimizer_D)]

    def g_state():
        sd = {k: v.detach().clone() for k, v in netG.state_dict().items()}
        steps = [e['step'].item() for e in st.optimizer_G.state_dict()['state'].values()]
        return sd, steps

    logs = []
    for it in range(1, 5):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            for sch in scheds:
                sch.step()
        lrs = np.array([st.optimizer_G.param_groups[0]['lr'], st.optimizer_D.param_groups[0]['lr']])
        assert np.allclose(lrs, g['lr_%d' % it], rtol=1e-12), (it, lrs)
        lr, hr, z = _data(dev, 70 + it, 80 + it, 90 + it, 'srgan4')
        before = g_state()
        log = dict(st.step(lr, hr, z=z))
        logs.append(log)
        assert st.iteration == it
        assert list(log) == list(g['log_keys_%d' % it]), (it, list(log))
        got, ref = np.array([log[k] for k in log]), g['log_%d' % it]
        print('iteration %d  hip %s\n             ref %s' % (it, got, ref))
        assert np.all(np.abs(got - ref) <= 5e-4 * np.maximum(1.0, np.abs(ref))), (it, got - ref)
        assert np.abs(checks(st.fake_H.detach()) - g['fake_H_chk_%d' % it]).max() <= 2e-3 * np.abs(g['fake_H_chk_%d' % it]).max()
        after = g_state()
        same = all(torch.equal(before[0][k], after[0][k]) for k in before[0])
        if it in (1, 3):
            assert same and before[1] == after[1], 'G moved at iteration %d' % it
        else:
            assert not same and all(s == it // 2 for s in after[1]) and after[1]
    assert not any(k in logs[0] for k in G_KEYS)
    assert [logs[2][k] for k in G_KEYS] == [logs[1][k] for k in G_KEYS]
    pg, pd = dict(netG.named_parameters()), dict(netD.named_parameters())
    chk = np.stack([checks(sdG[k]) for k in sdG.keys()])
    assert np.array_equal(chk, g['G_chk_1'])                     # (the fixture's own statement: iteration 1 left G alone)
    chk = np.stack([checks(pg[k]) for k in sdG.keys()])
    assert np.abs(chk - g['G_chk']).max() <= 2e-3 * np.abs(g['G_chk']).max()
    chk = np.stack([checks(pd[k]) for k in pd.keys()])
    assert np.abs(chk - g['D_chk']).max() <= 2e-3 * np.abs(g['D_chk']).max()
    for net, sd, k in ((pg, sdG, 'G_delta_model.0.weight'), (pg, sdG, 'G_delta_model.1.sub.1.RDB2.conv3.0.bias'),
                       (pd, sdD, 'D_delta_classifier.2.weight'), (pd, sdD, 'D_delta_features.3.weight')):
        name = k.split('_delta_')[1]
        d = (net[name].detach().cpu() - sd[name]).numpy()
        err = np.abs(d - g[k]).mean() / np.abs(g[k]).mean()
        print('%-45s mean|delta - ref| / mean|ref| = %.3e' % (k, err))
        assert err <= 0.08, (k, err)
    _check_buffers(netD, g, '', 1e-3, relative=True)            # (after several optimizer steps: 1e-3, as the three-iteration test)
    assert (_nbt(netD) == 2 + 3 + 2 + 3).all() and np.array_equal(_nbt(netD), g['num_batches_tracked'])


@pytest.mark.parametrize('scale', [1024.0, 'dynamic'])
def test_srgan_step_fp16_loss_scaled(dev, scale):
    """Iteration 1 of the 'vanilla' case in fp16 storage with a static and the dynamic loss scale, at the bounds of
    test_optimize_parameters_step_fp16_loss_scaled."""
    from esrganplus_amd import train
    g = dict(np.load(os.path.join(GOLDEN, 'srgan_step.npz')))
    netG, netD, netF, sdG, sdD = _nets(dev, 'fp16')
    lr, hr, z = _data(dev, 30, 30, 9, 'step')
    st = train.SRGANStep(netG, netD, netF, pixel_criterion='l2', feature_criterion='l2', loss_scale=scale)
    assert st._manual_ok()
    log = st.step(lr, hr, z=z)
    for k in ('l_g_pix', 'l_g_fea', 'l_g_gan', 'l_d_real', 'l_d_fake'):
        ref = float(g['vanilla.log_' + k])
        print('%-9s hip fp16 %.6e  ref %.6e' % (k, log[k], ref))
        assert np.isfinite(log[k]) and abs(log[k] - ref) <= 2e-2 * max(1e-3, abs(ref)), k
    pg = dict(netG.named_parameters())
    for k, v in pg.items():
        assert torch.isfinite(v).all(), k
    d = (pg['model.0.weight'].detach().cpu() - sdG['model.0.weight']).numpy()
    agree = np.mean(np.sign(d) == np.sign(g['vanilla.G_delta_model.0.weight']))
    print('sign agreement of the first Adam update (fp16, scale %s): %.4f' % (scale, agree))
    assert agree >= 0.95
    pd = dict(netD.named_parameters())
    dd = (pd['classifier.2.weight'].detach().cpu() - sdD['classifier.2.weight']).numpy()
    assert np.mean(np.sign(dd) == np.sign(g['vanilla.D_delta_classifier.2.weight'])) >= 0.95
    assert (_nbt(netD) == 3).all()
    if scale == 'dynamic':
        assert float(st.scaler.state[0]) == 1024.0 and float(st.scaler.state[1]) == 0.0 and float(st.scaler.state[2]) == 1.0


def _snapshot(netG, netD, st):
    st.finish()
    torch.cuda.synchronize()
    out = {'G.' + k: v.detach().clone() for k, v in netG.state_dict().items()}
    out.update({'D.' + k: v.detach().clone() for k, v in netD.state_dict().items()})
    for tag, opt in (('oG', st.optimizer_G), ('oD', st.optimizer_D)):
        for i, e in opt.state_dict()['state'].items():
            out['%s.%s.m' % (tag, i)], out['%s.%s.v' % (tag, i)], out['%s.%s.t' % (tag, i)] = e['exp_avg'], e['exp_avg_sq'], e['step']
    return out


def _run_steps(st, dev, lo, hi, name, sync_log):
    for it in range(lo, hi):
        torch.manual_seed(9000 + it)                    # the Philox seeds of the noise layers come from torch's generator
        lr, hr, _ = _data(dev, 900 + it, 950 + it, None, name)
        st.step(lr, hr, sync_log=sync_log)


def test_pipelined_steps_equal_synchronised_steps_and_test_runs_between(dev):
    """step(sync_log=False) x 3 + finish() against three synchronised steps, bit for bit (weights, buffers, both Adam
    states); a ``test()`` between the pipelined steps returns the eval forward of the weights as they stand and leaves
    the modules in training mode."""
    from esrganplus_amd import train

    def run(pipelined):
        netG, netD, netF, _, _ = _nets(dev, 'fp16', 41, 42)
        st = train.SRGANStep(netG, netD, netF, loss_scale=1024.0)
        assert st._manual_ok()
        _run_steps(st, dev, 0, 2, 'srgan.pipe', not pipelined)
        sr = None
        if pipelined:
            x = synth.image_batch(5, 2, 3, 24, 24, name='srgan.pipe.val').to(dev)
            sr = st.test(x)
            assert netG.training and netD.training and sr.shape == (2, 3, 96, 96) and st.fake_H is sr
            netG.eval()
            with torch.no_grad():
                want = netG(x)
            netG.train()
            assert torch.equal(sr, want)
            assert isinstance(st.log['l_d_real'], torch.Tensor) and st.log['l_d_real'].is_cuda
        _run_steps(st, dev, 2, 3, 'srgan.pipe', not pipelined)
        return _snapshot(netG, netD, st)

    a, b = run(False), run(True)
    assert a.keys() == b.keys()
    bad = [k for k in a if not torch.equal(a[k].cpu(), b[k].cpu())]
    assert not bad, bad[:8]


def test_resumed_srgan_training_continues_bit_for_bit(dev, tmp_path):
    """2 iterations, ``save_step``, fresh networks and step, ``resume_step``, 2 more — against 4 uninterrupted ones with
    (D_update_ratio, D_init_iters) = (2, 1): G, D, both Adam states and the BatchNorm buffers bit-identical, and the
    iteration counter restored (else G would move at the wrong iterations after the resume)."""
    from esrganplus_amd import train, checkpoint as ck

    def make(load):
        netG, netD, netF, _, _ = _nets(dev, 'fp16', 81, 82, load=load)
        return netG, netD, train.SRGANStep(netG, netD, netF, loss_scale=1024.0, D_update_ratio=2, D_init_iters=1)

    netG, netD, st = make(True)
    _run_steps(st, dev, 0, 4, 'srgan.resume', False)
    want = _snapshot(netG, netD, st)
    assert st.iteration == 4 and set(want['oG.0.t'].reshape(1).tolist()) == {2.0}

    netG, netD, st = make(True)
    _run_steps(st, dev, 0, 2, 'srgan.resume', False)
    paths = ck.save_step(st, str(tmp_path), epoch=0, iter_step=st.iteration)
    assert [os.path.basename(p) for p in paths] == ['2_G.pth', '2_D.pth', '2.state']
    assert st.state_dict()['iter'] == 2
    del netG, netD, st
    netG, netD, st = make(False)                    # default-initialised networks: everything comes from the files
    assert st.iteration == 0
    assert ck.resume_step(st, str(tmp_path), 2) == (0, 2)
    assert st.iteration == 2
    _run_steps(st, dev, 2, 4, 'srgan.resume', False)
    got = _snapshot(netG, netD, st)
    assert st.iteration == 4 and want.keys() == got.keys()
    bad = [k for k in want if not torch.equal(want[k].cpu(), got[k].cpu())]
    assert not bad, bad[:8]


@pytest.mark.parametrize('manual', ['1', '0'])
def test_step_without_pixel_and_feature_terms(monkeypatch, dev, manual):
    """pixel_weight = 0 and feature_weight = 0 with netF = None: the GAN term alone moves G, l_g_gan is the only G key,
    everything stays finite."""
    from esrganplus_amd import train
    monkeypatch.setenv('ESR_TRAIN_MANUAL', manual)
    netG, netD, _, sdG, _ = _nets(dev, 'fp32', netF=False)
    lr, hr, z = _data(dev, 30, 30, 9, 'step')
    st = train.SRGANStep(netG, netD, None, pixel_weight=0, feature_weight=0)
    assert st._manual_ok() == (manual == '1')
    log = st.step(lr, hr, z=z)
    assert tuple(log) == ('l_g_gan', 'l_d_real', 'l_d_fake', 'D_real', 'D_fake')
    assert all(np.isfinite(v) for v in log.values())
    g = dict(np.load(os.path.join(GOLDEN, 'srgan_step.npz')))
    for k in log:                                   # the same forward, the same netD: the remaining terms are the fixture's
        ref = float(g['vanilla.log_' + k])
        assert abs(log[k] - ref) <= 2e-4 * max(1.0, abs(ref)), k
    moved = 0
    for k, v in netG.named_parameters():
        assert torch.isfinite(v).all(), k
        moved += int(not torch.equal(v.detach().cpu(), sdG[k]))
    assert moved == len(sdG)
    for k, v in netD.state_dict().items():
        assert torch.isfinite(v).all(), k


# ---- the REAL RCCL backend on the one GPU a box has: a forced one-rank group (ESR_DP_FORCE=1, dp.forced) ------------
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rccl_one_rank_worker(port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK='0', WORLD_SIZE='1', LOCAL_RANK='0',
                      HSA_ENABLE_IPC_MODE_LEGACY='0', ESR_DP_FORCE='1')
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch.distributed as dist
    from esrganplus_amd import dp, train, _lib as L
    try:
        out = {}
        dev = torch.device('cuda', 0)

        def run(dp_on):
            netG, netD, netF, _, _ = _nets(dev, 'fp16', 43, 44)
            st = train.SRGANStep(netG, netD, netF, loss_scale=1024.0, data_parallel=dp_on)
            assert st.exG.inline == dp_on and st._manual_ok()
            torch.manual_seed(77)
            lr, hr, _ = _data(dev, 900, 950, None, 'srgan.rccl1')
            log = st.step(lr, hr)
            st.finish()
            torch.cuda.synchronize()
            assert L.lib().esr_rdb_check_abort() == 0, 'a chain gave up next to RCCL work'
            w = {'G.' + k: v.detach().float().cpu() for k, v in netG.state_dict().items()}
            w.update({'D.' + k: v.detach().float().cpu() for k, v in netD.state_dict().items()})
            return w, log, st

        w0, l0, _ = run(False)                     # BEFORE the process group exists: the plain single-GPU step
        assert not dp.active()
        assert dp.init_from_env('nccl') == 1       # one-rank group over RCCL
        assert dist.get_backend() == 'nccl' and dist.get_world_size() == 1 and dp.active() and dp.forced()
        w1, l1, st = run(True)
        rep = st.comm_report()
        out['bytes_per_step'], out['calls_per_step'] = rep['bytes_per_step'], rep['calls_per_step']
        out['expected_bytes'] = 4 * sum(p.numel() for net in (st.netG, st.netD) for p in net.parameters())
        out['weights_equal'] = all(torch.equal(w0[k], w1[k]) for k in w0)
        out['logs'] = (l0, l1)
        out['abort'] = int(L.lib().esr_rdb_check_abort())
        out['librccl_mapped'] = 'librccl' in open('/proc/self/maps').read()
        q.put(('ok', out))
    except Exception as e:   # noqa: BLE001
        import traceback
        q.put((repr(e) + traceback.format_exc(), None))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_forced_one_rank_rccl_step_equals_the_plain_step():
    """One step with ``data_parallel=True`` over the REAL RCCL backend with a forced one-rank group (the mean over one
    rank is the identity): the weights and logs of the plain step, 4 bytes per parameter of G and D exchanged, and no chain
    reports an abort with RCCL work enqueued next to it."""
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    p = ctx.Process(target=_rccl_one_rank_worker, args=(_free_port(), q))
    p.start()
    status, out = q.get(timeout=600)
    p.join(timeout=60)
    assert status == 'ok', status
    print(out)
    assert out['librccl_mapped'], 'RCCL was not loaded: the nccl backend did not run'
    assert out['bytes_per_step'] == out['expected_bytes'] and out['calls_per_step'] >= 2
    assert out['weights_equal'] and out['logs'][0] == out['logs'][1]
    assert tuple(out['logs'][0]) == LOG_KEYS and all(np.isfinite(v) for v in out['logs'][0].values())
    assert out['abort'] == 0


@pytest.mark.parametrize('srgan_first', [False, True])
def test_esrganplus_step_is_left_as_it_was(dev, srgan_first):
    """One default ``ESRGANPlusStep`` step against train_step.npz (the tolerances of
    test_optimize_parameters_step_matches_reference on the seven logs), alone and after an ``SRGANStep`` ran in the same
    process on other networks: the seven values are bit-identical either way — the new step leaves no state behind (loss
    scratch, cached streams, module-level buffers)."""
    from esrganplus_amd import train
    if srgan_first:
        netG, netD, netF, _, _ = _nets(dev, 'fp32', 45, 46)
        lr, hr, z = _data(dev, 31, 31, 10, 'step')
        train.SRGANStep(netG, netD, netF, gan_type='lsgan').step(lr, hr, z=z)
    g = dict(np.load(os.path.join(GOLDEN, 'train_step.npz')))
    netG, netD, netF, _, _ = _nets(dev, 'fp32')
    lr, hr, z = _data(dev, 30, 30, 9, 'step')
    log = train.ESRGANPlusStep(netG, netD, netF).step(lr, hr, z=z)
    for k in LOG_KEYS:
        ref = float(g['log_' + k])
        assert abs(log[k] - ref) <= 2e-4 * max(1.0, abs(ref)), k
    vals = tuple(log[k] for k in LOG_KEYS)
    seen = test_esrganplus_step_is_left_as_it_was.__dict__.setdefault('seen', vals)
    assert vals == seen, (vals, seen)
