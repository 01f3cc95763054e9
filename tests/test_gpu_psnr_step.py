"""train.PSNRStep — the PSNR-oriented pretraining step — against the reference's real ``SRModel`` (codes/models/
SR_model.py; tests/golden/psnr_steps3.npz, tools/gen_psnr_step_golden.py), and its own contracts: the pipelined form,
mixed LR shapes, ``test()``, checkpoints, a frozen parameter, a forced one-rank RCCL exchange.  nb = 2 throughout."""
import os
import socket
import sys
import warnings

import numpy as np
import pytest
import torch

from esrganplus_amd import synth
from tests.conftest import checks

pytestmark = pytest.mark.gpu

CASES = {'l1_wd0': ('l1', 0.0), 'l2_wd0': ('l2', 0.0), 'l2_wd1e-2': ('l2', 1e-2)}
FULL_GRADS = ('model.0.weight', 'model.1.sub.1.RDB2.conv3.0.bias')
FULL_DELTAS = FULL_GRADS + ('model.1.sub.0.RDB1.conv1.0.weight',)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _netG(dev, prec, seed=32):
    from esrganplus_amd import architecture as arch
    netG = arch.RRDBNet(3, 3, 64, 2).to(dev).train().set_precision(prec)
    netG.load_state_dict(synth.rrdbnet_state_dict(nb=2, seed=seed), strict=True)
    return netG


def _golden_batch(g, it, dev):
    """The fixture's data of iteration `it` (1..3), rebuilt from its recorded seeds, names and shapes."""
    from oracle import ref_torch as RT
    (s_lr, s_hr, s_z), (n_lr, n_hr, n_z) = [int(v) for v in g['seeds']], [str(v) for v in g['names']]
    lr = synth.image_batch(s_lr + it, *[int(v) for v in g['lr_shape']], name=n_lr).to(dev)
    hr = synth.image_batch(s_hr + it, *[int(v) for v in g['hr_shape']], name=n_hr).to(dev)
    z = [synth.normal_like(s_z + it, '%s.%d' % (n_z, i), s).to(dev) for i, s in enumerate(RT.noise_shapes(lr.shape, 2, 'codes'))]
    return lr, hr, z


@pytest.mark.parametrize('form', ['production', 'pipelined', 'autograd'])
@pytest.mark.parametrize('case', list(CASES))
def test_three_iterations_match_the_reference(golden, dev, monkeypatch, case, form):
    """Three iterations of the reference's loop body (codes/train.py:97-106: MultiStepLR([1, 2]) stepped BEFORE the
    optimizer, fresh data and noise per iteration) on the imported SRModel, fp32, loss scale 1, with the tolerances of
    test_three_training_iterations_match_the_reference: learning rates rtol 1e-12; l_pix within 5e-4 max(1, |ref|);
    checks(fake_H) within 2e-3 of the fixture's maximum; after iteration 1 (not in the pipelined run) every parameter's
    gradient within 1e-2 of that tensor's maximum; after iteration 3 the parameters' checks within 2e-3 and the stored
    deltas within mean|d - ref| / mean|ref| <= 0.08.  Adam hides the criterion in the weights: the losses and the
    gradients are what tell l2 from l1, the deltas what tells weight decay 1e-2 from 0."""
    from esrganplus_amd import train
    if form == 'autograd':
        monkeypatch.setenv('ESR_TRAIN_MANUAL', '0')
    g = golden('psnr_steps3')
    crit, wd = CASES[case]
    assert str(g['criteria'][list(g['cases']).index(case)]) == crit
    sd = synth.rrdbnet_state_dict(nb=2, seed=int(g['sd_seed']))
    netG = _netG(dev, 'fp32', int(g['sd_seed']))
    st = train.PSNRStep(netG, lr_G=float(g['lr_G']), weight_decay_G=wd, pixel_criterion=crit)
    assert st._manual_ok() == (form != 'autograd')
    sched = torch.optim.lr_scheduler.MultiStepLR(st.optimizer_G, [int(v) for v in g['lr_steps']], float(g['lr_gamma']))
    pg = dict(netG.named_parameters())
    logs = []
    for it in range(1, 4):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            sched.step()                                 # the reference's order: scheduler first (train.py:102)
        assert np.allclose(st.optimizer_G.param_groups[0]['lr'], g['%s.lr_%d' % (case, it)], rtol=1e-12), it
        lr, hr, z = _golden_batch(g, it, dev)
        logs.append(st.step(lr, hr, z=z, sync_log=form != 'pipelined')['l_pix'])
        assert st.log['l_pix'] is logs[-1] and isinstance(logs[-1], torch.Tensor if form == 'pipelined' else float)
        ref = g['%s.fake_H_chk_%d' % (case, it)]
        assert np.abs(checks(st.fake_H.detach()) - ref).max() <= 2e-3 * np.abs(ref).max(), it
        if it == 1 and form != 'pipelined':
            for row, k in zip(g[case + '.grad_chk'], sd.keys()):
                assert np.abs(checks(pg[k].grad) - row).max() <= 1e-2 * np.abs(row).max(), k
            for k in FULL_GRADS:
                ref = g['%s.grad_%s' % (case, k)]
                err = np.abs(pg[k].grad.cpu().numpy() - ref).max() / np.abs(ref).max()
                print('%s %s gradient of %-40s max|g - ref| / max|ref| = %.3e' % (case, form, k, err))
                assert err <= 1e-2, (k, err)
    st.finish()
    for it in range(1, 4):
        got, ref = float(logs[it - 1]), float(g['%s.l_pix_%d' % (case, it)])
        print('%s %s iteration %d  l_pix hip %.6f  ref %.6f' % (case, form, it, got, ref))
        assert abs(got - ref) <= 5e-4 * max(1.0, abs(ref)), (it, got, ref)
    chk = np.stack([checks(pg[k]) for k in sd.keys()])
    assert np.abs(chk - g[case + '.G_chk']).max() <= 2e-3 * np.abs(g[case + '.G_chk']).max()
    for k in FULL_DELTAS:
        d = (pg[k].detach().cpu() - sd[k]).numpy()
        ref = g['%s.delta_%s' % (case, k)]
        err = np.abs(d - ref).mean() / np.abs(ref).mean()
        print('%s %s delta of %-40s mean|d - ref| / mean|ref| = %.3e' % (case, form, k, err))
        assert err <= 0.08, (k, err)


@pytest.mark.parametrize('scale', [1024.0, 'dynamic'])
@pytest.mark.parametrize('case', ['l1_wd0', 'l2_wd0'])
def test_first_step_fp16_loss_scaled(golden, dev, case, scale):
    """Iteration 1 of the fixture in fp16 storage with loss scaling (static 1024 and the dynamic scaler), with the bounds
    of test_optimize_parameters_step_fp16_loss_scaled: l_pix within 2e-2 relative of the reference's fp32 value, the
    first Adam update of model.0.weight agrees in sign with the reference's on >= 95 %, everything finite, the dynamic
    scaler's state afterwards [1024, 0, 1]."""
    from esrganplus_amd import train
    g = golden('psnr_steps3')
    sd = synth.rrdbnet_state_dict(nb=2, seed=int(g['sd_seed']))
    netG = _netG(dev, 'fp16', int(g['sd_seed']))
    st = train.PSNRStep(netG, lr_G=float(g['lr_G']), pixel_criterion=CASES[case][0], loss_scale=scale)
    assert st._manual_ok()
    lr, hr, z = _golden_batch(g, 1, dev)
    got, ref = st.step(lr, hr, z=z)['l_pix'], float(g[case + '.l_pix_1'])
    print('%s scale %s  l_pix hip fp16 %.6f  ref %.6f' % (case, scale, got, ref))
    assert np.isfinite(got) and abs(got - ref) <= 2e-2 * max(1e-3, abs(ref))
    pg = dict(netG.named_parameters())
    for k, v in pg.items():
        assert torch.isfinite(v).all(), k
    d = (pg['model.0.weight'].detach().cpu() - sd['model.0.weight']).numpy()
    agree = np.mean(np.sign(d) == np.sign(g[case + '.delta1_model.0.weight']))
    print('sign agreement of the first Adam update (fp16, %s, scale %s): %.4f' % (case, scale, agree))
    assert agree >= 0.95
    if scale == 'dynamic':
        assert [float(v) for v in st.scaler.state[:3]] == [1024.0, 0.0, 1.0]


MIXED = ((2, 3, 32, 32), (1, 3, 48, 40), (2, 3, 32, 32))


def _mixed_batch(it, shape, dev):
    n, c, h, w = shape
    return (synth.image_batch(600 + it, n, c, h, w, name='psnr.mixed.lr').to(dev),
            synth.image_batch(700 + it, n, c, 4 * h, 4 * w, name='psnr.mixed.hr').to(dev))


def _weights(netG):
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in netG.state_dict().items()}


@pytest.mark.parametrize('crit', ['l1', 'l2'])
def test_mixed_shapes_equal_the_loop_of_public_pieces(dev, crit):
    """Steps on LR batches of alternating shape (the mixed 128 / 192 / 256 buckets of generator training, in small) in
    fp16 with loss scale 1024: the weights equal, bit for bit, those of the generator loop written out from the public
    pieces (bench.py's measure_gtrain / tests/test_gpu_dp.py's run_gtrain), and the step keeps ONE gradient buffer per
    shape."""
    from esrganplus_amd import train, functional as Fn, losses as LS
    from esrganplus_amd.optim import FusedAdam

    netG = _netG(dev, 'fp16', 43)
    st = train.PSNRStep(netG, pixel_criterion=crit, loss_scale=1024.0)
    ptrs = []
    for it, shape in enumerate(MIXED):
        torch.manual_seed(5000 + it)                    # the Philox seeds of the noise layers come from torch's generator
        st.step(*_mixed_batch(it, shape, dev), sync_log=False)
        ptrs.append(st._gys[((shape[0], 3, 4 * shape[2], 4 * shape[3]), dev)].data_ptr())
    st.finish()
    got = _weights(netG)
    assert len(st._gys) == 2 and ptrs[0] == ptrs[2] != ptrs[1]

    netG = _netG(dev, 'fp16', 43)
    opt = FusedAdam(netG.parameters(), lr=2e-4, betas=(0.9, 0.999))
    raw = {'l1': LS.l1_raw, 'l2': LS.l2_raw}[crit]
    for it, shape in enumerate(MIXED):
        torch.manual_seed(5000 + it)
        lr, hr = _mixed_batch(it, shape, dev)
        if not netG.mark_grads_stale():
            opt.zero_grad(set_to_none=True)
        with torch.no_grad():
            fake, stG = Fn.rrdbnet_train_forward(netG, lr)
            gy = torch.empty_like(fake)
            raw(fake, hr, 1.0, grad_out=gy, grad_scale=1024.0)
            Fn.rrdbnet_train_backward(netG, stG, gy)
        opt.step(grad_scale=1.0 / 1024.0)
    want = _weights(netG)
    bad = [k for k in want if not torch.equal(want[k], got[k])]
    assert not bad, bad[:8]
    assert any(not torch.equal(v, synth.rrdbnet_state_dict(nb=2, seed=43)[k].to(dev)) for k, v in want.items())


def test_pipelined_steps_and_test_between_them(dev):
    """step(sync_log=False) three times + finish() leaves the weights and losses of three synchronised steps, bit for
    bit; ``test()`` (SR_model.py:76-80) between pipelined steps returns the eval forward of the weights after exactly
    that many steps, leaves the generator in training mode, and does not change the trajectory."""
    from esrganplus_amd import architecture as arch, train
    val_lr = synth.image_batch(990, 1, 3, 40, 24, name='psnr.val.lr').to(dev)

    def run(pipelined, validate_at=()):
        netG = _netG(dev, 'fp16', 85)
        st = train.PSNRStep(netG, pixel_criterion='l2', loss_scale=1024.0)
        logs, seen = [], {}
        for it in range(3):
            torch.manual_seed(7000 + it)
            lr = synth.image_batch(970 + it, 2, 3, 24, 32, name='psnr.pipe.lr').to(dev)
            hr = synth.image_batch(980 + it, 2, 3, 96, 128, name='psnr.pipe.hr').to(dev)
            logs.append(st.step(lr, hr, sync_log=not pipelined)['l_pix'])
            if it + 1 in validate_at:
                y = st.test(val_lr)
                assert netG.training and y is st.fake_H and not y.requires_grad
                seen[it + 1] = (y.clone(), {k: v.detach().clone() for k, v in netG.state_dict().items()})
        st.finish()
        return _weights(netG), [float(v) for v in logs], seen

    w_sync, l_sync, _ = run(False)
    w_pipe, l_pipe, _ = run(True)
    w_val, l_val, seen = run(True, (1, 2))
    assert l_sync == l_pipe == l_val and all(np.isfinite(l_sync))
    for other in (w_pipe, w_val):
        bad = [k for k in w_sync if not torch.equal(w_sync[k], other[k])]
        assert not bad, bad[:8]
    assert sorted(seen) == [1, 2]
    for n, (y, sd) in seen.items():
        ref = arch.RRDBNet(3, 3, 64, 2).to(dev).eval().set_precision('fp16')
        ref.load_state_dict(sd, strict=True)
        with torch.no_grad():
            assert torch.equal(ref(val_lr), y), n
    assert not torch.equal(seen[1][0], seen[2][0])


@pytest.mark.parametrize('prec,scale', [('fp32', 1.0), ('fp16', 1024.0)])
def test_resumed_pretraining_continues_bit_for_bit(dev, tmp_path, prec, scale):
    """checkpoint.save_step / resume_step on a step without a discriminator: 2 steps, save ({iter}_G.pth and
    {iter}.state, nothing else), a FRESH generator, optimizer and scheduler, resume, 2 more steps — against 4
    uninterrupted steps: every weight and Adam moment bit-identical.  The .state file's one optimizer entry loads into
    torch.optim.Adam (the reference's resume path, base_model.py:76-85)."""
    from esrganplus_amd import architecture as arch, train, checkpoint as ck

    def make(load):
        netG = arch.RRDBNet(3, 3, 64, 2).to(dev).train().set_precision(prec)
        if load:
            netG.load_state_dict(synth.rrdbnet_state_dict(nb=2, seed=81), strict=True)
        st = train.PSNRStep(netG, pixel_criterion='l2', weight_decay_G=1e-3, loss_scale=scale)
        return netG, st, [torch.optim.lr_scheduler.MultiStepLR(st.optimizer_G, [1, 3], 0.5)]

    def steps(st, scheds, lo, hi):
        for it in range(lo, hi):
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                scheds[0].step()
            torch.manual_seed(9000 + it)
            lr = synth.image_batch(900 + it, 2, 3, 24, 24, name='psnr.resume.lr').to(dev)
            hr = synth.image_batch(950 + it, 2, 3, 96, 96, name='psnr.resume.hr').to(dev)
            st.step(lr, hr, sync_log=False)

    def snapshot(netG, st):
        out = {'G.' + k: v for k, v in _weights(netG).items()}
        sd = st.state_dict()['optimizers']
        assert len(sd) == 1
        for i, e in sd[0]['state'].items():
            out['o.%s.m' % i], out['o.%s.v' % i], out['o.%s.t' % i] = e['exp_avg'], e['exp_avg_sq'], e['step']
        out['lr'] = torch.tensor(st.optimizer_G.param_groups[0]['lr'])
        return out

    netG, st, scheds = make(True)
    steps(st, scheds, 0, 4)
    want = snapshot(netG, st)

    netG, st, scheds = make(True)
    steps(st, scheds, 0, 2)
    paths = ck.save_step(st, str(tmp_path), epoch=0, iter_step=2, schedulers=scheds)      # no finish() by the caller
    assert [os.path.basename(p) for p in paths] == ['2_G.pth', '2.state']
    assert sorted(os.listdir(str(tmp_path))) == ['2.state', '2_G.pth']
    state = torch.load(paths[1], map_location='cpu')
    assert set(state) == {'epoch', 'iter', 'schedulers', 'optimizers'} and len(state['optimizers']) == 1
    plain = torch.optim.Adam([torch.nn.Parameter(p.detach().cpu().clone()) for p in netG.parameters()], lr=1.0)
    plain.load_state_dict(state['optimizers'][0])
    assert plain.param_groups[0]['lr'] == st.optimizer_G.param_groups[0]['lr'] and plain.param_groups[0]['weight_decay'] == 1e-3
    assert len(plain.state) == len(list(netG.parameters()))
    del netG, st, scheds
    netG, st, scheds = make(False)                          # a default-initialised generator: everything comes from the files
    assert ck.resume_step(st, str(tmp_path), 2, schedulers=scheds) == (0, 2)
    steps(st, scheds, 2, 4)
    got = snapshot(netG, st)
    assert want.keys() == got.keys()
    bad = [k for k in want if not torch.equal(want[k].cpu(), got[k].cpu())]
    assert not bad, bad[:8]


def test_frozen_parameter_is_left_alone(golden, dev):
    """"can optimize for a part of the model" (SR_model.py:40-44): with model.0.weight frozen the step takes the autograd
    form; that tensor is bit-identical afterwards and has no gradient, every other parameter moved, and the loss is the
    fixture's iteration 1 (the forward does not depend on what trains)."""
    from esrganplus_amd import train
    g = golden('psnr_steps3')
    netG = _netG(dev, 'fp32', int(g['sd_seed']))
    pg = dict(netG.named_parameters())
    pg['model.0.weight'].requires_grad = False
    before = {k: v.detach().clone() for k, v in pg.items()}
    st = train.PSNRStep(netG, lr_G=float(g['lr_G']), pixel_criterion='l2')
    assert not st._manual_ok() and len(st.optimizer_G.param_groups[0]['params']) == len(pg) - 1
    lr, hr, z = _golden_batch(g, 1, dev)
    got, ref = st.step(lr, hr, z=z)['l_pix'], float(g['l2_wd0.l_pix_1'])
    assert abs(got - ref) <= 5e-4 * max(1.0, abs(ref)), (got, ref)
    torch.cuda.synchronize()
    assert torch.equal(pg['model.0.weight'], before['model.0.weight']) and pg['model.0.weight'].grad is None
    still = [k for k, v in pg.items() if k != 'model.0.weight' and torch.equal(v, before[k])]
    assert not still, still[:8]
    ref = g['l2_wd0.grad_model.1.sub.1.RDB2.conv3.0.bias']
    got = pg['model.1.sub.1.RDB2.conv3.0.bias'].grad.cpu().numpy()
    assert np.abs(got - ref).max() <= 1e-2 * np.abs(ref).max()


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
            netG = _netG(dev, 'fp16', 43)
            st = train.PSNRStep(netG, pixel_criterion='l2', loss_scale=1024.0, data_parallel=dp_on)
            assert st.exG.inline == dp_on and st._manual_ok()
            logs = []
            for it in range(2):
                torch.manual_seed(77 + it)
                lr = synth.image_batch(900 + it, 2, 3, 32, 32, name='psnr.rccl1.lr').to(dev)
                hr = synth.image_batch(950 + it, 2, 3, 128, 128, name='psnr.rccl1.hr').to(dev)
                logs.append(st.step(lr, hr)['l_pix'])
            st.finish()
            torch.cuda.synchronize()
            assert L.lib().esr_rdb_check_abort() == 0, 'a chain gave up next to RCCL work'
            return {k: v.detach().float().cpu() for k, v in netG.state_dict().items()}, logs, st

        w0, l0, _ = run(False)                     # BEFORE the process group exists: the plain single-GPU step
        assert not dp.active()
        assert dp.init_from_env('nccl') == 1       # one-rank group over RCCL
        assert dist.get_backend() == 'nccl' and dist.get_world_size() == 1 and dp.active() and dp.forced()
        w1, l1, st = run(True)
        rep = st.comm_report()
        out['bytes_per_step'], out['calls_per_step'] = rep['bytes_per_step'], rep['calls_per_step']
        out['expected_bytes'] = 4 * sum(p.numel() for p in st.netG.parameters())
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


def test_forced_one_rank_rccl_steps_equal_the_plain_steps():
    """Two l2 steps with ``data_parallel=True`` over the REAL RCCL backend with a forced one-rank group (the mean over one
    rank is the identity): the weights and l_pix of the plain step, 4 bytes per parameter exchanged per step, and no chain
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
    assert out['bytes_per_step'] == out['expected_bytes'] and out['calls_per_step'] >= 1
    assert out['weights_equal'] and out['logs'][0] == out['logs'][1] and all(np.isfinite(out['logs'][0]))
    assert out['abort'] == 0
