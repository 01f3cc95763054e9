"""Data-parallel backward on the GPU: the segmented RRDBNet backward that feeds dp.GradExchange slice by
slice (one GPU: against the one-piece backward, with a recording stand-in for the all-reduce), and the real
exchange over RCCL on two GPUs (skipped on boxes with fewer)."""
import os
import socket
import sys

import numpy as np
import pytest
import torch

from esrganplus_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


class _Recorder:
    """Stands in for dp.GradExchange inside the backward node: notes the slices it is handed."""

    def __init__(self, bucket_elems):
        self.bucket_elems = bucket_elems
        self.spans = []

    def __call__(self, t):
        self.spans.append((t.storage_offset(), t.numel()))
        return None


@pytest.mark.parametrize('precision', ['fp32', 'fp16'])
@pytest.mark.parametrize('bucket_elems', [1, 1 << 30])
def test_segmented_backward_equals_one_piece(dev, precision, bucket_elems):
    from esrganplus_amd import architecture as arch
    nb = 3
    sd = synth.rrdbnet_state_dict(nb=nb, seed=5)
    x = synth.image_batch(5, 2, 3, 16, 24, name='seg.x').to(dev)
    gy = synth.normal_like(5, 'seg.gy', (2, 3, 64, 96)).to(dev)
    grads = {}
    for seg in (False, True):
        net = arch.RRDBNet(3, 3, 64, nb).to(dev).eval().set_precision(precision)
        net.load_state_dict(sd)
        rec = _Recorder(bucket_elems)
        if seg:
            net.attach_grad_sync(rec)
        (net(x) * gy).sum().backward()
        grads[seg] = {k: p.grad.clone() for k, p in net.named_parameters()}
        if seg:
            total = sum(p.numel() for p in net.parameters())
            spans = sorted(rec.spans)
            assert spans[0][0] == 0 and sum(n for _, n in spans) == total      # slices tile the flat buffer
            assert all(a + n == b for (a, n), (b, _) in zip(spans, spans[1:]))
            # tail, RRDB 2, 1, 0, first conv — merged into one when the bucket is larger than the net
            assert len(spans) == (nb + 2 if bucket_elems == 1 else 1)
    for k in grads[False]:
        a, b = grads[False][k], grads[True][k]
        # fp32 atomics: run-to-run rounding only
        assert (a - b).norm().item() <= 1e-5 * a.norm().clamp_min(1e-6).item(), k


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _nccl_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), HSA_ENABLE_IPC_MODE_LEGACY='0')
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch.distributed as dist
    from esrganplus_amd import architecture as arch, dp
    try:
        assert dp.init_from_env('nccl') == world
        dev = torch.device('cuda', rank)
        sd = synth.rrdbnet_state_dict(nb=2, seed=9)
        x = synth.image_batch(9 + rank, 2, 3, 16, 16, name='dp.x').to(dev)      # every rank its own minibatch shard
        gy = synth.normal_like(9 + rank, 'dp.gy', (2, 3, 64, 64)).to(dev)

        def grads_of(attach):
            net = arch.RRDBNet(3, 3, 64, 2).to(dev).eval().set_precision('fp32')
            net.load_state_dict(sd)
            ex = dp.GradExchange(net, bucket_bytes=1 << 20, overlap=attach)
            assert ex.inline == attach
            (net(x) * gy).sum().backward()
            if attach:
                ex.start(); ex.wait()                       # no-ops: the gradients arrive averaged
            return torch.cat([p.grad.reshape(-1) for p in net.parameters()]), ex
        local, ex0 = grads_of(False)
        want = local.clone()
        dist.all_reduce(want)
        want /= world
        got, _ = grads_of(True)                             # in-backward exchange over RCCL
        assert (got - want).norm().item() <= 1e-5 * want.norm().item(), 'in-backward exchange'
        ex0.start(); ex0.wait()                             # after-backward exchange of the same gradients
        q.put((rank, 'ok'))
    except Exception as e:   # noqa: BLE001
        q.put((rank, repr(e)))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_in_backward_exchange_two_ranks_rccl():
    if torch.cuda.device_count() < 2:
        pytest.skip('needs 2 GPUs (RCCL)')
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_nccl_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=600) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert sorted(res) == [(0, 'ok'), (1, 'ok')], res


# ---- the full ESRGAN+ step, data-parallel: 2 ranks sharing cuda:0 over gloo --------------------------------------
def _make_nets(dev, precision='fp32'):
    from esrganplus_amd import architecture as arch
    netG = arch.RRDBNet(3, 3, 64, 1).to(dev).train().set_precision(precision)
    netD = arch.Discriminator_VGG_128(3, 64).to(dev).train().set_precision(precision)
    netF = arch.VGGFeatureExtractor(34, False, True, dev).to(dev).eval().set_precision(precision)
    netG.load_state_dict(synth.rrdbnet_state_dict(nb=1, seed=40), strict=True)
    netD.load_state_dict(synth.discriminator_state_dict(seed=41), strict=True)
    netF.load_state_dict(synth.vgg19_state_dict(6, 34), strict=False)
    return netG, netD, netF


def _shard(rank, dev):
    lr = synth.image_batch(50 + rank, 2, 3, 32, 32, name='dpstep.lr').to(dev)
    hr = synth.image_batch(60 + rank, 2, 3, 128, 128, name='dpstep.hr').to(dev)
    return lr, hr


def _noise_z(rank, dev):
    from oracle import ref_torch as RT
    return [synth.normal_like(70 + rank, 'dpstep.z.%d' % i, s).to(dev)
            for i, s in enumerate(RT.noise_shapes((2, 3, 32, 32), 1, 'codes'))]


def _step_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK='0', HSA_ENABLE_IPC_MODE_LEGACY='0')
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch.distributed as dist
    from esrganplus_amd import dp, train
    try:
        torch.cuda.set_device(0)
        dist.init_process_group('gloo', rank=rank, world_size=world)
        dev = torch.device('cuda', 0)
        netG, netD, netF = _make_nets(dev)
        st = train.ESRGANPlusStep(netG, netD, netF)
        assert st.exG.inline and dp.world_size() == world
        st.optimizer_G.step = lambda **kw: None            # keep the (averaged) gradients: they are what is compared
        st.optimizer_D.step = lambda **kw: None
        lr, hr = _shard(rank, dev)
        log = st.step(lr, hr, z=_noise_z(rank, dev))
        torch.cuda.synchronize()
        gG = torch.cat([p.grad.reshape(-1) for p in netG.parameters()]).cpu()
        gD = torch.cat([p.grad.reshape(-1) for p in netD.parameters()]).cpu()
        q.put((rank, 'ok', gG.numpy(), gD.numpy(), {k: float(v) for k, v in log.items()}))
    except Exception as e:   # noqa: BLE001
        import traceback
        q.put((rank, repr(e) + traceback.format_exc(), None, None, None))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.parametrize('world', [2, 8])
def test_train_step_two_ranks_equals_global_batch_loss(dev, world):
    """train.ESRGANPlusStep under torch.distributed (2 — and 8, the node's shape: BASELINE configs[3] — ranks on cuda:0,
    gloo): the gradients that reach the
    optimizers are the rank-average of a loss whose relativistic means run over the GLOBAL batch
    (SRRaGAN_model.py:136-137,151-152) with per-rank BatchNorm statistics — restated here in one
    process with torch formulas over the shards.  Exercises the fused global-mean RaGAN loss, the in-backward
    G exchange, the D exchange and both stream overlaps."""
    import torch.multiprocessing as mp
    import torch.nn.functional as F
    ctx = mp.get_context('spawn')
    # `world` processes on one GPU over a loopback rendezvous: a rank that dies of the INFRASTRUCTURE (rendezvous, a
    # context that does not come up next to seven others — seen once in ~20 runs on a fresh box) gets one more
    # attempt; what the ranks computed is never retried
    for attempt in range(2):
        q = ctx.Queue()
        port = _free_port()
        procs = [ctx.Process(target=_step_worker, args=(r, world, port, q)) for r in range(world)]
        for p in procs:
            p.start()
        res = sorted((q.get(timeout=900) for _ in procs), key=lambda r: r[0])
        for p in procs:
            p.join(timeout=60)
        if all(r[1] == 'ok' for r in res) or attempt == 1:
            break
        print('attempt 1 failed on the worker side, retrying once:', [r[1][:300] for r in res if r[1] != 'ok'])
    assert all(r[1] == 'ok' for r in res), [r[1] for r in res]
    # all ranks hold the same averaged gradients
    for r in range(1, world):
        assert np.abs(res[0][2] - res[r][2]).max() <= 1e-6 * np.abs(res[0][2]).max()
        assert np.abs(res[0][3] - res[r][3]).max() <= 1e-6 * np.abs(res[0][3]).max()

    # ---- single-process restatement
    netG, netD, netF = _make_nets(dev)
    shards = [_shard(r, dev) for r in range(world)]
    bce = lambda v, real: F.binary_cross_entropy_with_logits(v, torch.ones_like(v) if real else torch.zeros_like(v))
    for p in netD.parameters():
        p.requires_grad = False
    fakes, pix, fea, pg, pr = [], [], [], [], []
    for r, (lr, hr) in enumerate(shards):
        fake = netG(lr, z=_noise_z(r, dev))
        fakes.append(fake)
        pix.append(1e-2 * F.l1_loss(fake, hr))
        ff, rf = netF.forward_pair(fake, hr)
        fea.append(F.l1_loss(ff, rf.detach()))
        a, b = netD.forward_pair(fake, hr)
        pg.append(a); pr.append(b.detach())
    m_fake, m_real = torch.cat(pg).mean(), torch.cat(pr).mean()
    tot = 0
    for r in range(world):
        gan = 5e-3 * (bce(pr[r] - m_fake, False) + bce(pg[r] - m_real, True)) / 2
        tot = tot + (pix[r] + fea[r] + gan) / world
    tot.backward()
    wantG = torch.cat([p.grad.reshape(-1) for p in netG.parameters()]).cpu().numpy()
    for p in netD.parameters():
        p.requires_grad = True
    netD.zero_grad(set_to_none=True)
    dr, df = [], []
    for r, (lr, hr) in enumerate(shards):
        a, b = netD.forward_pair(hr, fakes[r].detach())
        dr.append(a); df.append(b)
    m_real, m_fake = torch.cat(dr).mean(), torch.cat(df).mean()
    totd = 0
    for r in range(world):
        totd = totd + (bce(dr[r] - m_fake, True) + bce(df[r] - m_real, False)) / 2 / world
    totd.backward()
    wantD = torch.cat([p.grad.reshape(-1) for p in netD.parameters()]).cpu().numpy()
    eG = np.linalg.norm(res[0][2] - wantG) / np.linalg.norm(wantG)
    eD = np.linalg.norm(res[0][3] - wantD) / np.linalg.norm(wantD)
    print('relative gradient error  G %.3e  D %.3e' % (eG, eD))
    assert eG <= 2e-4 and eD <= 2e-4


@pytest.mark.parametrize('N', [2, 8])
def test_bench_two_ranks_prints_the_dp_train_object(N):
    """`bench.py --gpus N` (2, and 8: the node BASELINE configs[3] / configs[4] name) as the driver launches it for the
    scaling runs, here with all ranks on cuda:0 and gloo in
    place of RCCL (ESR_BENCH_BACKEND): at world > 1 the --full line must carry a `dp_train` object — the configs[3]
    step over the process group with its all-reduce volume, the exposed communication time and the same process's
    no-exchange step time — so that the multi-GPU run exercises the collective path, not only independent forwards."""
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ESR_BENCH_BACKEND='gloo', MASTER_PORT=str(_free_port()), HSA_ENABLE_IPC_MODE_LEGACY='0')
    out = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', str(N), '--steps', '2', '--warmup', '1',
                          '--batch', '2', '--lr', '32', '--train-batch', '2', '--dp-steps', '2', '--full', '--no-cpu-baseline',
                          '--gtrain-buckets', '2x32,1x48,1x64'],
                         cwd=root, env=env, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         timeout=1500).stdout.decode()
    lines = [l for l in out.strip().splitlines() if l.startswith('{')]
    assert len(lines) == 1, out
    d = json.loads(lines[0])
    assert d['n_gpus'] == N and 'dp_train' in d and 'train_step' not in d
    o = d['dp_train']
    assert o['n_ranks'] == N and o['backend'] == 'gloo' and o['scaling'] == 'weak'
    # G 16 839 299 + D 14 502 281 fp32 gradients + the relativistic means' scalars
    assert o['allreduce_bytes_per_step'] == 4 * (16839299 + 14502281) + 40
    assert o['allreduce_calls_per_step'] >= 2
    assert o['ms_per_step'] > 0 and o['ms_per_step_no_exchange'] > 0 and o['exposed_comm_ms_per_step'] >= 0
    assert abs(o['value'] - N * 2 * 128 * 128 / 1e6 / (o['ms_per_step'] / 1e3)) <= 1e-2 * o['value']
    # BASELINE configs[4] at world > 1 (VERDICT r04 #3a): the mixed-tile generator step over the process group — three
    # buckets per step, each all-reducing G's 16 839 299 fp32 gradients inside its backward
    g = d['dp_gtrain']
    assert g['n_ranks'] == N and g['backend'] == 'gloo' and g['scaling'] == 'weak'
    assert g['allreduce_bytes_per_step'] == g['expected_allreduce_bytes_per_step'] == 3 * 4 * 16839299
    assert g['allreduce_calls_per_step'] >= 3 and g['exposed_comm_ms_per_step'] >= 0
    assert set(g['buckets_ms']) == set(g['buckets_ms_no_exchange']) == {'2x32^2', '1x48^2', '1x64^2'}
    assert all(v > 0 for v in g['buckets_ms'].values()) and g['ms_per_step'] > 0 and g['ms_per_step_no_exchange'] > 0
    lr_pix = 2 * 32 * 32 + 48 * 48 + 64 * 64
    assert abs(g['value'] - N * 16 * lr_pix / 1e6 / (g['ms_per_step'] / 1e3)) <= 1e-2 * g['value']


# ---- the REAL RCCL backend on the one GPU a box has: a forced one-rank group (ESR_DP_FORCE=1, dp.forced) -------------
def _rccl_one_rank_worker(port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK='0', WORLD_SIZE='1', LOCAL_RANK='0',
                      HSA_ENABLE_IPC_MODE_LEGACY='0', ESR_DP_FORCE='1')
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import ctypes as C
    import torch.distributed as dist
    from esrganplus_amd import dp, train, _lib as L, functional as Fn, losses as LS
    from esrganplus_amd.optim import FusedAdam
    from esrganplus_amd import architecture as arch
    try:
        out = {}
        dev = torch.device('cuda', 0)

        def run_step(dp_on, steps=3):
            torch.manual_seed(77)
            netG, netD, netF = _make_nets(dev, 'fp16')
            st = train.ESRGANPlusStep(netG, netD, netF, loss_scale=1024.0, data_parallel=dp_on)
            assert st.exG.inline == dp_on
            logs = []
            for it in range(steps):
                lr = synth.image_batch(900 + it, 4, 3, 32, 32, name='rccl1.lr').to(dev)
                hr = synth.image_batch(950 + it, 4, 3, 128, 128, name='rccl1.hr').to(dev)
                logs.append({k: float(v) for k, v in st.step(lr, hr).items()})
            st.finish()
            torch.cuda.synchronize()
            assert L.lib().esr_rdb_check_abort() == 0, 'a chain gave up next to RCCL work'
            g = torch.cat([p.grad.reshape(-1).float() for p in netG.parameters()]).cpu()
            w = {k: v.detach().float().cpu() for k, v in list(netG.state_dict().items()) + [('D.' + k, v) for k, v in netD.state_dict().items()]}
            return g, w, logs, st

        g0, w0, l0, _ = run_step(False)            # BEFORE the process group exists: the plain single-GPU step
        assert not dp.active()
        assert dp.init_from_env('nccl') == 1       # one-rank group over RCCL (device_id= path)
        assert dist.get_backend() == 'nccl' and dist.get_world_size() == 1 and dp.active() and dp.forced()
        g1, w1, l1, st = run_step(True)
        rep = st.comm_report()
        out['calls_per_step'], out['bytes_per_step'] = rep['calls_per_step'], rep['bytes_per_step']
        nG = sum(p.numel() for p in st.netG.parameters())
        nD = sum(p.numel() for p in st.netD.parameters())
        out['expected_bytes'] = 4 * (nG + nD)
        out['grad_equal'] = bool(torch.equal(g0, g1))
        out['weights_equal'] = all(torch.equal(w0[k], w1[k]) for k in w0)
        out['logs_equal'] = l0 == l1
        out['max_grad_diff'] = float((g0 - g1).abs().max())

        # the generator-only bucket loop (bench.py measure_gtrain's form) with the exchange inside each backward
        def run_gtrain(dp_on):
            torch.manual_seed(78)
            netG = arch.RRDBNet(3, 3, 64, 2).to(dev).train().set_precision('fp16')
            netG.load_state_dict(synth.rrdbnet_state_dict(nb=2, seed=43, gain=0.5))
            opt = FusedAdam(netG.parameters(), lr=1e-4, betas=(0.9, 0.999))
            ex = dp.GradExchange(netG, enabled=dp_on, measure=dp_on)
            assert ex.inline == dp_on
            scale = torch.full((), 1024.0, device=dev)
            for it in range(2):
                for k, (n, sz) in enumerate(((2, 32), (1, 48))):
                    lr = synth.image_batch(600 + 10 * it + k, n, 3, sz, sz, name='rccl1.glr').to(dev)
                    hr = synth.image_batch(700 + 10 * it + k, n, 3, 4 * sz, 4 * sz, name='rccl1.ghr').to(dev)
                    if not netG.mark_grads_stale():
                        opt.zero_grad(set_to_none=True)
                    with torch.no_grad():
                        fake, stG = Fn.rrdbnet_train_forward(netG, lr)
                        gy = torch.empty_like(fake)
                        LS.l1_raw(fake, hr, 1.0, grad_out=gy, grad_scale=1024.0)
                        Fn.rrdbnet_train_backward(netG, stG, gy)
                    ex.start(); ex.wait()
                    opt.step(grad_scale=1.0 / 1024.0)
            torch.cuda.synchronize()
            assert L.lib().esr_rdb_check_abort() == 0, 'a chain gave up next to RCCL work'
            return {k: v.detach().float().cpu() for k, v in netG.state_dict().items()}, ex
        wa, _ = run_gtrain(False)
        wb, exg = run_gtrain(True)
        out['gtrain_weights_equal'] = all(torch.equal(wa[k], wb[k]) for k in wa)
        out['gtrain_calls'], out['gtrain_bytes'] = exg.calls, exg.bytes
        out['gtrain_expected_bytes'] = 4 * sum(p.numel() for p in exg.params) * 4        # 2 iterations x 2 buckets
        maps = open('/proc/self/maps').read()
        out['librccl_mapped'] = 'librccl' in maps
        out['rccl_version'] = '.'.join(str(v) for v in torch.cuda.nccl.version())
        q.put(('ok', out))
    except Exception as e:   # noqa: BLE001
        import traceback
        q.put((repr(e) + traceback.format_exc(), None))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_forced_one_rank_rccl_step_equals_the_plain_step():
    """the data-parallel branches of dp.GradExchange (AVG all-reduce of flat-gradient slices inside
    the segmented RRDBNet backward, D's buckets under it, stream-side Work.wait()), of losses' global RaGAN means and of
    train.ESRGANPlusStep over the REAL RCCL backend ('nccl', device_id=) with a forced one-rank group: three train steps
    and the generator-only bucket loop must leave exactly the gradients / weights / losses of the plain step (the mean
    over one rank is the identity), the byte counts are the networks' gradient bytes, librccl is in the process's maps,
    and no chain reports an abort with RCCL work enqueued next to it."""
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    p = ctx.Process(target=_rccl_one_rank_worker, args=(_free_port(), q))
    p.start()
    status, out = q.get(timeout=900)
    p.join(timeout=60)
    assert status == 'ok', status
    print(out)
    assert out['librccl_mapped'], 'RCCL was not loaded: the nccl backend did not run'
    assert out['bytes_per_step'] == out['expected_bytes'] and out['calls_per_step'] >= 2
    assert out['gtrain_bytes'] == out['gtrain_expected_bytes'] and out['gtrain_calls'] >= 4
    assert out['logs_equal'] and out['grad_equal'] and out['weights_equal'], out
    assert out['gtrain_weights_equal']


def test_bench_forced_one_rank_rccl_prints_the_dp_objects():
    """`ESR_DP_FORCE=1 python bench.py --gpus 1 --full`: the dp_train / dp_gtrain objects over a one-rank RCCL group — n_ranks 1,
    backend nccl, the all-reduce volume of BASELINE configs[3] (125 MB) and configs[4] (3 x 67.4 MB) — and the `dist`
    object that proves which backend / RCCL version / world size a line was measured under."""
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ESR_DP_FORCE='1', MASTER_PORT=str(_free_port()), HSA_ENABLE_IPC_MODE_LEGACY='0')
    env.pop('ESR_BENCH_BACKEND', None)
    out = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '2',
                          '--dp-steps', '4', '--full', '--no-cpu-baseline', '--no-fwd-bwd', '--no-mfma-probe'],
                         cwd=root, env=env, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         timeout=1500).stdout.decode()
    line = json.loads([l for l in out.splitlines() if l.startswith('{')][-1])
    d = line['dist']
    assert d['world_size'] == 1 and d['backend'] == 'nccl' and d['forced_one_rank'] and d['rccl_version']
    dpo, dpg = line['dp_train'], line['dp_gtrain']
    assert dpo['n_ranks'] == 1 and dpo['backend'] == 'nccl' and dpg['n_ranks'] == 1
    assert abs(dpo['allreduce_bytes_per_step'] - 125.4e6) < 0.5e6, dpo['allreduce_bytes_per_step']
    assert dpg['allreduce_bytes_per_step'] == dpg['expected_allreduce_bytes_per_step'] == 3 * 4 * 16839299
    assert dpo['allreduce_calls_per_step'] >= 2 and dpg['allreduce_calls_per_step'] >= 3
    # one rank: the exchange is RCCL's bookkeeping only — the DP step may not cost more than a few percent
    print('dp_train %.3f ms (no exchange %.3f), exposed %.3f ms; dp_gtrain %.2f (%.2f)' % (
        dpo['ms_per_step'], dpo['ms_per_step_no_exchange'], dpo['exposed_comm_ms_per_step'],
        dpg['ms_per_step'], dpg['ms_per_step_no_exchange']))
    assert dpo['ms_per_step'] <= 1.25 * dpo['ms_per_step_no_exchange'] + 0.5
