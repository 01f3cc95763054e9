"""GPU parity of the RRDBNet backward (dgrad through the fused conv kernel with transposed weights,
wgrad kernel, LeakyReLU/noise/residual backward in epilogues) against the golden gradients captured
from the imported reference (oracle/gen_golden.py)."""
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


def zs(seed, shapes, tag):
    return [synth.normal_like(seed, '%s.%d' % (tag, i), s) for i, s in enumerate(shapes)]


FULL = ('model.0.weight', 'model.1.sub.0.RDB2.conv2.0.weight', 'model.1.sub.0.RDB3.conv1x1.weight',
        'model.1.sub.0.RDB1.conv5.0.bias', 'model.6.weight', 'model.10.weight', 'model.10.bias')


@pytest.mark.parametrize('tag,nb,shape,variant', [('a', 1, (1, 3, 16, 20), 'codes'),
                                                  ('b', 2, (2, 3, 24, 24), 'codes'),
                                                  ('c', 1, (1, 3, 13, 18), 'test_image')])
@pytest.mark.parametrize('mode', ['eval', 'train'])
def test_rrdbnet_param_grads_fp32(dev, golden, tag, nb, shape, variant, mode):
    from esrganplus_amd import architecture as arch
    from oracle import ref_torch as RT
    g = golden('rrdbnet_small')
    sd = synth.rrdbnet_state_dict(nb=nb, seed=20 + nb)
    cls = arch.RRDBNet if variant == 'codes' else arch.RRDB_Net
    net = cls(3, 3, 64, nb).to(dev)
    net.load_state_dict(sd, strict=True)
    net.train(mode == 'train')
    x = synth.image_batch(3, *shape, name='small.x.' + tag).to(dev).requires_grad_(True)
    gy = synth.normal_like(3, 'small.gy.' + tag, (shape[0], 3, shape[2] * 4, shape[3] * 4)).to(dev)
    z = None
    if mode == 'train':
        z = [t.to(dev) for t in zs(7, RT.noise_shapes(shape, nb, variant), 'small.z.' + tag)]
    y = net(x, z=z)
    assert np.abs(y.detach().cpu().numpy() - g['%s_y_%s' % (tag, mode)]).max() <= 1e-4
    (y * gy).sum().backward()
    # dL/dx of the whole generator (autograd through architecture.py:76-78) against the reference's
    gxr = g['%s_gx_%s' % (tag, mode)]
    assert x.grad is not None and tuple(x.grad.shape) == tuple(x.shape)
    egx = np.abs(x.grad.cpu().numpy() - gxr).max()
    print('dL/dx max|diff| %.3e (|ref| max %.3f)' % (egx, np.abs(gxr).max()))
    assert egx <= 2e-3 * max(1.0, np.abs(gxr).max()), egx
    params = dict(net.named_parameters())
    if mode == 'train':
        for k in FULL:
            ref = g['%s_g_%s' % (tag, k)]
            got = params[k].grad.cpu().numpy()
            err = np.abs(got - ref).max()
            assert err <= 2e-3 * max(1.0, np.abs(ref).max()), (k, err, np.abs(ref).max())
    chk = np.stack([checks(params[k].grad) for k in sd.keys()])
    ref = g['%s_gchk_%s' % (tag, mode)]
    rel = np.abs(chk - ref) / np.maximum(1.0, np.abs(ref[:, 1:2]))
    assert rel.max() <= 2e-3, (np.unravel_index(rel.argmax(), rel.shape), rel.max())


def test_backward_fp16_close_to_fp32(dev):
    """fp16 storage path: gradients track the fp32 path (loss-scaled by the caller in training)."""
    from esrganplus_amd import architecture as arch
    sd = synth.rrdbnet_state_dict(nb=1, seed=3)
    x = synth.image_batch(3, 2, 3, 16, 16, name='bw16.x').to(dev)
    gy = synth.normal_like(3, 'bw16.gy', (2, 3, 64, 64)).to(dev)
    grads = {}
    for prec in ('fp32', 'fp16'):
        net = arch.RRDBNet(3, 3, 64, 1).to(dev).eval().set_precision(prec)
        net.load_state_dict(sd)
        (net(x) * gy).sum().backward()
        grads[prec] = {k: p.grad.clone() for k, p in net.named_parameters()}
    for k in grads['fp32']:
        a, b = grads['fp32'][k], grads['fp16'][k]
        rel = ((a - b).norm() / a.norm().clamp_min(1e-6)).item()   # fp16 storage: ~1e-2 relative
        assert rel <= 6e-2, (k, rel)


def test_two_forwards_before_backward_use_distinct_plans(dev):
    from esrganplus_amd import architecture as arch
    net = arch.RRDBNet(3, 3, 64, 1).to(dev).eval()
    net.load_state_dict(synth.rrdbnet_state_dict(1, 4))
    x1 = synth.image_batch(1, 1, 3, 8, 8, name='p.x1').to(dev)
    x2 = synth.image_batch(2, 1, 3, 8, 8, name='p.x2').to(dev)
    y1, y2 = net(x1), net(x2)
    (y1.sum() + 2 * y2.sum()).backward()
    g12 = {k: p.grad.clone() for k, p in net.named_parameters()}
    net.zero_grad()
    net(x1).sum().backward()
    (2 * net(x2).sum()).backward()
    for k, p in net.named_parameters():
        assert (p.grad - g12[k]).abs().max().item() <= 1e-4 * max(1.0, g12[k].abs().max().item()), k


@pytest.mark.parametrize('mode', ['eval', 'train'])
def test_standalone_rdb_backward_golden(dev, golden, mode):
    """ResidualDenseBlock_5C used on its own (block.py:232-268): input gradient and parameter
    gradients against the reference's (tests/golden/rdb.npz, captured from the imported reference)."""
    from esrganplus_amd import block as B
    g = golden('rdb')
    sd = synth.rrdbnet_state_dict(nb=1, seed=11)
    p = 'model.1.sub.0.RDB1.'
    m = B.ResidualDenseBlock_5C(64).to(dev).set_precision('fp32')
    m.load_state_dict({k[len(p):]: v for k, v in sd.items() if k.startswith(p)})
    m.train(mode == 'train')
    x = synth.normal_like(11, 'rdb.x', (1, 64, 12, 12)).to(dev).requires_grad_(True)
    gy = synth.normal_like(11, 'rdb.gy', (1, 64, 12, 12)).to(dev)
    z = zs(5, [(1, 64, 12, 12)], 'rdb.z')[0].to(dev) if mode == 'train' else None
    y = m(x, z=z) if z is not None else m(x)
    assert np.abs(y.detach().cpu().numpy() - g['y_' + mode]).max() <= 2e-5
    (y * gy).sum().backward()
    gx = x.grad.cpu().numpy()
    ref = g['gx_' + mode]
    assert np.abs(gx - ref).max() <= 2e-4 * max(1.0, np.abs(ref).max())
    if mode == 'train':
        for name, par in (('gw_conv1', m.conv1[0].weight), ('gw_conv3', m.conv3[0].weight),
                          ('gw_conv5', m.conv5[0].weight), ('gb_conv4', m.conv4[0].bias),
                          ('gw_conv1x1', m.conv1x1.weight)):
            got, want = par.grad.cpu().numpy(), g[name]
            assert np.abs(got - want).max() <= 2e-3 * max(1e-3, np.abs(want).max()), name


@pytest.mark.parametrize('variant', ['codes', 'test_image'])
def test_standalone_rrdb_backward_vs_oracle(dev, variant):
    """RRDB on its own (block.py:271-291 / test_image/block.py:236-256), train mode with explicit
    noise: input + parameter gradients against the CPU restatement of the reference."""
    from esrganplus_amd import block as B
    from oracle import ref_torch as RT
    sd = synth.rrdbnet_state_dict(nb=1, seed=31)
    p = 'model.1.sub.0.'
    m = B.RRDB(64, extra_noise=(variant == 'test_image')).to(dev).set_precision('fp32').train()
    m.load_state_dict({k[len(p):]: v for k, v in sd.items() if k.startswith(p)})
    shape = (2, 64, 10, 14)
    x = synth.normal_like(31, 'rrdb.x', shape)
    gy = synth.normal_like(31, 'rrdb.gy', shape)
    nz = 4 if variant == 'test_image' else 3
    z = zs(6, [shape] * nz, 'rrdb.z')
    # oracle
    sdr = {k: v.clone().requires_grad_(True) for k, v in sd.items() if k.startswith(p)}
    xo = x.clone().requires_grad_(True)
    yo = RT.rrdb_forward(xo, sdr, p[:-1], z[:3], z[3] if nz == 4 else None)
    (yo * gy).sum().backward()
    # HIP
    xg = x.to(dev).requires_grad_(True)
    y = m(xg, z=[t.to(dev) for t in z])
    assert (y.detach().cpu() - yo.detach()).abs().max().item() <= 5e-5
    (y * gy.to(dev)).sum().backward()
    ref = xo.grad
    assert (xg.grad.cpu() - ref).abs().max().item() <= 2e-4 * max(1.0, ref.abs().max().item())
    for k in ('RDB1.conv1.0.weight', 'RDB2.conv1x1.weight', 'RDB3.conv5.0.weight', 'RDB2.conv4.0.bias'):
        got = dict(m.named_parameters())[k].grad.cpu()
        want = sdr[p + k].grad
        assert (got - want).abs().max().item() <= 2e-3 * max(1e-3, want.abs().max().item()), k


@pytest.mark.parametrize('prec', ['fp32', 'fp16'])
def test_full_depth_backward_at_bench_shape_vs_reference_golden(dev, golden, prec):
    """nb=23 at the shape bench.py's fwd_bwd times (batch 16 of 128x128 LR: 256-tile chain / 512-tile dgrad
    instantiations, the fused dense-block wgrad over 69 blocks) under tests/golden/rrdbnet_full_grad.npz — the
    imported reference's gradients for ONE tile (oracle/gen_golden.py: gen_rrdbnet_full_grad).  Parameter
    gradients add over the batch: the golden tile sits at batch positions 0 and 9 with upstream gradients gy and
    gy/2, every other tile gets a zero upstream gradient, so each gradient must equal 1.5 x the golden one."""
    from esrganplus_amd import architecture as arch
    g = golden('rrdbnet_full_grad')
    sd = synth.rrdbnet_state_dict(nb=23, seed=0, gain=0.5)
    net = arch.RRDBNet(3, 3, 64, 23).to(dev).eval().set_precision(prec)
    net.load_state_dict(sd, strict=True)
    x = synth.image_batch(42, 16, 3, 128, 128, name='fullgrad.fill')
    x[0] = x[9] = synth.image_batch(41, 1, 3, 128, 128, name='fullgrad.x')[0]
    gy1 = synth.normal_like(41, 'fullgrad.gy', (1, 3, 512, 512))[0] / (3 * 512 * 512)
    S = 1.0 if prec == 'fp32' else 2.0 ** 17               # loss scale: fp16 gradients would underflow otherwise
    gy = torch.zeros(16, 3, 512, 512)
    gy[0], gy[9] = gy1 * S, gy1 * (0.5 * S)
    y = net(x.to(dev))
    ytol = 2e-4 if prec == 'fp32' else 6e-3
    assert np.abs(y[0, :, :8, :8].detach().cpu().numpy() - g['y_head']).max() <= ytol
    assert torch.equal(y[0], y[9])
    (y * gy.to(dev)).sum().backward()
    keys = [str(k) for k in g['keys']]
    assert keys == list(sd.keys())
    params = dict(net.named_parameters())
    errs = []
    worst = {'l2': (0.0, ''), 'proj': (0.0, ''), 'head': (0.0, '')}
    for row, k in zip(g['probe'], keys):
        got = (params[k].grad.double() / (1.5 * S)).reshape(-1)
        assert torch.isfinite(got).all(), k
        l2 = float(row[2])
        e_l2 = abs(got.norm().item() - l2) / max(l2, 1e-30)
        e_pr = 0.0
        for i in range(3):
            r = synth.normal_like(77, 'gproj.%s.%d' % (k, i), tuple(got.shape)).to(dev).double()
            e_pr = max(e_pr, abs((got * r).sum().item() - float(row[3 + i])) / max(l2, 1e-30))
        n = min(32, got.numel())
        head = row[6:6 + n]
        e_hd = np.abs(got[:n].cpu().numpy() - head).max() / max(np.abs(head).max(), l2 / np.sqrt(got.numel()))
        errs.append((e_l2, e_pr, e_hd))
        for name, e in (('l2', e_l2), ('proj', e_pr), ('head', e_hd)):
            if e > worst[name][0]:
                worst[name] = (e, k)
    mean = np.mean(np.array(errs), axis=0)
    print('full-depth backward %s: worst rel errors' % prec, worst, 'mean (l2, proj, head)', mean)
    # What bounds the error at this depth is not the arithmetic but LeakyReLU sign flips: a pre-activation within
    # rounding of zero (fp32: ~1e-7, fp16 storage: ~1e-3 of its scale) takes the other slope, which moves a bias
    # gradient (a 16384-term sum with cancellation) by ~0.8/128 of its size per flipped pixel.  Hence per-tensor
    # bounds with room for a few flips and tight bounds on the means over the 700 tensors; a lost tile / block /
    # tap would show as tens of percent everywhere.
    # fp16: the limits are DERIVED, not picked — tests/golden/rrdbnet_full_grad_fp16emu.npz holds the same metrics for
    # a CPU restatement of "fp16 storage, fp32 accumulate" (oracle/gen_golden.py: rrdbnet_forward_fp16_storage: every
    # tensor the fp16 path keeps in memory rounded to fp16, gradients too, loss scale 2^17) against the imported
    # reference: worst (l2, proj, head) = (0.036, 0.249, 0.181), mean (0.0087, 0.064, 0.045) — fp16 storage alone puts
    # ANY implementation there (LeakyReLU masks of pre-activations within fp16 rounding of zero flip).  The chains must
    # stay within 2x of that emulation's worst case and 1.5x of its means (measured: 0.041 / 0.262 / 0.264, means
    # 0.0064 / 0.067 / 0.048); each full tensor within 2x of the emulation's error on that tensor.
    emu = dict(np.load(os.path.join(GOLDEN, 'rrdbnet_full_grad_fp16emu.npz')))
    if prec == 'fp32':
        lim_w, lim_m = (4e-3, 2.5e-2, 2.5e-2), (8e-4, 4e-3, 3e-3)
    else:
        assert float(emu['loss_scale']) == S
        lim_w, lim_m = tuple(2.0 * emu['worst']), tuple(1.5 * emu['mean'])
        print('fp16 limits from the fp16-storage emulation: worst <= %s, mean <= %s' % (np.round(lim_w, 4), np.round(lim_m, 4)))
    assert worst['l2'][0] <= lim_w[0] and worst['proj'][0] <= lim_w[1] and worst['head'][0] <= lim_w[2], worst
    assert (mean <= np.array(lim_m)).all(), mean
    emu_full = dict(zip([str(k) for k in emu['full_keys']], emu['full_err']))
    for k in [n[2:] for n in g if n.startswith('g_')]:
        want = g['g_' + k]
        got = (params[k].grad / (1.5 * S)).cpu().numpy()
        e = np.abs(got - want).max() / np.abs(want).max()
        lim = 6e-3 if prec == 'fp32' else 2.0 * float(emu_full[k])
        print('  %-40s max|diff| / max|ref| = %.2e  (limit %.2e)' % (k, e, lim))
        assert e <= lim, (k, e, lim)


@pytest.mark.parametrize('prec,tol', [('fp32', 2e-4), ('fp16', 4e-2)])
def test_rrdbnet_input_gradient_only(dev, golden, prec, tol):
    """Frozen generator, gradient w.r.t. the LR image only (e.g. an adversarial / inversion loop around
    architecture.py:76-78): no parameter gradient is produced, dL/dx matches the reference's (fp32) and the fp16
    chains track it."""
    from esrganplus_amd import architecture as arch
    g = golden('rrdbnet_small')
    nb, shape = 2, (2, 3, 24, 24)
    net = arch.RRDBNet(3, 3, 64, nb).to(dev).eval().set_precision(prec)
    net.load_state_dict(synth.rrdbnet_state_dict(nb=nb, seed=20 + nb), strict=True)
    for p in net.parameters():
        p.requires_grad = False
    x = synth.image_batch(3, *shape, name='small.x.b').to(dev).requires_grad_(True)
    gy = synth.normal_like(3, 'small.gy.b', (shape[0], 3, shape[2] * 4, shape[3] * 4)).to(dev)
    (net(x) * gy).sum().backward()
    ref = g['b_gx_eval']
    err = np.abs(x.grad.cpu().numpy() - ref).max() / max(1.0, np.abs(ref).max())
    assert err <= tol, err
    assert all(p.grad is None for p in net.parameters())


def test_data_parallel_replica_hands_gradients_back_to_the_original(dev):
    """networks.py:105-107 wraps the generator in nn.DataParallel: a replica's weights are Broadcast outputs (non-leaf),
    so its backward must return per-tensor gradients that autograd carries back to the ORIGINAL parameters (ADVICE r04:
    the flat-gradient route assigned `.grad` on the copies and the originals got nothing)."""
    from esrganplus_amd import architecture as arch
    nb = 1
    sd = synth.rrdbnet_state_dict(nb=nb, seed=5)
    x = synth.image_batch(4, 2, 3, 16, 24, name='dp.x').to(dev)
    gy = synth.normal_like(4, 'dp.gy', (2, 3, 64, 96)).to(dev)

    def grads(replicated):
        net = arch.RRDBNet(3, 3, 64, nb).to(dev).eval()
        net.load_state_dict(sd, strict=True)
        run = torch.nn.parallel.replicate(net, [0])[0] if replicated else net
        if replicated:
            assert all(not p.is_leaf for p in run._convs()[1])
        (run(x) * gy).sum().backward()
        return {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}
    ref, got = grads(False), grads(True)
    assert len(ref) == len(got) == len(sd)
    for k in ref:
        assert torch.equal(ref[k], got[k]), k


def test_data_parallel_discriminator_replica_hands_gradients_back(dev):
    """The same for networks.py:136-137 (netD under nn.DataParallel): a replica's `parameters()` is empty, its weights
    are non-leaf attributes; the plan must still see that they want gradients and autograd must carry them back."""
    from esrganplus_amd import architecture as arch
    sd = synth.discriminator_state_dict(seed=9)
    x = synth.image_batch(5, 2, 3, 128, 128, name='dpd.x').to(dev)

    def grads(replicated):
        net = arch.Discriminator_VGG_128(3, 64).to(dev).train()
        net.load_state_dict(sd, strict=True)
        run = torch.nn.parallel.replicate(net, [0])[0] if replicated else net
        run(x).sum().backward()
        return {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}
    ref, got = grads(False), grads(True)
    assert len(ref) == len(got) == len(list(arch.Discriminator_VGG_128(3, 64).parameters()))
    for k in ref:
        assert torch.allclose(ref[k], got[k], rtol=1e-5, atol=1e-6), k


@pytest.mark.parametrize('prec', ['fp32', 'fp16'])
def test_data_parallel_two_replicas_on_one_gpu_end_to_end(dev, prec):
    """networks.py:105-107 end to end on a one-GPU box: `nn.DataParallel(net, device_ids=[0, 0])` — scatter, Broadcast
    replicas, two threads driving the two replicas through the library at once, gather, gradients reduced into the
    originals.  Round 5 found two bugs here: replicas took the inference route (no gradients), and the training plan did
    not keep its packed input-gradient operands alive — a replica is gone when its forward returns, so the backward read
    freed memory whenever the allocator had re-used the block (wrong gradients on 76 of 78 tensors in fp32)."""
    from esrganplus_amd import architecture as arch
    nb = 2
    net = arch.RRDBNet(3, 3, 64, nb).to(dev).eval().set_precision(prec)
    net.load_state_dict(synth.rrdbnet_state_dict(nb=nb, seed=3), strict=True)
    x = synth.image_batch(3, 4, 3, 24, 32, name='dpt.x').to(dev)
    gy = synth.normal_like(3, 'dpt.gy', (4, 3, 96, 128)).to(dev)
    ref = net(x)
    (ref * gy).sum().backward()
    g_ref = {k: p.grad.clone() for k, p in net.named_parameters()}
    for rep in range(3):                                   # (allocator state differs from call to call)
        net.zero_grad(set_to_none=True)
        y = torch.nn.DataParallel(net, device_ids=[0, 0])(x)
        (y * gy).sum().backward()
        torch.cuda.synchronize()
        # a replica sees HALF the batch: its tiles differ, the sums over pixels are the same up to fp32 summation order
        assert (y - ref).abs().max().item() <= (1e-5 if prec == 'fp32' else 2e-2) * ref.abs().max().item()
        lim = 1e-4 if prec == 'fp32' else 2e-2
        for k, g in g_ref.items():
            got = net.get_parameter(k).grad
            assert got is not None, k
            err = (got - g).norm().item() / (g.norm().item() + 1e-20)
            assert err <= lim, (rep, k, err)


def test_data_parallel_discriminator_two_replicas_on_one_gpu(dev):
    """networks.py:136-137: `nn.DataParallel(netD, device_ids=[0, 0])`, BatchNorm in eval mode (batch statistics are per
    replica under DataParallel — SURVEY 8e — so only the eval form equals the one-batch result): logits and every
    parameter gradient against the plain module."""
    from esrganplus_amd import architecture as arch
    net = arch.Discriminator_VGG_128(3, 64).to(dev).eval()
    net.load_state_dict(synth.discriminator_state_dict(seed=12), strict=True)
    x = synth.image_batch(6, 4, 3, 128, 128, name='dpd2.x').to(dev)
    ref = net(x)
    ref.sum().backward()
    g_ref = {k: p.grad.clone() for k, p in net.named_parameters()}
    for rep in range(2):
        net.zero_grad(set_to_none=True)
        y = torch.nn.DataParallel(net, device_ids=[0, 0])(x)
        y.sum().backward()
        torch.cuda.synchronize()
        assert torch.allclose(y, ref, rtol=1e-5, atol=1e-6)
        for k, g in g_ref.items():
            got = net.get_parameter(k).grad
            assert got is not None and (got - g).norm().item() <= 1e-4 * (g.norm().item() + 1e-12), (rep, k)
