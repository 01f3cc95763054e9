"""GPU parity of Discriminator_VGG_128 and the VGG19 feature extractor (forward + backward) against
the golden vectors captured from the imported reference / torch.nn restatement (oracle/gen_golden.py)."""
import numpy as np
import pytest
import torch

from esrganplus_amd import synth
from tests.conftest import checks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def test_transposed_stride2_conv_is_adjoint(dev):
    """dgrad of the 4x4/s2 conv (upsample==2 mode) == autograd's conv_transpose."""
    from esrganplus_amd import engine as E, _lib as L
    g = np.random.default_rng(0)
    B, ci, co, H, W = 2, 48, 40, 12, 20
    w = torch.from_numpy(g.standard_normal((co, ci, 4, 4), dtype=np.float32)) * 0.1
    gy = torch.from_numpy(g.standard_normal((B, co, H, W), dtype=np.float32))
    ref = torch.nn.functional.conv_transpose2d(gy, w, stride=2, padding=1)       # [B, ci, 2H, 2W]
    wd = w.to(dev)
    dp = E.DgradPack([('c', wd)], 'fp32', dev, {'c': {'ts2': True}})
    st = E.current_stream()
    dp.ensure(st)
    gin = E.G32(B, co, H, W, 'fp32', dev)
    gout = E.G32(B, 64, 2 * H, 2 * W, 'fp32', dev)
    ops = L.OpList()
    gyd = gy.to(dev)
    out = torch.empty(B, ci, 2 * H, 2 * W, device=dev)
    lo = L.esr_layout()
    lo.dtype, lo.to_g32, lo.B, lo.C, lo.H, lo.W, lo.nchw, lo.g32 = L.ESR_F32, 1, B, co, H, W, gyd.data_ptr(), gin.view(0, co)
    ops.add(L.OP_LAYOUT, 'layout', lo)
    c = E._conv(L.ESR_F32, B, 2 * H, 2 * W, gin.view(0), co, gout.view(0, ci), dp.entries['c'], L.ACT_NONE,
                ks=4, stride=1, upsample=2)
    c.bias = None
    ops.add_conv(c)
    lo2 = L.esr_layout()
    lo2.dtype, lo2.to_g32, lo2.B, lo2.C, lo2.H, lo2.W, lo2.nchw, lo2.g32 = L.ESR_F32, 0, B, ci, 2 * H, 2 * W, out.data_ptr(), gout.view(0, ci)
    ops.add(L.OP_LAYOUT, 'layout', lo2)
    ops.run(st)
    torch.cuda.synchronize()
    assert (out.cpu() - ref).abs().max().item() <= 1e-4


def test_discriminator_golden(dev, golden):
    from esrganplus_amd import architecture as arch
    g = golden('disc')
    sd = synth.discriminator_state_dict(seed=4)
    net = arch.Discriminator_VGG_128(3, 64).to(dev)
    net.load_state_dict(sd, strict=True)
    x = synth.image_batch(4, 4, 3, 128, 128, name='disc.x').to(dev)
    gy = synth.normal_like(4, 'disc.gy', (4, 1)).to(dev)
    net.eval()
    with torch.no_grad():
        ye = net(x).cpu().numpy()
    assert np.abs(ye - g['y_eval']).max() <= 2e-4
    net.train()
    xr = x.clone().requires_grad_(True)
    y = net(xr)
    assert np.abs(y.detach().cpu().numpy() - g['y_train']).max() <= 2e-4
    (y * gy).sum().backward()
    gx = xr.grad.cpu().numpy()
    assert np.abs(gx[:, :, ::8, ::8] - g['gx_sub8']).max() <= 2e-4
    params = dict(net.named_parameters())
    for k in ('features.0.weight', 'features.3.weight', 'features.3.bias', 'features.26.bias',
              'features.27.weight', 'classifier.2.weight', 'classifier.0.bias'):
        ref = g['g_' + k]
        err = np.abs(params[k].grad.cpu().numpy() - ref).max()
        assert err <= 2e-3 * max(1.0, np.abs(ref).max()), (k, err)
    ref = g['g_features.2.weight_sub']
    assert np.abs(params['features.2.weight'].grad.cpu().numpy()[::4, ::4] - ref).max() <= 2e-3 * max(1.0, np.abs(ref).max())
    chk = np.stack([checks(p.grad) for p in params.values()])
    rel = np.abs(chk - g['gchk']) / np.maximum(1.0, np.abs(g['gchk'][:, 1:2]))
    assert rel.max() <= 2e-3, rel.max()
    # BN running statistics after 4 training forwards (SRRaGAN_model.py:133-134,149-150 -> 4 per step)
    with torch.no_grad():
        for i in range(3):
            net(x * (0.5 + 0.25 * i))
    bufs = dict(net.named_buffers())
    for k in ('features.3', 'features.15', 'features.27'):
        assert np.abs(bufs[k + '.running_mean'].cpu().numpy() - g['rm_' + k]).max() <= 1e-4
        assert np.abs(bufs[k + '.running_var'].cpu().numpy() - g['rv_' + k]).max() <= 1e-4
    assert int(bufs['features.3.num_batches_tracked']) == 4


@pytest.mark.parametrize('size,batch', [(96, 3), (192, 2)])
def test_discriminator_variants_golden(dev, golden, size, batch):
    """Discriminator_VGG_96 / _192 (architecture.py:178-270) on the HIP kernels against the reference's outputs."""
    from esrganplus_amd import architecture as arch
    g = golden('disc%d' % size)
    sd = synth.discriminator_state_dict(seed=40 + size, size=size)
    net = getattr(arch, 'Discriminator_VGG_%d' % size)(3, 64).to(dev)
    net.load_state_dict(sd, strict=True)
    x = synth.image_batch(size, batch, 3, size, size, name='disc%d.x' % size).to(dev)
    gy = synth.normal_like(size, 'disc%d.gy' % size, (batch, 1)).to(dev)
    net.eval()
    with torch.no_grad():
        assert np.abs(net(x).cpu().numpy() - g['y_eval']).max() <= 2e-4
    net.train()
    xr = x.clone().requires_grad_(True)
    y = net(xr)
    assert np.abs(y.detach().cpu().numpy() - g['y_train']).max() <= 2e-4
    (y * gy).sum().backward()
    params = dict(net.named_parameters())
    for k in ('classifier.0.bias', 'features.0.weight'):
        ref = g['g_' + k]
        assert np.abs(params[k].grad.cpu().numpy() - ref).max() <= 2e-3 * max(1.0, np.abs(ref).max()), k
    chk = np.stack([checks(p.grad) for p in params.values()])
    rel = np.abs(chk - g['gchk']) / np.maximum(1.0, np.abs(g['gchk'][:, 1:2]))
    assert rel.max() <= 2e-3, rel.max()
    gchk = checks(xr.grad)
    assert np.abs(gchk - g['gx_chk']).max() <= 2e-3 * max(1.0, np.abs(g['gx_chk'][1]))


def test_discriminator_frozen_params_still_give_input_grad(dev):
    """SRRaGAN_model.py:115-116: D's parameters are frozen during the G step."""
    from esrganplus_amd import architecture as arch
    net = arch.Discriminator_VGG_128(3, 64).to(dev).train()
    net.load_state_dict(synth.discriminator_state_dict(seed=5))
    x = synth.image_batch(5, 2, 3, 128, 128, name='d.frozen').to(dev).requires_grad_(True)
    for p in net.parameters():
        p.requires_grad = False
    net(x).sum().backward()
    g1 = x.grad.clone()
    assert all(p.grad is None for p in net.parameters())
    for p in net.parameters():
        p.requires_grad = True
    x.grad = None
    net(x).sum().backward()
    assert (x.grad - g1).abs().max().item() <= 1e-5 * max(1.0, g1.abs().max().item())
    assert all(p.grad is not None for p in net.parameters())


def test_vgg_golden(dev, golden):
    from esrganplus_amd import architecture as arch
    g = golden('vgg')
    netF = arch.VGGFeatureExtractor(feature_layer=34, use_bn=False, use_input_norm=True, device=dev).to(dev).eval()
    netF.load_state_dict(synth.vgg19_state_dict(6, 34), strict=False)
    x = synth.image_batch(6, 2, 3, 128, 128, name='vgg.x').to(dev)
    gy = synth.normal_like(6, 'vgg.gy', (2, 512, 8, 8)).to(dev)
    xr = x.clone().requires_grad_(True)
    y = netF(xr)
    assert tuple(y.shape) == (2, 512, 8, 8)
    assert np.abs(y.detach().cpu().numpy() - g['y']).max() <= 5e-4
    (y * gy).sum().backward()
    # 15 ReLUs + 4 max-pools: a pre-activation within fp32 round-off of 0 (or a pooling near-tie) may
    # resolve differently than in the oneDNN run that produced the golden, which moves a handful of
    # input-gradient pixels by O(1).  Gate on the relative L2 error and on the outlier fraction.
    ref = g['gx_sub2']
    got = xr.grad.cpu().numpy()[:, :, ::2, ::2]
    err = np.abs(got - ref)
    bad = (err > 2e-3 * max(1.0, np.abs(ref).max())).mean()
    rel = np.sqrt((err.astype(np.float64) ** 2).sum() / (ref.astype(np.float64) ** 2).sum())
    print('VGG dgrad: rel L2 %.3e, outlier fraction %.3e, max err %.3e' % (rel, bad, err.max()))
    assert rel <= 5e-3 and bad <= 1e-3
    chk = g['gx_chk']
    a = xr.grad.cpu().numpy().astype(np.float64)
    assert abs(np.abs(a).sum() - chk[1]) <= 5e-3 * chk[1]
    with torch.no_grad():
        y16 = netF.set_precision('fp16')(x)
    assert ((y16 - y.detach()).norm() / y.detach().norm()).item() <= 2e-2


def test_discriminator_fp16_grads_track_fp32(dev):
    """fp16 path (incl. the fp16 4x4/s2 and wide 3x3 wgrad kernels with tap-major accumulation)."""
    from esrganplus_amd import architecture as arch
    sd = synth.discriminator_state_dict(seed=7)
    x = synth.image_batch(7, 4, 3, 128, 128, name='d16.x').to(dev)
    gy = synth.normal_like(7, 'd16.gy', (4, 1)).to(dev)
    grads, gxs = {}, {}
    for prec in ('fp32', 'fp16'):
        net = arch.Discriminator_VGG_128(3, 64).to(dev).train().set_precision(prec)
        net.load_state_dict(sd)
        xr = x.clone().requires_grad_(True)
        scale = 1024.0 if prec == 'fp16' else 1.0        # static loss scaling, as train.py does
        (net(xr) * gy * scale).sum().backward()
        grads[prec] = {k: p.grad.clone() / scale for k, p in net.named_parameters()}
        gxs[prec] = xr.grad.clone() / scale
    # fp16 activations flip a few LeakyReLU signs (9 BatchNorms re-normalise the rounding noise), which
    # alone moves gradients by ~10-15 % in norm — even classifier.0, which is computed in fp32 from
    # the exported features.  So gate on direction (cosine) and a loose norm bound: an indexing bug in
    # the fp16 wgrad kernels (taps, transposed reads, tap-major scatter) gives cosines far below 0.9.
    worst = {}
    bn_fed = {'features.%d.bias' % i for i in (2, 5, 8, 11, 14, 17, 20, 23, 26)}
    for k in grads['fp32']:
        if k in bn_fed:      # a bias in front of train-mode BN has an exactly-zero gradient: pure round-off
            continue
        a, b = grads['fp32'][k].flatten(), grads['fp16'][k].flatten()
        cos = torch.nn.functional.cosine_similarity(a, b, dim=0).item()
        worst[k] = (round(cos, 4), round(((a - b).norm() / a.norm().clamp_min(1e-6)).item(), 4))
    print(worst)
    bad = {k: v for k, v in worst.items() if v[0] < 0.97 or v[1] > 0.3}
    assert not bad, bad
    a, b = gxs['fp32'].flatten(), gxs['fp16'].flatten()
    assert torch.nn.functional.cosine_similarity(a, b, dim=0).item() >= 0.97


def _ragan(ya, yb):
    f = torch.nn.functional.binary_cross_entropy_with_logits
    return (f(ya - yb.mean(), torch.ones_like(ya)) + f(yb - ya.mean(), torch.zeros_like(yb))) / 2


@pytest.mark.parametrize('prec,tol', [('fp32', 2e-4), ('fp16', 3e-2)])
@pytest.mark.parametrize('mode', ['d_step', 'g_step'])
def test_discriminator_forward_pair_matches_two_calls(dev, mode, prec, tol):
    """``forward_pair(a, b)`` (one pass over the concatenated batch, BatchNorm statistics per half) against the
    two calls of the reference's train step (SRRaGAN_model.py:133-134 G step: D frozen, ``real`` detached;
    150-151 D step): logits, input / parameter gradients, running statistics and num_batches_tracked."""
    from esrganplus_amd import architecture as arch
    sd = synth.discriminator_state_dict(5)
    a0 = synth.image_batch(61, 3, 3, 128, 128, name='pair.a').to(dev)
    b0 = synth.image_batch(62, 3, 3, 128, 128, name='pair.b').to(dev)
    res = {}
    for how in ('two', 'pair'):
        net = arch.Discriminator_VGG_128(3, 64).to(dev).train().set_precision(prec)
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
            assert yb.requires_grad == (mode == 'd_step')
        _ragan(ya, yb).backward()
        bn = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
        res[how] = dict(ya=ya.detach(), yb=yb.detach(), ga=a.grad,
                        gp=[p.grad for p in net.parameters()] if mode == 'd_step' else [],
                        rm=[m.running_mean.clone() for m in bn], rv=[m.running_var.clone() for m in bn],
                        nbt=[int(m.num_batches_tracked) for m in bn])
    two, pair = res['two'], res['pair']
    assert pair['nbt'] == two['nbt'] == [2] * len(two['nbt'])
    rel = lambda x, y: ((x - y).abs().max() / y.abs().max().clamp_min(1e-12)).item()
    assert rel(pair['ya'], two['ya']) <= tol and rel(pair['yb'], two['yb']) <= tol
    for x, y in zip(pair['rm'] + pair['rv'], two['rm'] + two['rv']):
        assert rel(x, y) <= max(tol * 0.1, 1e-5)
    if mode == 'g_step':
        assert rel(pair['ga'], two['ga']) <= tol
    else:
        assert pair['ga'] is None
        gmax = max(y.abs().max().item() for y in two['gp'])
        for x, y in zip(pair['gp'], two['gp']):       # (conv biases in front of a BatchNorm: exact gradient 0, noise)
            assert (x - y).abs().max().item() <= tol * max(y.abs().max().item(), 1e-3 * gmax)


@pytest.mark.parametrize('prec', ['fp32', 'fp16'])
def test_two_stage_pair_forward_is_the_one_pass_pair_forward(dev, prec):
    """``_pair_begin(real)`` + ``_pair_finish(plan, fake)`` (the train step runs netD's `real` half on the side stream
    under the generator's forward and the `fake` half behind it) against ONE dual pair forward over ``cat([fake, real])``:
    the same launches on half the batch each, so logits, both backward passes (the D step's parameter gradients over
    the whole batch, the G step's input gradient of the fake half) and the BatchNorm buffers after the deferred update
    (plan.restat1) and the second pair's replay (plan.restat) must agree BIT FOR BIT."""
    from esrganplus_amd import architecture as arch, convnet as CN, engine as E
    sd = synth.discriminator_state_dict(9)
    n = 3
    fake = synth.image_batch(91, n, 3, 128, 128, name='two.f').to(dev)
    real = synth.image_batch(92, n, 3, 128, 128, name='two.r').to(dev)
    gy = synth.image_batch(93, 2 * n, 1, 1, 1, name='two.g').to(dev).reshape(2 * n, 1)
    res = {}
    for how in ('one', 'two'):
        net = arch.Discriminator_VGG_128(3, 64).to(dev).train().set_precision(prec)
        net.load_state_dict(sd)
        with torch.no_grad():
            if how == 'one':
                out, lease = net._run_forward(torch.cat([fake, real]), need_bwd=True, groups=2, dual=n)
                P = lease.plan
            else:
                P, lease = net._pair_begin(real)
                out = net._pair_finish(P, fake)
                P.restat1.run(E.current_stream())
            P.restat.run(E.current_stream())
            P.gy_tensor.copy_(gy)
            P.second.gy_tensor.copy_(gy[:n])
            CN.run_pass_into(P)
            CN.run_pass_into(P.second)
            torch.cuda.synchronize()
            bn = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
            res[how] = dict(out=out.clone(), grads=P.grad_flat.clone(), gx=P.second.gx_tensor.clone(),
                            rm=[m.running_mean.clone() for m in bn], rv=[m.running_var.clone() for m in bn],
                            nbt=[int(m.num_batches_tracked) for m in bn])
        lease.release()
    one, two = res['one'], res['two']
    assert two['nbt'] == one['nbt'] == [4] * len(one['nbt'])
    assert torch.equal(one['out'], two['out'])
    assert torch.equal(one['gx'], two['gx'])
    assert torch.equal(one['grads'], two['grads'])
    for x, y in zip(one['rm'] + one['rv'], two['rm'] + two['rv']):
        assert torch.equal(x, y)


@pytest.mark.parametrize('prec,tol', [('fp32', 2e-4), ('fp16', 3e-2)])
def test_discriminator_forward_shared_matches_four_calls(dev, prec, tol):
    """The train step calls netD four times with unchanged weights — G step: netD(fake), netD(real).detach() with D
    frozen (SRRaGAN_model.py:133-134), D step: netD(real), netD(fake.detach()) (150-151) — and the second pair sees
    the values of the first.  ``forward_shared`` runs ONE forward for all four: its logits, the gradient it gives
    ``fake`` (first pair's loss), the parameter gradients (second pair's loss), and the BatchNorm buffers after the
    four calls (updates in call order fake, real, real, fake; num_batches_tracked + 4) against four separate calls."""
    from esrganplus_amd import architecture as arch
    sd = synth.discriminator_state_dict(7)
    f0 = synth.image_batch(81, 3, 3, 128, 128, name='shared.f').to(dev)
    r0 = synth.image_batch(82, 3, 3, 128, 128, name='shared.r').to(dev)
    res = {}
    for how in ('four', 'shared'):
        net = arch.Discriminator_VGG_128(3, 64).to(dev).train().set_precision(prec)
        net.load_state_dict(sd)
        fake, real = f0.clone().requires_grad_(True), r0.clone()
        for p in net.parameters():
            p.requires_grad = False
        if how == 'four':
            pg, pr = net(fake), net(real).detach()
        else:
            pg, pr, h = net.forward_shared(fake, real)
            assert not pr.requires_grad
        _ragan(pr, pg).backward()                       # G step's relativistic term -> d/d fake
        for p in net.parameters():
            p.requires_grad = True
        if how == 'four':
            dr, df = net(real), net(fake.detach())
        else:
            dr, df = h.second_pass()
        (2.0 * _ragan(dr, df)).backward()               # D step's loss -> parameter gradients
        bn = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
        res[how] = dict(pg=pg.detach(), pr=pr.detach(), dr=dr.detach(), df=df.detach(), gf=fake.grad,
                        gp=[p.grad for p in net.parameters()],
                        rm=[m.running_mean.clone() for m in bn], rv=[m.running_var.clone() for m in bn],
                        nbt=[int(m.num_batches_tracked) for m in bn])
    four, sh = res['four'], res['shared']
    assert sh['nbt'] == four['nbt'] == [4] * len(four['nbt'])
    rel = lambda x, y: ((x - y).abs().max() / y.abs().max().clamp_min(1e-12)).item()
    for k in ('pg', 'pr', 'dr', 'df', 'gf'):
        assert rel(sh[k], four[k]) <= tol, k
    assert torch.equal(sh['dr'], sh['pr']) and torch.equal(sh['df'], sh['pg'])
    for x, y in zip(sh['rm'] + sh['rv'], four['rm'] + four['rv']):
        assert rel(x, y) <= max(tol * 0.1, 1e-5)
    gmax = max(y.abs().max().item() for y in four['gp'])
    for x, y in zip(sh['gp'], four['gp']):       # (conv biases in front of a BatchNorm: exact gradient 0, noise)
        assert (x - y).abs().max().item() <= tol * max(y.abs().max().item(), 1e-3 * gmax)


def test_vgg_forward_pair_matches_two_calls(dev):
    """netF(fake) / netF(real).detach() (SRRaGAN_model.py:128-129) as one batch: features and d/d fake."""
    from esrganplus_amd import architecture as arch
    net = arch.VGGFeatureExtractor(34, False, True, dev).to(dev).eval().set_precision('fp32')
    net.load_state_dict(synth.vgg19_state_dict(3, 34), strict=False)
    a0 = synth.image_batch(71, 2, 3, 64, 64, name='vpair.a').to(dev)
    b0 = synth.image_batch(72, 2, 3, 64, 64, name='vpair.b').to(dev)
    out = {}
    for how in ('two', 'pair'):
        a = a0.clone().requires_grad_(True)
        if how == 'two':
            fa, fb = net(a), net(b0).detach()
        else:
            fa, fb = net.forward_pair(a, b0)
            assert not fb.requires_grad
        torch.nn.functional.l1_loss(fa, fb).backward()
        out[how] = (fa.detach(), fb, a.grad)
    for x, y in zip(out['pair'], out['two']):
        assert torch.equal(x, y)


def test_discriminator_sn_matches_reference_golden(dev, golden):
    """Discriminator_VGG_128_SN (architecture.py:131-175 + spectral_norm.py) against tests/golden/disc_sn.npz, captured
    from the imported reference: the first training forward's logits, input gradient and ALL parameter gradients
    (through W / sigma to weight_orig), the second training forward (another power iteration on the updated u), the u
    and normalised-weight buffers both calls leave, and an eval forward on those buffers."""
    from esrganplus_amd import architecture as arch
    g = golden('disc_sn')
    sd = synth.discriminator_sn_state_dict(seed=6)
    net = arch.Discriminator_VGG_128_SN().to(dev)
    net.load_state_dict(sd, strict=True)
    assert sorted(net.state_dict().keys()) == sorted(sd.keys())
    x = synth.image_batch(6, 3, 3, 128, 128, name='dsn.x').to(dev)
    gy = synth.normal_like(6, 'dsn.gy', (3, 1)).to(dev)
    net.train()
    xr = x.clone().requires_grad_(True)
    y1 = net(xr)
    assert np.abs(y1.detach().cpu().numpy() - g['y1']).max() <= 2e-4 * max(1.0, np.abs(g['y1']).max())
    (y1 * gy).sum().backward()
    assert np.abs(checks(xr.grad) - g['gx_chk']).max() <= 2e-3 * max(1.0, abs(g['gx_chk'][1]))
    assert np.abs(xr.grad.cpu().numpy()[:, :, ::8, ::8] - g['gx_sub8']).max() <= 2e-3 * max(1e-6, np.abs(g['gx_sub8']).max())
    params = dict(net.named_parameters())
    keys = [str(k) for k in g['keys']]
    assert keys == sorted(params.keys())
    chk = np.stack([checks(params[k].grad) for k in keys])
    rel = np.abs(chk - g['gchk']) / np.maximum(1e-3, np.abs(g['gchk'][:, 1:2]))
    assert rel.max() <= 3e-3, (keys[int(rel.argmax() // 3)], rel.max())
    for k in ('conv0.weight_orig', 'conv0.bias', 'conv3.bias', 'linear1.weight_orig', 'linear0.bias'):
        want = g['g_' + k]
        assert np.abs(params[k].grad.cpu().numpy() - want).max() <= 3e-3 * max(1e-6, np.abs(want).max()), k
    want = g['g_conv5.weight_orig_sub']
    assert np.abs(params['conv5.weight_orig'].grad.cpu().numpy()[::8, ::8] - want).max() <= 3e-3 * np.abs(want).max()
    with torch.no_grad():
        y2 = net(x * 0.75)
    assert np.abs(y2.cpu().numpy() - g['y2']).max() <= 2e-4 * max(1.0, np.abs(g['y2']).max())
    bufs = dict(net.named_buffers())
    for k in ('conv0', 'conv4', 'conv9', 'linear0', 'linear1'):
        assert np.abs(bufs[k + '.weight_u'].cpu().numpy() - g['u_' + k]).max() <= 1e-5, k
        assert np.abs(checks(bufs[k + '.weight']) - g['wchk_' + k]).max() <= 1e-4 * max(1.0, g['wchk_' + k][1]), k
    net.eval()
    with torch.no_grad():
        ye = net(x)
    assert np.abs(ye.cpu().numpy() - g['y_eval']).max() <= 2e-4 * max(1.0, np.abs(g['y_eval']).max())


def test_discriminator_sn_two_forwards_then_backward(dev, golden):
    """The D step's call order (SRRaGAN_model.py:150-167): netD(real), netD(fake) — two training forwards, each with its
    own power iteration and therefore its own W / sigma — and THEN the backward of both.  The first call's backward must
    run on the weights its forward used (the module's weight buffers have been rewritten by the second call by then):
    every parameter gradient and dL/dx of the first call against the imported reference (tests/golden/disc_sn_two.npz)."""
    from esrganplus_amd import architecture as arch
    g = golden('disc_sn_two')
    net = arch.Discriminator_VGG_128_SN().to(dev)
    net.load_state_dict(synth.discriminator_sn_state_dict(seed=8), strict=True)
    xa = synth.image_batch(8, 2, 3, 128, 128, name='dsn2.xa').to(dev).requires_grad_(True)
    xb = synth.image_batch(9, 2, 3, 128, 128, name='dsn2.xb').to(dev)
    ga = synth.normal_like(8, 'dsn2.ga', (2, 1)).to(dev)
    gb = synth.normal_like(9, 'dsn2.gb', (2, 1)).to(dev)
    net.train()
    ya = net(xa)
    yb = net(xb)
    assert np.abs(ya.detach().cpu().numpy() - g['ya']).max() <= 2e-4 * max(1.0, np.abs(g['ya']).max())
    assert np.abs(yb.detach().cpu().numpy() - g['yb']).max() <= 2e-4 * max(1.0, np.abs(g['yb']).max())
    ((ya * ga).sum() + (yb * gb).sum()).backward()
    params = dict(net.named_parameters())
    keys = [str(k) for k in g['keys']]
    chk = np.stack([checks(params[k].grad) for k in keys])
    rel = np.abs(chk - g['gchk']) / np.maximum(1e-3, np.abs(g['gchk'][:, 1:2]))
    e_chk = np.abs(checks(xa.grad) - g['gx_chk']).max() / max(1.0, abs(g['gx_chk'][1]))
    e_sub = np.abs(xa.grad.cpu().numpy()[:, :, ::8, ::8] - g['gx_sub8']).max() / max(1e-6, np.abs(g['gx_sub8']).max())
    print('SN two forwards: dL/dx checks %.2e, sub8 %.2e; parameter checks worst %.2e (%s)'
          % (e_chk, e_sub, rel.max(), keys[int(rel.argmax() // 3)]))
    # (with the module-wide packs of round 3 — the first call's backward on the second call's weights — these read
    # 1.7e-1 / 5.8e-1 and 4.4e-2 on the parameters; single pixels of a gradient whose maximum is 2e-5 move by a few
    # 1e-3 of that maximum through LeakyReLU masks of pre-activations within fp32 rounding of zero)
    assert e_chk <= 2e-3 and e_sub <= 1e-2, (e_chk, e_sub)
    assert rel.max() <= 3e-3, (keys[int(rel.argmax() // 3)], rel.max())
    for k in ('conv0.weight_orig', 'conv9.bias', 'linear1.weight_orig', 'linear0.bias'):
        want = g['g_' + k]
        assert np.abs(params[k].grad.cpu().numpy() - want).max() <= 3e-3 * max(1e-6, np.abs(want).max()), k


@pytest.mark.parametrize('case', [(512, 512, 4, 32, 8), (512, 256, 8, 16, 4), (256, 128, 16, 9, 2), (64, 96, 4, 3, 2), (160, 64, 8, 5, 4)])
def test_transposed_stride2_conv_packed_split_k(dev, case):
    """Input gradient of the discriminator's deep 4x4/s2 convs (esr_conv.upsample == 2 on 8 / 16 / 32-column output
    maps): with esr_conv.ksplit the tile holds several images and the K loop (the forward conv's output channels) is
    split over workgroups, finished in split order.  Against autograd's conv_transpose2d on the fp16-rounded operands,
    against the one-image-per-tile launch (<= 1 fp16 ulp: summation order only), bit-identical run to run; batches that
    do not fill the last tile, forward input channels that do not fill the last 32-block."""
    from esrganplus_amd import engine as E, _lib as L
    co, ci, H, B, ksplit = case                     # forward conv: ci -> co, output H x H; its input gradient is 2H x 2H
    g = np.random.default_rng(co + ci + H + B)
    w = torch.from_numpy(g.standard_normal((co, ci, 4, 4), dtype=np.float32)) * (1.0 / np.sqrt(co * 4))
    gy = torch.from_numpy(g.standard_normal((B, co, H, H), dtype=np.float32))
    ref = torch.nn.functional.conv_transpose2d(gy.half().float(), w.half().float(), stride=2, padding=1)
    wd = w.to(dev)
    dp = E.DgradPack([('c', wd)], 'fp16', dev, {'c': {'ts2': True}})
    st = E.current_stream()
    dp.ensure(st)
    outs = []
    for ks_ in (ksplit, ksplit, 0):
        gin = E.G32(B, co, H, H, 'fp16', dev)
        gout = E.G32(B, ((ci + 31) // 32) * 32, 2 * H, 2 * H, 'fp16', dev)
        ops = L.OpList()
        gyd = gy.to(dev)
        out = torch.empty(B, ci, 2 * H, 2 * H, device=dev)
        lo = L.esr_layout()
        lo.dtype, lo.to_g32, lo.B, lo.C, lo.H, lo.W, lo.nchw, lo.g32 = L.ESR_F16, 1, B, co, H, H, gyd.data_ptr(), gin.view(0, co)
        ops.add(L.OP_LAYOUT, 'layout', lo)
        c = E._conv(L.ESR_F16, B, 2 * H, 2 * H, gin.view(0), co, gout.view(0, ci), dp.entries['c'], L.ACT_NONE,
                    ks=4, stride=1, upsample=2)
        c.bias = None
        ws = None
        if ks_:
            ws = torch.empty(ks_ * B * 4 * H * H * ((ci + 31) // 32) * 32, dtype=torch.float32, device=dev)
            c.ksplit, c.split_ws = ks_, ws.data_ptr()
        ops.add_conv(c)
        lo2 = L.esr_layout()
        lo2.dtype, lo2.to_g32, lo2.B, lo2.C, lo2.H, lo2.W, lo2.nchw, lo2.g32 = L.ESR_F16, 0, B, ci, 2 * H, 2 * H, out.data_ptr(), gout.view(0, ci)
        ops.add(L.OP_LAYOUT, 'layout', lo2)
        ops.run(st)
        torch.cuda.synchronize()
        outs.append(out.cpu())
    scale = max(1.0, ref.abs().max().item())
    assert torch.equal(outs[0], outs[1])
    assert (outs[0] - ref).abs().max().item() <= 2e-3 * scale
    assert (outs[0] - outs[2]).abs().max().item() <= 2.0 ** -10 * scale


_VGG_ODD_REF = {}


@pytest.mark.parametrize('prec', ['fp32', 'fp16'])
@pytest.mark.parametrize('hw', [(100, 120), (72, 40), (132, 68)])
def test_vgg_at_map_sizes_that_leave_odd_pools(dev, hw, prec):
    """VGGFeatureExtractor at HR sizes that are not multiples of 16: 100 x 120 pools a 25 x 30 and a 12 x 15 map,
    72 x 40 a 9 x 5 map, 132 x 68 a 33 x 17 map, so MaxPool2d drops a row or a column (which gets gradient 0; at
    33 rows the pooled map's 2 x 16 rows take one padded-plane size less than the 33 the conv in front reads: the
    plan sizes the pool's gradient buffer as the conv's output, not as the pooled region).  Expected: the plan takes these
    sizes (no HipExtensionError) and matches oracle.ref_torch.vgg19_features_forward in float64 with autograd.
    Features: fp32 within 1e-4 of the output scale, fp16 within test_vgg_golden's relative L2 of 2e-2.
    Input gradient: a ReLU pre-activation or a pooling pair within fp32 round-off of a tie resolves differently here
    and in float64 and moves the gradient of that element by O(1), spread over its receptive field in the input (at
    100 x 120 a single flip in conv1 leaves a 3 x 3 cluster at ~5e-4 relative L2, one in the third pool ~8e-3 spread
    over a tenth of the image); so the fp32 gradient is gated on its relative L2 error, <= 2e-2, which a wrong row or
    column of a pooled map (~1/25 of it) exceeds.  fp16 stores every
    activation in fp16, which flips many more of those decisions: 0.11-0.13 relative L2 at 64^2, 128^2 and these
    sizes alike, gated at 0.2."""
    from esrganplus_amd import architecture as arch
    from oracle import ref_torch as RT
    H, W = hw
    sd = synth.vgg19_state_dict(8, 34)
    x = synth.image_batch(8, 2, 3, H, W, name='vgg_odd.x')
    gy = synth.normal_like(8, 'vgg_odd.gy', (2, 512, H // 16, W // 16))
    if hw not in _VGG_ODD_REF:
        xr = x.double().requires_grad_(True)
        yr = RT.vgg19_features_forward(xr, {k: v.double() for k, v in sd.items()}, 34, True)
        (yr * gy.double()).sum().backward()
        _VGG_ODD_REF[hw] = (yr.detach(), xr.grad)
    yref, gref = _VGG_ODD_REF[hw]
    net = arch.VGGFeatureExtractor(34, False, True, dev).to(dev).eval()
    net.load_state_dict(sd, strict=False)
    net.set_precision(prec)
    xd = x.to(dev).requires_grad_(True)
    y = net(xd)
    assert tuple(y.shape) == tuple(yref.shape)
    (y * gy.to(dev)).sum().backward()
    y, g = y.detach().cpu().double(), xd.grad.cpu().double()
    rel = lambda a, b: ((a - b).norm() / b.norm()).item()  # noqa: E731
    ey, eg = (y - yref).abs().max().item() / yref.abs().max().item(), rel(g, gref)
    out = ((g - gref).abs() > 2e-3 * gref.abs().max()).double().mean().item()
    print('VGG %dx%d %s: features max err / scale %.3e, rel L2 %.3e; input grad rel L2 %.3e, outliers %.3e'
          % (H, W, prec, ey, rel(y, yref), eg, out))
    if prec == 'fp32':
        assert ey <= 1e-4
        assert eg <= 2e-2
    else:
        assert rel(y, yref) <= 2e-2 and eg <= 0.2
