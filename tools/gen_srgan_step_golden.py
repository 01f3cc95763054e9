#!/usr/bin/env python
"""Pins ``train.SRGANStep`` against the reference's own ``SRGANModel`` (codes/models/SRGAN_model.py, built by
``models.create_model({'model': 'srgan'})``): writes tests/golden/srgan_step.npz, srgan_steps4.npz and
srgan_step_srresnet.npz.  Needs the reference checkout (oracle.ref_import), CPU only:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_srgan_step_golden.py

srgan_step.npz — cases 'vanilla' and 'lsgan' (``gan_type``): one ``optimize_parameters(1)`` at the set-up and seeds of
tools/gen_psnr_step_golden.py: gen_train_step_l2 (nb = 2, batch 4 of 32 x 32 LR, 'l2' pixel and feature criteria, the
``install_vgg_stub(6)`` feature net).  Besides that file's contents: ``D_buf_chk`` — checksums of every BatchNorm
buffer of netD after the step's three calls (fake, real, fake) —, ``D_buf_tol`` — what a test may allow on them, see
``buf_tol`` —, ``num_batches_tracked``, and three layers' running statistics in full.  The buffers are also computed
under two WRONG call orders, (fake, real, real, fake) and (real, fake), and each is asserted to move ``D_buf_chk`` by at
least ten times ``D_buf_tol``: else the order would not be pinned.
srgan_steps4.npz — 'vanilla', four iterations of the loop body of codes/train.py:97-106 (``update_learning_rate()``
BEFORE ``optimize_parameters``), MultiStepLR([2], 0.5), ``D_update_ratio`` 2, ``D_init_iters`` 1 (G moves at iterations
2 and 4 only), fresh data and noise per iteration.
srgan_step_srresnet.npz — one 'vanilla' step with ``which_model_G: sr_resnet`` (nb = 2, pixelshuffle), no noise.
Weights, inputs and noise are regenerated from the recorded seeds and names (esrganplus_amd.synth): the files hold
seeds, names, shapes and results only.  An existing file is compared with what was generated."""
import os
import sys
import types
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from esrganplus_amd import synth
from oracle import ref_import as RI
from oracle import ref_torch as RT
from oracle.gen_golden import checks, draw_z, inject_z, install_vgg_stub, npy

LOG_KEYS = ('l_g_pix', 'l_g_fea', 'l_g_gan', 'l_d_real', 'l_d_fake', 'D_real', 'D_fake')
NB = 2
BUF_ELEM_TOL = 1e-4          # tests/test_gpu_dnet_vgg.py: test_discriminator_golden, per element of a running statistic
FULL_BUFS = ('features.3', 'features.15', 'features.27')


def _network_G(which='RRDB_net'):
    return {'which_model_G': which, 'norm_type': None, 'mode': 'CNA', 'nf': 64, 'nb': NB, 'in_nc': 3,
            'out_nc': 3, 'gc': 32, 'scale': 4}


def _opt(gan_type, which='RRDB_net', criterion='l2', lr_steps=(50000, 100000, 200000, 300000), ratio=None, init=None):
    return {'model': 'srgan', 'scale': 4, 'gpu_ids': None, 'is_train': True,
            'path': {'pretrain_model_G': None, 'pretrain_model_D': None},
            'network_G': _network_G(which),
            'network_D': {'which_model_D': 'discriminator_vgg_128', 'norm_type': 'batch',
                          'act_type': 'leakyrelu', 'mode': 'CNA', 'nf': 64, 'in_nc': 3},
            'train': {'lr_G': 1e-4, 'weight_decay_G': 0, 'beta1_G': 0.9, 'lr_D': 1e-4,
                      'weight_decay_D': 0, 'beta1_D': 0.9, 'lr_scheme': 'MultiStepLR',
                      'lr_steps': list(lr_steps), 'lr_gamma': 0.5,
                      'pixel_criterion': criterion, 'pixel_weight': 0.01, 'feature_criterion': criterion,
                      'feature_weight': 1, 'gan_type': gan_type, 'gan_weight': 0.005,
                      'D_update_ratio': ratio, 'D_init_iters': init}}


def _create(opt):
    install_vgg_stub(6)
    sys.modules.setdefault('cv2', types.ModuleType('cv2'))
    RI.codes_arch()
    from models import create_model
    with RI.cuda_to_cpu():
        return create_model(opt)


def _bn_buffers(netD):
    return [(k, v) for k, v in netD.named_buffers() if k.endswith('running_mean') or k.endswith('running_var')]


def buf_chk(netD):
    return np.stack([checks(v) for _, v in _bn_buffers(netD)])


def buf_tol(netD):
    """What BUF_ELEM_TOL per element allows on the three checksums of a buffer of C elements: C times it on the sum
    and the abs-sum (triangle inequality), sqrt(C) times it on the L2 norm."""
    return np.stack([np.array([v.numel(), v.numel(), np.sqrt(v.numel())]) * BUF_ELEM_TOL for _, v in _bn_buffers(netD)])


def nbt(netD):
    return np.array([int(v) for k, v in netD.named_buffers() if k.endswith('num_batches_tracked')], dtype=np.int64)


def _buffers_after(sdD, calls):
    """netD's BatchNorm checksums after the training-mode calls `calls` on the weights `sdD`."""
    arch, _ = RI.codes_arch()
    net = arch.Discriminator_VGG_128(3, 64, norm_type='batch', act_type='leakyrelu', mode='CNA').train()
    net.load_state_dict(sdD, strict=True)
    with torch.no_grad():
        for x in calls:
            net(x)
    return buf_chk(net)


def _results(model, sdG, sdD, full_G, full_D):
    res = {}
    for k, v in model.get_current_log().items():
        res['log_' + k] = np.array(float(v))
        print('  %-10s %.6e' % (k, float(v)))
    res['fake_H_chk'] = checks(model.fake_H)
    res['fake_H_sub4'] = npy(model.fake_H)[:, :, ::4, ::4]
    g = dict(model.netG.named_parameters())
    d = dict(model.netD.named_parameters())
    res['G_new_chk'] = np.stack([checks(g[k]) for k in sdG.keys()])
    res['D_new_chk'] = np.stack([checks(d[k]) for k in d.keys()])
    res['G_delta_' + full_G] = npy(g[full_G] - sdG[full_G])
    res['D_delta_' + full_D] = npy(d[full_D] - sdD[full_D])
    res['D_buf_chk'] = buf_chk(model.netD)
    res['D_buf_tol'] = buf_tol(model.netD)
    res['num_batches_tracked'] = nbt(model.netD)
    bufs = dict(model.netD.named_buffers())
    for k in FULL_BUFS:
        res['rm_' + k] = npy(bufs[k + '.running_mean'])
        res['rv_' + k] = npy(bufs[k + '.running_var'])
    return res


def _assert_order_is_pinned(res, sdD, fake, real):
    tol = res['D_buf_tol']
    same = _buffers_after(sdD, (fake, real, fake))
    assert np.all(np.abs(same - res['D_buf_chk']) <= 0.1 * tol), 'the replay (fake, real, fake) is not the step'
    for name, calls in (('fake, real, real, fake', (fake, real, real, fake)), ('real, fake', (real, fake))):
        moved = (np.abs(_buffers_after(sdD, calls) - res['D_buf_chk']) / tol).max()
        print('  call order (%s) moves D_buf_chk by %.1f x the tolerance' % (name, moved))
        assert moved >= 10.0, (name, moved)


def gen_srgan_step():
    out = {'cases': np.array(['vanilla', 'lsgan']), 'seeds': np.array([30, 31, 30, 30, 9], dtype=np.int64),
           'names': np.array(['step.lr', 'step.hr', 'step.z'])}
    for gan_type in ('vanilla', 'lsgan'):
        print('[gen_srgan_step_golden] SRGANModel,', gan_type)
        model = _create(_opt(gan_type))
        sdG, sdD = synth.rrdbnet_state_dict(nb=NB, seed=30), synth.discriminator_state_dict(seed=31)
        model.netG.load_state_dict(sdG, strict=True)
        model.netD.load_state_dict(sdD, strict=True)
        lr = synth.image_batch(30, 4, 3, 32, 32, name='step.lr')
        hr = synth.image_batch(30, 4, 3, 128, 128, name='step.hr')
        model.feed_data({'LR': lr, 'HR': hr})
        with inject_z(draw_z(9, RT.noise_shapes(lr.shape, NB, 'codes'), 'step.z')):
            model.optimize_parameters(1)
        res = _results(model, sdG, sdD, 'model.0.weight', 'classifier.2.weight')
        assert np.all(res['num_batches_tracked'] == 3)
        _assert_order_is_pinned(res, sdD, model.fake_H.detach(), hr)
        out.update({gan_type + '.' + k: v for k, v in res.items()})
    return out


def gen_srgan_steps4():
    print('[gen_srgan_step_golden] SRGANModel, four iterations, D_update_ratio 2, D_init_iters 1')
    model = _create(_opt('vanilla', lr_steps=(2,), ratio=2, init=1))
    sdG, sdD = synth.rrdbnet_state_dict(nb=NB, seed=32), synth.discriminator_state_dict(seed=33)
    model.netG.load_state_dict(sdG, strict=True)
    model.netD.load_state_dict(sdD, strict=True)
    g = dict(model.netG.named_parameters())
    d = dict(model.netD.named_parameters())
    res = {'D_update_ratio': np.int64(2), 'D_init_iters': np.int64(1), 'lr_steps': np.array([2], dtype=np.int64),
           'seeds': np.array([32, 33, 70, 80, 90], dtype=np.int64),
           'names': np.array(['srgan4.lr', 'srgan4.hr', 'srgan4.z'])}
    G0 = np.stack([checks(sdG[k]) for k in sdG.keys()])
    for it in range(1, 5):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')          # "lr_scheduler.step() before optimizer.step()": the reference's order
            model.update_learning_rate()
        lr = synth.image_batch(70 + it, 4, 3, 32, 32, name='srgan4.lr')
        hr = synth.image_batch(80 + it, 4, 3, 128, 128, name='srgan4.hr')
        model.feed_data({'LR': lr, 'HR': hr})
        with inject_z(draw_z(90 + it, RT.noise_shapes(lr.shape, NB, 'codes'), 'srgan4.z')):
            model.optimize_parameters(it)
        log = model.get_current_log()
        res['lr_%d' % it] = np.array([model.optimizer_G.param_groups[0]['lr'], model.optimizer_D.param_groups[0]['lr']])
        res['log_keys_%d' % it] = np.array([k for k in LOG_KEYS if k in log])
        res['log_%d' % it] = np.array([float(log[k]) for k in LOG_KEYS if k in log])
        res['fake_H_chk_%d' % it] = checks(model.fake_H)
        print('  iteration %d lr %s  %s' % (it, res['lr_%d' % it], dict(zip(res['log_keys_%d' % it], res['log_%d' % it]))))
        Gc = np.stack([checks(g[k]) for k in sdG.keys()])
        if it == 1:
            res['G_chk_1'] = Gc
            assert np.array_equal(Gc, G0), 'G moved at iteration 1'
            assert not any(k.startswith('l_g_') for k in log)
        if it == 2:
            assert not np.array_equal(Gc, G0), 'G did not move at iteration 2'
            G2 = Gc
        if it == 3:
            assert np.array_equal(Gc, G2), 'G moved at iteration 3'
    res['G_chk'] = np.stack([checks(g[k]) for k in sdG.keys()])
    res['D_chk'] = np.stack([checks(d[k]) for k in d.keys()])
    for k in ('model.0.weight', 'model.1.sub.1.RDB2.conv3.0.bias'):
        res['G_delta_' + k] = npy(g[k] - sdG[k])
    for k in ('classifier.2.weight', 'features.3.weight'):
        res['D_delta_' + k] = npy(d[k] - sdD[k])
    res['D_buf_chk'] = buf_chk(model.netD)
    res['D_buf_tol'] = buf_tol(model.netD)
    res['num_batches_tracked'] = nbt(model.netD)
    assert np.all(res['num_batches_tracked'] == 2 + 3 + 2 + 3)
    bufs = dict(model.netD.named_buffers())
    for k in FULL_BUFS:
        res['rm_' + k] = npy(bufs[k + '.running_mean'])
        res['rv_' + k] = npy(bufs[k + '.running_var'])
    return res


def gen_srgan_step_srresnet():
    print('[gen_srgan_step_golden] SRGANModel, which_model_G sr_resnet')
    model = _create(_opt('vanilla', which='sr_resnet'))
    sdG = synth.srresnet_state_dict(nb=NB, seed=34, upsample_mode='pixelshuffle')
    sdD = synth.discriminator_state_dict(seed=35)
    model.netG.load_state_dict(sdG, strict=True)
    model.netD.load_state_dict(sdD, strict=True)
    lr = synth.image_batch(36, 4, 3, 32, 32, name='srgan_srresnet.lr')
    hr = synth.image_batch(36, 4, 3, 128, 128, name='srgan_srresnet.hr')
    model.feed_data({'LR': lr, 'HR': hr})
    model.optimize_parameters(1)
    res = _results(model, sdG, sdD, 'model.0.weight', 'classifier.2.weight')
    res['seeds'] = np.array([34, 35, 36, 36], dtype=np.int64)
    res['names'] = np.array(['srgan_srresnet.lr', 'srgan_srresnet.hr'])
    res['nb'] = np.int64(NB)
    return res


def write(name, res):
    path = os.path.join(ROOT, 'tests', 'golden', name)
    if os.path.exists(path):
        old = dict(np.load(path))
        assert set(old) == set(res), sorted(set(old) ^ set(res))
        diff = max(float(np.abs(old[k].astype(np.float64) - np.asarray(res[k], dtype=np.float64)).max())
                   if old[k].dtype.kind in 'fiu' else float(not np.array_equal(old[k], res[k])) for k in res)
        print('  %s: max difference to the existing file %.1e' % (name, diff))
    np.savez_compressed(path, **res)
    print('done ->', path, os.path.getsize(path), 'bytes')


def main():
    assert RI.available(), 'the reference checkout is needed (ESRGAN_REFERENCE)'
    torch.set_grad_enabled(True)
    write('srgan_step.npz', gen_srgan_step())
    write('srgan_steps4.npz', gen_srgan_steps4())
    write('srgan_step_srresnet.npz', gen_srgan_step_srresnet())


if __name__ == '__main__':
    main()
