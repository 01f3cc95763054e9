#!/usr/bin/env python
"""Pins ``train.PSNRStep`` and the 'l2' criteria of ``train.ESRGANPlusStep`` against the reference's own models: writes
tests/golden/psnr_steps3.npz and tests/golden/train_step_l2.npz.  Needs the reference checkout (oracle.ref_import), CPU only:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_psnr_step_golden.py [--scale S]

--scale S (default 4; 1, 2, 3 or 8): the ``SRModel`` run with ``scale: S`` in its options (HR = S x LR) instead, written
to tests/golden/psnr_steps3_x<S>.npz alone; without the option the two files below are written exactly as before.

psnr_steps3.npz — the real ``SRModel`` (codes/models/SR_model.py, built by ``models.create_model({'model': 'sr'})``),
three iterations of the loop body of codes/train.py:97-106 (``update_learning_rate()`` BEFORE ``optimize_parameters``)
at nb = 2, batch 4 of 20 x 28 LR, MultiStepLR([1, 2], 0.5), lr_G 2e-4, fresh data and noise per iteration, for the
cases of ``CASES``.  Adam hides the criterion (the three-step deltas of l1 and l2 differ by ~1 %), so what pins l2 are the
logged losses and the gradients after iteration 1; the weight-decay case is asserted to move every stored delta.
train_step_l2.npz — one ``SRRaGANModel.optimize_parameters`` step set up as oracle/gen_golden.py: gen_train_step, with
pixel_criterion and feature_criterion 'l2'.
Weights, inputs and noise are regenerated from the recorded seeds and names (esrganplus_amd.synth): the files hold seeds,
names, shapes and results only.  An existing file is compared with what was generated (max difference printed)."""
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

# (tag, pixel_criterion, weight_decay_G)
CASES = (('l1_wd0', 'l1', 0.0), ('l2_wd0', 'l2', 0.0), ('l2_wd1e-2', 'l2', 1e-2))
NB, SD_SEED, LR_G, STEPS, GAMMA = 2, 32, 2e-4, (1, 2), 0.5
LR_SHAPE, HR_SHAPE = (4, 3, 20, 28), (4, 3, 80, 112)
LR_SEED, HR_SEED, Z_SEED = 70, 80, 90               # + iteration (1..3)
LR_NAME, HR_NAME, Z_NAME = 'psnr.lr', 'psnr.hr', 'psnr.z'
FULL_GRADS = ('model.0.weight', 'model.1.sub.1.RDB2.conv3.0.bias')
FULL_DELTAS = FULL_GRADS + ('model.1.sub.0.RDB1.conv1.0.weight',)          # the last: a 32-cout dense conv


SCALE = 4


def _network_G():
    return {'which_model_G': 'RRDB_net', 'norm_type': None, 'mode': 'CNA', 'nf': 64, 'nb': NB, 'in_nc': 3,
            'out_nc': 3, 'gc': 32, 'scale': SCALE}


def _create(opt):
    sys.modules.setdefault('cv2', types.ModuleType('cv2'))
    RI.codes_arch()
    from models import create_model
    with RI.cuda_to_cpu():
        return create_model(opt)


def psnr_case(criterion, wd):
    opt = {'model': 'sr', 'scale': SCALE, 'gpu_ids': None, 'is_train': True, 'path': {'pretrain_model_G': None},
           'network_G': _network_G(),
           'train': {'lr_G': LR_G, 'weight_decay_G': wd, 'lr_scheme': 'MultiStepLR', 'lr_steps': list(STEPS),
                     'lr_gamma': GAMMA, 'pixel_criterion': criterion, 'pixel_weight': 1.0}}
    model = _create(opt)
    sd = synth.rrdbnet_state_dict(nb=NB, seed=SD_SEED, upscale=SCALE)
    model.netG.load_state_dict(sd, strict=True)
    g = dict(model.netG.named_parameters())
    res = {}
    for it in range(1, 4):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')          # "lr_scheduler.step() before optimizer.step()": the reference's order
            model.update_learning_rate()
        lr = synth.image_batch(LR_SEED + it, *LR_SHAPE, name=LR_NAME)
        hr = synth.image_batch(HR_SEED + it, *HR_SHAPE, name=HR_NAME)
        model.feed_data({'LR': lr, 'HR': hr})
        with inject_z(draw_z(Z_SEED + it, RT.noise_shapes(lr.shape, NB, 'codes'), Z_NAME)):
            model.optimize_parameters(it)
        res['lr_%d' % it] = np.array(model.optimizer_G.param_groups[0]['lr'])
        res['l_pix_%d' % it] = np.array(float(model.get_current_log()['l_pix']))
        res['fake_H_chk_%d' % it] = checks(model.fake_H)
        print('  iteration %d  lr %.3e  l_pix %.6f' % (it, res['lr_%d' % it], res['l_pix_%d' % it]))
        if it == 1:
            res['grad_chk'] = np.stack([checks(g[k].grad) for k in sd.keys()])
            for k in FULL_GRADS:
                res['grad_' + k] = npy(g[k].grad).copy()
            res['delta1_model.0.weight'] = npy(g['model.0.weight'] - sd['model.0.weight'])
    res['G_chk'] = np.stack([checks(g[k]) for k in sd.keys()])
    for k in FULL_DELTAS:
        res['delta_' + k] = npy(g[k] - sd[k])
    return res


def gen_psnr_steps3():
    out = {'cases': np.array([c[0] for c in CASES]), 'criteria': np.array([c[1] for c in CASES]),
           'weight_decay': np.array([c[2] for c in CASES]), 'nb': np.int64(NB), 'sd_seed': np.int64(SD_SEED),
           'lr_G': np.float64(LR_G), 'lr_steps': np.array(STEPS, dtype=np.int64), 'lr_gamma': np.float64(GAMMA),
           'lr_shape': np.array(LR_SHAPE, dtype=np.int64), 'hr_shape': np.array(HR_SHAPE, dtype=np.int64),
           'seeds': np.array([LR_SEED, HR_SEED, Z_SEED], dtype=np.int64), 'names': np.array([LR_NAME, HR_NAME, Z_NAME]),
           'param_keys': np.array(list(synth.rrdbnet_state_dict(nb=NB, seed=SD_SEED, upscale=SCALE).keys()))}
    per = {}
    for tag, criterion, wd in CASES:
        print('[gen_psnr_step_golden] SRModel', tag)
        per[tag] = psnr_case(criterion, wd)
        out.update({tag + '.' + k: v for k, v in per[tag].items()})
    for k in FULL_DELTAS:
        d0, d1 = per['l2_wd0']['delta_' + k], per['l2_wd1e-2']['delta_' + k]
        moved = np.abs(d1 - d0).mean() / np.abs(d0).mean()
        print('  weight decay 1e-2 moves delta %-40s by %.3f of its mean magnitude' % (k, moved))
        # else the wd case would pin nothing the wd 0 case does not.  Other scales: twice the 0.08 the tests allow a
        # delta (a shorter tail moves model.0.weight less: 0.21 at x2)
        assert moved >= (0.3 if SCALE == 4 else 0.16), (k, moved)
    return out


def gen_train_step_l2():
    install_vgg_stub(6)
    opt = {'model': 'srragan', 'scale': 4, 'gpu_ids': None, 'is_train': True,
           'path': {'pretrain_model_G': None, 'pretrain_model_D': None},
           'network_G': _network_G(),
           'network_D': {'which_model_D': 'discriminator_vgg_128', 'norm_type': 'batch',
                         'act_type': 'leakyrelu', 'mode': 'CNA', 'nf': 64, 'in_nc': 3},
           'train': {'lr_G': 1e-4, 'weight_decay_G': 0, 'beta1_G': 0.9, 'lr_D': 1e-4,
                     'weight_decay_D': 0, 'beta1_D': 0.9, 'lr_scheme': 'MultiStepLR',
                     'lr_steps': [50000, 100000, 200000, 300000], 'lr_gamma': 0.5,
                     'pixel_criterion': 'l2', 'pixel_weight': 0.01, 'feature_criterion': 'l2',
                     'feature_weight': 1, 'gan_type': 'vanilla', 'gan_weight': 0.005,
                     'D_update_ratio': None, 'D_init_iters': None}}
    print('[gen_psnr_step_golden] SRRaGANModel, pixel / feature criterion l2')
    model = _create(opt)
    sdG = synth.rrdbnet_state_dict(nb=2, seed=30)
    sdD = synth.discriminator_state_dict(seed=31)
    model.netG.load_state_dict(sdG, strict=True)
    model.netD.load_state_dict(sdD, strict=True)
    lr = synth.image_batch(30, 4, 3, 32, 32, name='step.lr')
    hr = synth.image_batch(30, 4, 3, 128, 128, name='step.hr')
    model.feed_data({'LR': lr, 'HR': hr})
    with inject_z(draw_z(9, RT.noise_shapes(lr.shape, 2, 'codes'), 'step.z')):
        model.optimize_parameters(1)
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
    res['G_delta_model.0.weight'] = npy(g['model.0.weight'] - sdG['model.0.weight'])
    res['D_delta_classifier.2.weight'] = npy(d['classifier.2.weight'] - sdD['classifier.2.weight'])
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
    global SCALE, HR_SHAPE
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument('--scale', type=int, default=4, choices=(1, 2, 3, 4, 8))
    SCALE = ap.parse_args().scale
    assert RI.available(), 'the reference checkout is needed (ESRGAN_REFERENCE)'
    torch.set_grad_enabled(True)
    if SCALE != 4:
        HR_SHAPE = LR_SHAPE[:2] + (SCALE * LR_SHAPE[2], SCALE * LR_SHAPE[3])
        out = gen_psnr_steps3()
        out['scale'] = np.int64(SCALE)
        write('psnr_steps3_x%d.npz' % SCALE, out)
        return
    write('psnr_steps3.npz', gen_psnr_steps3())
    write('train_step_l2.npz', gen_train_step_l2())


if __name__ == '__main__':
    main()
