#!/usr/bin/env python
"""Pins RRDBNet / RRDB_Net at the scales other than 4 against the reference's own modules: writes
tests/golden/rrdbnet_scales.npz (state-dict key lists with shapes and eval outputs) and, one file per scale so that each
stays under the size limit for committed files, tests/golden/rrdbnet_scales_x<s>_train.npz (one train-mode case: output,
input gradient, full gradients of the tail convs, checksums of every gradient).  Needs the reference checkout
(oracle.ref_import), CPU only:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_scales_golden.py

The recipe is oracle/gen_golden.py's for rrdbnet_small.npz: weights, inputs, upstream gradients and the training noise
are regenerated from the recorded seeds and names (esrganplus_amd.synth; the noise is injected into the reference's
``normal_()`` draws), so the files hold key lists, seeds, names, shapes and results only.  Each train case records the
image seed it took: the first from X_SEED up that leaves no LeakyReLU input within fp32 rounding of 0 (``lrelu_margins``)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from esrganplus_amd import synth
from oracle import ref_import as RI
from oracle import ref_torch as RT
from oracle.gen_golden import checks, draw_z, inject_z, npy

SCALES = (1, 2, 3, 8)
NB, SD_SEED, X_SEED, Z_SEED = 1, 0, 5, 9
EVAL_SHAPE = (1, 3, 16, 20)
# x8 adds a third up-conv to the default-gain net and its output for a U[0, 1) image peaks at 0.015: the 1e-3 gate of the
# tests would be vacuous.  The x8 eval input is the same image times 16 (output peak 0.24, as the other scales').
EVAL_GAIN = {1: 1.0, 2: 1.0, 3: 1.0, 8: 16.0}
TRAIN_SHAPE = {1: (2, 3, 12, 12), 2: (2, 3, 12, 12), 3: (2, 3, 12, 12), 8: (1, 3, 8, 12)}    # x8: the outputs are 64 x the input
U32 = 2.0 ** -24


class lrelu_margins:
    """Conditioning guard of a train case.  LeakyReLU's derivative jumps at 0, so where a pre-activation lies within fp32
    rounding of 0 two correct fp32 implementations that sum in different orders may take different slopes, and every
    gradient upstream then differs by 0.8 x that element's share (the x8 case has 1.3 M such elements over a 96-pixel
    image: one flip moves the tail gradients by 3e-3 of their peak).  Such a case measures the summation order, not the
    code.  Recorded per LeakyReLU of the reference net: min |input| and the margin sqrt(K) 2^-24 median |input|, the
    standard deviation of the rounding error of a K-term fp32 dot product (K = 9 x 64 taps of the narrowest conv that
    feeds one) whose terms are of the output's own size.  ``ok`` asks every min to exceed its margin."""
    K = 9 * 64

    def __init__(self, net):
        self.net, self.rows, self.hooks = net, [], []

    def __enter__(self):
        for m in self.net.modules():
            if isinstance(m, torch.nn.LeakyReLU):
                self.hooks.append(m.register_forward_pre_hook(self._see))
        return self

    def _see(self, _m, args):
        a = args[0].detach().abs()
        self.rows.append((float(a.min()), float(np.sqrt(self.K) * U32 * a.median()), a.numel()))

    def __exit__(self, *exc):
        for h in self.hooks:
            h.remove()

    def ok(self):
        return all(lo > margin for lo, margin, _ in self.rows)


def train_inputs(s, x_seed):
    shape = TRAIN_SHAPE[s]
    x = synth.image_batch(x_seed, *shape, name='scales.x.train')
    gy = synth.normal_like(x_seed, 'scales.gy.x%d' % s, (shape[0], 3, s * shape[2], s * shape[3]))
    return x, gy, draw_z(Z_SEED, RT.noise_shapes(shape, NB, 'codes'), 'scales.z')


def well_conditioned_seed(net, s):
    """The first image seed from X_SEED up whose train case passes ``lrelu_margins``."""
    for x_seed in range(X_SEED, X_SEED + 64):
        x, _, z = train_inputs(s, x_seed)
        with torch.no_grad(), lrelu_margins(net) as guard, inject_z(z):
            net(x)
        lo, margin, _ = min(guard.rows, key=lambda r: r[0] / r[1])
        print('   x%d train seed %d: tightest LeakyReLU input %.3e against a margin of %.3e -> %s'
              % (s, x_seed, lo, margin, 'ok' if guard.ok() else 'refused'))
        if guard.ok():
            return x_seed
    raise RuntimeError('no well-conditioned x%d train case in 64 seeds' % s)


def build(variant, upscale):
    with RI.cuda_to_cpu():
        if variant == 'codes':
            arch, _ = RI.codes_arch()
            return arch.RRDBNet(3, 3, 64, NB, gc=32, upscale=upscale, norm_type=None, act_type='leakyrelu', mode='CNA',
                                upsample_mode='upconv')
        arch, _ = RI.test_image_arch()
        return arch.RRDB_Net(3, 3, 64, NB, gc=32, upscale=upscale, norm_type=None, act_type='leakyrelu', mode='CNA',
                             res_scale=1, upsample_mode='upconv')


def key_list(net):
    sd = net.state_dict()
    shapes = np.full((len(sd), 4), -1, dtype=np.int64)
    for i, v in enumerate(sd.values()):
        shapes[i, :v.dim()] = list(v.shape)
    return np.array(list(sd.keys())), shapes


def tail_keys(keys):
    """model.0, LR_conv, every up-conv, HR_conv0, HR_conv1: every parameter outside the dense blocks."""
    return [k for k in keys if 'RDB' not in k]


def main():
    assert RI.available(), 'the reference checkout is needed (ESRGAN_REFERENCE)'
    torch.set_grad_enabled(True)
    gold = os.path.join(ROOT, 'tests', 'golden')
    res = {'scales': np.array(SCALES, dtype=np.int64), 'nb': np.int64(NB),
           'seeds': np.array([SD_SEED, X_SEED, Z_SEED], dtype=np.int64), 'eval_shape': np.array(EVAL_SHAPE, dtype=np.int64)}
    for s in SCALES:
        tag = 'x%d' % s
        net = build('codes', s)
        res[tag + '_keys'], res[tag + '_shapes'] = key_list(net)
        sd = synth.rrdbnet_state_dict(NB, SD_SEED, upscale=s)
        assert list(sd.keys()) == [str(k) for k in res[tag + '_keys']], 'synth.rrdbnet_keys disagrees with the reference'
        net.load_state_dict(sd, strict=True)
        net.eval()
        with torch.no_grad():
            y = net(synth.image_batch(X_SEED, *EVAL_SHAPE, name='scales.x.eval') * EVAL_GAIN[s])
        assert float(y.abs().max()) > 0.1
        res[tag + '_eval_gain'] = np.float64(EVAL_GAIN[s])
        assert tuple(y.shape) == (1, 3, s * EVAL_SHAPE[2], s * EVAL_SHAPE[3])
        res[tag + '_y_eval'] = npy(y)
        print('[gen_scales_golden] %s eval %s -> %s  |y| max %.3f' % (tag, EVAL_SHAPE, tuple(y.shape), float(y.abs().max())))
        # one train-mode case
        shape = TRAIN_SHAPE[s]
        net.train()
        net.zero_grad()
        x_seed = well_conditioned_seed(net, s)
        x, gy, z = train_inputs(s, x_seed)
        x.requires_grad_(True)
        with inject_z(z):
            yt = net(x)
        (yt * gy).sum().backward()
        grads = {k: p.grad for k, p in net.named_parameters()}
        tr = {'shape': np.array(shape, dtype=np.int64), 'x_seed': np.int64(x_seed), 'y': npy(yt), 'gx': npy(x.grad),
              'gchk': np.stack([checks(grads[k]) for k in sd.keys()])}
        for k in tail_keys(sd.keys()):
            tr['g_' + k] = npy(grads[k])
        path = os.path.join(gold, 'rrdbnet_scales_%s_train.npz' % tag)
        np.savez_compressed(path, **tr)
        print('   train %s -> %s, %d tail gradients; %s %d bytes' % (shape, tuple(yt.shape), len(tail_keys(sd.keys())),
                                                                     os.path.basename(path), os.path.getsize(path)))
    # the inference copy (test_image/architecture.py) at x3: keys and the eval output
    net = build('test_image', 3)
    res['ti3_keys'], res['ti3_shapes'] = key_list(net)
    net.load_state_dict(synth.rrdbnet_state_dict(NB, SD_SEED, upscale=3), strict=True)
    net.eval()
    with torch.no_grad():
        res['ti3_y_eval'] = npy(net(synth.image_batch(X_SEED, *EVAL_SHAPE, name='scales.x.eval')))
    path = os.path.join(gold, 'rrdbnet_scales.npz')
    np.savez_compressed(path, **res)
    print('done ->', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
