#!/usr/bin/env python
"""PSNR-oriented pretraining from a folder of PNGs, fed by the device-resident training set (``data.TrainSet``: the
decoded uint8 images stay on the device and every batch is one launch):

    python tools/train_folder.py HR_DIR [--lr-dir DIR] [--scale S] [--lr-size N] [--batch B] [--iters N] [--nb N]
                                 [--precision fp16|fp32] [--seed K] [--out DIR] [--val LR_DIR HR_DIR | --val-hr HR_DIR] [--val-freq N]
                                 [--val-x8]

HR_DIR: the HR images (sizes may differ; each is cut to a multiple of the scale with ``data.modcrop``, as the reference
does for validation images — without --lr-dir the LR windows are resampled from them on the fly).  --lr-dir: the LR
images, paired with the HR ones by sorted name (HR = scale x LR).  The generator is an ``RRDBNet`` with synthetic weights
(as ``sr_infer.py synthetic``), trained by a ``PSNRStep`` (l1) for --iters iterations over ``TrainSet.epoch``.  Prints
the loss of every iteration and a last line ``iters N, last loss X``.  --out DIR: the generator's state dict is saved
there as ``G_iters<N>.pth``; nothing else is written, nothing is downloaded.  --val LR_DIR HR_DIR: a validation set, paired
by sorted name (HR = 4 x LR; x4 only), scored every --val-freq iterations (default 100) with ``PSNRStep.validate`` — the
validation pass of the reference's train loop, one device pass — and printed as the reference logs it:
``# Validation # PSNR: 2.3456e+01``.  --val-hr HR_DIR: a validation set of ground-truth images alone (the reference's
``dataroot_LR: null``), scored with ``PSNRStep.validate_hr``: the LR is made from the HR images inside the gather, not
rounded to 8 bits; x4 only, no --val-x8."""
import argparse
import glob
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from PIL import Image

from esrganplus_amd import architecture as arch, data as D, synth, train


def read_dir(path):
    files = sorted(glob.glob(os.path.join(path, '*.png')) + glob.glob(os.path.join(path, '*.PNG')))
    if not files:
        sys.exit('train_folder.py: no PNG files in %s' % path)
    return [np.array(Image.open(f).convert('RGB')) for f in files]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('hr_dir')
    ap.add_argument('--lr-dir')
    ap.add_argument('--scale', type=int, default=4, choices=D.SCALES)
    ap.add_argument('--lr-size', type=int, default=32)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--nb', type=int, default=23)
    ap.add_argument('--precision', default='fp16', choices=('fp16', 'fp32'))
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out')
    ap.add_argument('--val', nargs=2, metavar=('LR_DIR', 'HR_DIR'))
    ap.add_argument('--val-hr', metavar='HR_DIR', help='validate from ground-truth images alone: validate_hr(...)')
    ap.add_argument('--val-freq', type=int, default=100)
    ap.add_argument('--val-x8', action='store_true', help='score the x8 self-ensemble: validate(..., x8=True)')
    a = ap.parse_args()
    if a.val and a.val_hr:
        sys.exit('train_folder.py: --val and --val-hr are two ways to validate: give one')
    if a.val_hr and a.val_x8:
        sys.exit('train_folder.py: --val-x8 is not offered with --val-hr')
    random.seed(a.seed)
    torch.manual_seed(a.seed)
    hr = read_dir(a.hr_dir)
    lr = read_dir(a.lr_dir) if a.lr_dir else None
    if lr is None:
        hr = [D.modcrop(im, a.scale) for im in hr]
    try:
        ts = D.TrainSet(hr, lr, scale=a.scale, lr_size=a.lr_size)
    except ValueError as e:
        sys.exit('train_folder.py: %s' % e)
    if len(ts) < a.batch:
        sys.exit('train_folder.py: %d images are fewer than one batch of %d' % (len(ts), a.batch))
    print('%d images, %.1f MB on the device, LR %s' % (len(ts), ts.pool_bytes / 1e6, 'given' if lr else 'generated'))
    dev = ts.device
    netG = arch.RRDBNet(3, 3, 64, a.nb, upscale=a.scale).to(dev).train().set_precision(a.precision)
    netG.load_state_dict(synth.rrdbnet_state_dict(nb=a.nb, seed=a.seed, upscale=a.scale), strict=True)
    step = train.PSNRStep(netG, loss_scale='dynamic' if a.precision == 'fp16' else 1.0)
    val = None
    if a.val or a.val_hr:
        if a.val_freq < 1:
            sys.exit('train_folder.py: --val-freq takes an int >= 1, got %d' % a.val_freq)
        val = [[torch.from_numpy(im).to(dev) for im in read_dir(d)] for d in (a.val or [a.val_hr])]
    it, loss = 0, float('nan')
    while it < a.iters:
        for var_L, real_H in ts.epoch(a.batch):
            it += 1
            loss = step.step(var_L, real_H)['l_pix']
            print('iter %d  l_pix %.6f' % (it, loss), flush=True)
            if val and it % a.val_freq == 0:
                try:
                    psnr = step.validate_hr(val[0]) if a.val_hr else step.validate(*val, x8=a.val_x8)
                    print('# Validation # PSNR: {:.4e}'.format(psnr), flush=True)
                except ValueError as e:
                    sys.exit('train_folder.py: %s: %s' % ('--val-hr' if a.val_hr else '--val', e))
            if it == a.iters:
                break
    step.finish()
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        torch.save(netG.state_dict(), os.path.join(a.out, 'G_iters%d.pth' % a.iters))
    print('iters %d, last loss %.6f' % (a.iters, loss))


if __name__ == '__main__':
    main()
