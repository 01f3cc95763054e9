#!/usr/bin/env python
"""The reference's test script (``codes/test.py:49-110``) on the HIP path, with PIL instead of cv2:

    python tools/sr_eval.py <model.pth|synthetic> <lr_dir> <hr_dir> [fp16|fp32] [--tile-u8 N[,PAD]] [--x8] [--save out_dir]
    python tools/sr_eval.py <model.pth|synthetic> <hr_dir> [fp16|fp32] [--tile-u8 N[,PAD]] [--save out_dir]

The LR and HR images are paired by sorted base name (HR = 4 x LR; x4 only).  Images are queued as ``sr_infer.py
--tile-u8`` queues them — until they hold at least 4 x 16 windows, or the folder ends — and every queue runs through
``model.evaluate_images(lr, hr, tile=N, pad=PAD)``: the 8-bit tiled forward over the set, then PSNR, SSIM, PSNR_Y and
SSIM_Y of every result against its ground truth in one device pass, cropped by the scale; four doubles per image come
back.  --tile-u8 defaults to 96,16.  Prints one line per image and the two average blocks in the reference's formats.
--x8: the score of the x8 self-ensemble per window (the reference's ``test_x8``), ``evaluate_images(..., x8=True)``.
--save out_dir: the results are written there as ``<name>.png``.
With an HR folder alone (the reference's ``dataroot_LR: null``) every queue runs through
``model.evaluate_hr_images(hr, tile=N, pad=PAD)``: the LR is the dataset's — modcrop, the bicubic resample of the float
image by 1 / 4, not rounded to 8 bits — made inside the gather, and the results are scored against the modcropped HR
images.  The numbers differ from those of stored 8-bit LR files; --x8 is not offered on this route.
--nb N: the number of RRDBs of the model (default 23)."""
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from PIL import Image

from esrganplus_amd import architecture as arch, synth


def _option(argv, flag):
    """Removes ``flag VALUE`` / ``flag=VALUE`` from argv -> VALUE or None."""
    for i, a in enumerate(argv):
        if a == flag or a.startswith(flag + '='):
            val = a[len(flag) + 1:] if '=' in a else ''.join(argv[i + 1:i + 2])
            del argv[i:i + (1 if '=' in a else 2)]
            return val
    return None


def paired_files(lr_dir, hr_dir):
    """[(base name, lr path, hr path)] by sorted base name; both folders must hold the same names."""
    def names(d):
        return {os.path.splitext(os.path.basename(p))[0]: p for p in sorted(glob.glob(os.path.join(d, '*'))) if os.path.isfile(p)}
    lr, hr = names(lr_dir), names(hr_dir)
    if not lr:
        sys.exit('sr_eval.py: no files in %s' % lr_dir)
    if sorted(lr) != sorted(hr):
        sys.exit('sr_eval.py: %s and %s do not hold the same base names: %s' % (lr_dir, hr_dir, sorted(set(lr) ^ set(hr))[:5]))
    return [(k, lr[k], hr[k]) for k in sorted(lr)]


def main():
    argv = [a for a in sys.argv[1:] if a != '--x8']
    x8 = '--x8' in sys.argv[1:]
    val = _option(argv, '--tile-u8')
    try:
        tiling = [int(v) for v in val.split(',')] if val is not None else [96, 16]
    except ValueError:
        tiling = []
    if len(tiling) not in (1, 2):
        sys.exit('sr_eval.py: --tile-u8 takes N or N,PAD (LR pixels), got %r' % val)
    tile, pad = tiling[0], (tiling[1] if len(tiling) == 2 else 16)
    save = _option(argv, '--save')
    nb = _option(argv, '--nb')
    try:
        nb = 23 if nb is None else int(nb)
    except ValueError:
        sys.exit('sr_eval.py: --nb takes an int, got %r' % nb)
    if len(argv) < 2:
        sys.exit(__doc__)
    hr_only = len(argv) == 2 or argv[2] in ('fp16', 'fp32')              # no lr_dir: an HR folder alone
    if hr_only:
        model_path, hr_dir = argv[:2]
        prec = argv[2] if len(argv) > 2 else 'fp32'
        if x8:
            sys.exit('sr_eval.py: --x8 is not offered with an HR folder alone')
        files = paired_files(hr_dir, hr_dir)
    else:
        model_path, lr_dir, hr_dir = argv[:3]
        prec = argv[3] if len(argv) > 3 else 'fp32'
        files = paired_files(lr_dir, hr_dir)
    dev = torch.device('cuda')
    model = arch.RRDB_Net(3, 3, 64, nb, gc=32, upscale=4, norm_type=None, act_type='leakyrelu',
                          mode='CNA', res_scale=1, upsample_mode='upconv')
    sd = synth.rrdbnet_state_dict(nb, 0) if model_path == 'synthetic' else torch.load(model_path, map_location='cpu')
    model.load_state_dict(sd, strict=False)
    model.eval()
    for _, v in model.named_parameters():
        v.requires_grad = False
    model = model.to(dev).set_precision(prec)
    if save:
        os.makedirs(save, exist_ok=True)
    rows, queue, windows = [], [], 0

    def flush():
        try:
            with torch.no_grad():
                if hr_only:
                    sr, res = model.evaluate_hr_images([q[2] for q in queue], tile, pad)
                else:
                    sr, res = model.evaluate_images([q[1] for q in queue], [q[2] for q in queue], tile, pad, x8=x8)
        except ValueError as e:
            sys.exit('sr_eval.py: %s' % e)
        for (name, _, _), img, (psnr, ssim, psnr_y, ssim_y) in zip(queue, sr, res.read()):
            if save:
                Image.fromarray(img.cpu().numpy()).save(os.path.join(save, name + '.png'))
            print('{:20s} - PSNR: {:.6f} dB; SSIM: {:.6f}; PSNR_Y: {:.6f} dB; SSIM_Y: {:.6f}.'
                  .format(name, psnr, ssim, psnr_y, ssim_y), flush=True)
            rows.append((psnr, ssim, psnr_y, ssim_y))
        del queue[:]

    for name, lr_path, hr_path in files:
        hr = torch.from_numpy(np.array(Image.open(hr_path).convert('RGB'))).to(dev)
        lr = None if hr_only else torch.from_numpy(np.array(Image.open(lr_path).convert('RGB'))).to(dev)
        queue.append((name, lr, hr))
        lh, lw = (hr.shape[0] // 4, hr.shape[1] // 4) if hr_only else lr.shape[:2]
        windows += -(-lh // max(tile, 1)) * -(-lw // max(tile, 1))
        if windows >= 4 * 16:
            flush()
            windows = 0
    if queue:
        flush()
    ave = [sum(float(r[k]) for r in rows) / len(rows) for k in range(4)]
    set_name = os.path.basename(os.path.normpath(hr_dir))
    print('----Average PSNR/SSIM results for {}----\n\tPSNR: {:.6f} dB; SSIM: {:.6f}\n'.format(set_name, ave[0], ave[1]))
    print('----Y channel, average PSNR/SSIM----\n\tPSNR_Y: {:.6f} dB; SSIM_Y: {:.6f}\n'.format(ave[2], ave[3]))


if __name__ == '__main__':
    main()
