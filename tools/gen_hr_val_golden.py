#!/usr/bin/env python
"""Pins ``functional.hr_lr_reference`` — and through it ``forward_hr_images`` — against the reference's own
``LRHRDataset.__getitem__`` (codes/data/LRHR_dataset.py:44-125) in the HR-only validation configuration: phase 'val',
``dataroot_LR: None``, scale 4.  Writes tests/golden/hr_val.npz.  Needs the reference checkout (oracle.ref_import), CPU
only:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_hr_val_golden.py

The dataset class runs as it stands on in-memory images, over the ``cv2`` stand-in of tools/gen_batch_golden.py (its
``resize`` only knows the identity; in this phase the dataset never asks for it).  Three small BGR uint8 images: 55 x 86
(both sides are cut by modcrop), 52 x 240 (a wide LR of 13 x 60) and 64 x 64.  Stored: the images and the dataset's
``LR`` and ``HR`` tensors (float32 CHW, RGB), data only.  What is generated is compared with ``hr_lr_reference`` before
it is written: HR bit for bit, LR within 2e-6."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np
import torch

import gen_batch_golden as GB
from esrganplus_amd import functional as F
from oracle import ref_import as RI

SIZES = ((55, 86), (52, 240), (64, 64))                 # H x W
IMG_SEED = 5200


def images():
    """gen_batch_golden's pictures at these sizes: smooth colour gradients under uniform noise."""
    out = []
    for k, (h, w) in enumerate(SIZES):
        rs = np.random.RandomState(IMG_SEED + k)
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        base = np.stack([40 + 150 * yy / h, 30 + 170 * xx / w, 60 + 60 * (yy / h) * (xx / w) + 50 * np.sin(xx / 5.0)], axis=2)
        out.append(np.clip(base + rs.uniform(-30, 30, size=(h, w, 3)), 0, 255).round().astype(np.uint8))
    return out


def main():
    assert RI.available(), 'the reference checkout is needed (ESRGAN_REFERENCE)'
    imgs = images()
    store = {'HR/%02d' % k: im for k, im in enumerate(imgs)}
    LRHRDataset = GB.dataset_class(store)
    ds = LRHRDataset({'phase': 'val', 'scale': 4, 'HR_size': None, 'subset_file': None, 'data_type': 'img',
                      'dataroot_HR': 'HR', 'dataroot_LR': None, 'color': None, 'use_flip': False, 'use_rot': False})
    assert len(ds) == len(imgs)
    res = {'n_images': np.int64(len(imgs))}
    lrs, hrs = F.hr_lr_reference([torch.from_numpy(im) for im in imgs], bgr=True)
    for k, im in enumerate(imgs):
        item = ds[k]
        lr, hr = item['LR'].numpy().astype(np.float32), item['HR'].numpy().astype(np.float32)
        h, w = im.shape[0] - im.shape[0] % 4, im.shape[1] - im.shape[1] % 4
        assert hr.shape == (3, h, w) and lr.shape == (3, h // 4, w // 4), (hr.shape, lr.shape)
        res['img%d' % k], res['LR%d' % k], res['HR%d' % k] = im, lr, hr
        dl = float(np.abs(lrs[k].numpy() - lr).max())
        assert np.array_equal(hrs[k].numpy(), hr), k
        assert dl <= 2e-6, (k, dl)
        print('[gen_hr_val_golden] image %d %s: HR equal, LR %s max difference %.2e, LR range [%.4f, %.4f]'
              % (k, im.shape, lr.shape, dl, lr.min(), lr.max()))
    out = os.path.join(ROOT, 'tests', 'golden', 'hr_val.npz')
    np.savez_compressed(out, **res)
    print('done ->', out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
