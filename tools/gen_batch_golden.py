#!/usr/bin/env python
"""Pins ``data.batch_reference`` — and through it ``data.TrainSet.batch`` — against the reference's own
``LRHRDataset.__getitem__`` (codes/data/LRHR_dataset.py:44-125, phase 'train'): writes tests/golden/batch_assemble.npz.
Needs the reference checkout (oracle.ref_import), CPU only:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_batch_golden.py

The dataset class runs as it stands, on in-memory images: ``data.util.get_image_paths`` is replaced by one that returns
the images' names, and the ``cv2`` module the reference imports is a stand-in with two entry points —

  * ``imread(name, flag)`` hands out the uint8 array of that name, so that the reference's own ``read_img``
    (util.py:72-85: the float32 conversion, the 4-channel cut) runs on it;
  * ``resize(img, (w, h), interpolation)`` ASSERTS that the requested size is the image's and returns the image:
    identity at equal size is assumed of OpenCV, and the assertion keeps the fixture from ever resting on more than
    that (the images are multiples of 12, so at scales 2, 3 and 4 the dataset asks for no other size).

Per scale (2, 3, 4) and mode ('given': LR images are stored; 'gen': ``dataroot_LR`` is None and the dataset makes LR
with its ``imresize_np``) the file holds B = 6 items: Python's ``random`` is seeded with a recorded seed before each
``__getitem__``, and the window / flips the item drew are recovered by re-seeding and drawing in the dataset's order
(``random.choice`` of the random-scale list first in 'gen' mode, LRHR_dataset.py:66; then randint, randint and
util.augment's three coins).  Stored: the uint8 images (cv2's channel order, i.e. BGR), the item indices, the seeds, the
recovered draws and the returned ``LR`` / ``HR`` tensors.  The LR images of 'given' mode are ``hr[::scale, ::scale]``
(any image of the right size would do; they are not stored).  What is generated is compared with
``data.batch_reference`` before it is written: HR and given LR bit for bit, generated LR within 2e-6."""
import importlib
import os
import random
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from esrganplus_amd import data as D
from oracle import ref_import as RI

SIZES = ((36, 48), (48, 36), (60, 72), (96, 84))       # H x W: multiples of 12, all different, under 100 x 100
IMG_SEED = 4100
INDICES = (0, 1, 2, 3, 1, 2)
SCALES = (2, 3, 4)
LR_SIZE = 8
SEED0 = 700                                             # item b of (scale, mode) is drawn under SEED0 + 100 scale + 10 gen + b


def images():
    """Smooth colour gradients under uniform noise, uint8: every pixel differs from its neighbours and from its
    mirror images, so a wrong window, flip or channel order cannot pass."""
    out = []
    for k, (h, w) in enumerate(SIZES):
        rs = np.random.RandomState(IMG_SEED + k)
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        base = np.stack([40 + 150 * yy / h, 30 + 170 * xx / w, 60 + 60 * (yy / h) * (xx / w) + 50 * np.sin(xx / 5.0)], axis=2)
        out.append(np.clip(base + rs.uniform(-30, 30, size=(h, w, 3)), 0, 255).round().astype(np.uint8))
    return out


def dataset_class(store):
    for m in ('lmdb',):
        sys.modules.setdefault(m, types.ModuleType(m))
    cv2 = sys.modules.setdefault('cv2', types.ModuleType('cv2'))

    def imread(name, flag=None):
        return store[name].copy()

    def resize(img, size, interpolation=None):
        assert tuple(size) == (img.shape[1], img.shape[0]), 'the stand-in only knows the identity: %s of %s' % (size, img.shape)
        return img

    cv2.imread, cv2.resize = imread, resize
    cv2.IMREAD_UNCHANGED, cv2.INTER_LINEAR = -1, 1
    RI.codes_arch()                                     # puts <reference>/codes on sys.path
    util = importlib.import_module('data.util')
    util.get_image_paths = lambda data_type, dataroot: (None, None if dataroot is None else
                                                        sorted(k for k in store if k.startswith(dataroot + '/')))
    return importlib.import_module('data.LRHR_dataset').LRHRDataset


def main():
    assert RI.available(), 'the reference checkout is needed (ESRGAN_REFERENCE)'
    imgs = images()
    res = {'indices': np.array(INDICES, dtype=np.int64), 'scales': np.array(SCALES, dtype=np.int64),
           'lr_size': np.int64(LR_SIZE), 'n_images': np.int64(len(imgs))}
    for k, im in enumerate(imgs):
        res['img%d' % k] = im
    store = {}
    LRHRDataset = dataset_class(store)
    for scale in SCALES:
        store.clear()
        for k, im in enumerate(imgs):
            store['HR/%02d' % k] = im
            store['LR/%02d' % k] = np.ascontiguousarray(im[::scale, ::scale])
        for gen in (0, 1):
            tag = 'x%d_%s' % (scale, 'gen' if gen else 'given')
            ds = LRHRDataset({'phase': 'train', 'scale': scale, 'HR_size': LR_SIZE * scale, 'subset_file': None,
                              'data_type': 'img', 'dataroot_HR': 'HR', 'dataroot_LR': None if gen else 'LR',
                              'color': None, 'use_flip': True, 'use_rot': True})
            seeds, draws, lrs, hrs = [], [], [], []
            for b, i in enumerate(INDICES):
                seed = SEED0 + 100 * scale + 10 * gen + b
                random.seed(seed)
                item = ds[i]
                after = random.getstate()
                random.seed(seed)
                if gen:
                    random.choice([1])
                h, w = imgs[i].shape[0] // scale, imgs[i].shape[1] // scale
                y0, x0 = random.randint(0, max(0, h - LR_SIZE)), random.randint(0, max(0, w - LR_SIZE))
                hf, vf, r9 = random.random() < 0.5, random.random() < 0.5, random.random() < 0.5
                assert random.getstate() == after, 'the item drew something else'
                seeds.append(seed)
                draws.append((y0, x0, int(hf) | int(vf) << 1 | int(r9) << 2))
                lrs.append(item['LR'].numpy())
                hrs.append(item['HR'].numpy())
            res[tag + '_seeds'] = np.array(seeds, dtype=np.int64)
            res[tag + '_draws'] = np.array(draws, dtype=np.int64)
            res[tag + '_LR'] = np.stack(lrs).astype(np.float32)
            res[tag + '_HR'] = np.stack(hrs).astype(np.float32)
            # the restatement the GPU tests are gauged by, on the same draws
            rl, rh = D.batch_reference([imgs[i] for i in INDICES], None if gen else [imgs[i][::scale, ::scale] for i in INDICES],
                                       scale, LR_SIZE, draws, bgr=True)
            dl = float(np.abs(rl.numpy() - res[tag + '_LR']).max())
            assert np.array_equal(rh.numpy(), res[tag + '_HR']), tag
            assert (dl <= 2e-6) if gen else np.array_equal(rl.numpy(), res[tag + '_LR']), (tag, dl)
            print('[gen_batch_golden] %-9s flags %s  batch_reference: HR equal, LR max difference %.2e'
                  % (tag, [d[2] for d in draws], dl))
    flags = {int(f) for k in res if k.endswith('_draws') for f in res[k][:, 2]}
    print('[gen_batch_golden] flag combinations seen:', sorted(flags))
    out = os.path.join(ROOT, 'tests', 'golden', 'batch_assemble.npz')
    np.savez_compressed(out, **res)
    print('done ->', out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
