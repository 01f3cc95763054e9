#!/usr/bin/env python
"""What feeding a train step costs (profiles/data_path.md): a pool of eight synthetic uint8 images of about 480 x 320,
batches of 16 x 32^2 LR at scale 4, in three forms —

  (a) ``TrainSet.batch`` with LR images given (uint8 pool, one launch per batch);
  (b) ``TrainSet.batch`` with LR generated from the HR window (uint8 pool, one launch per batch);
  (c) the helpers alone, as before ``TrainSet``: a float32 pool, ``imresize`` of every whole image once outside the loop,
      and per batch one ``crop_and_augment`` per group of images of one size, concatenated.

Per form: host wall time per batch (no synchronisation inside the loop, one at the end — what the Python thread spends
before it can launch the step) and device time per batch (HIP events round the whole loop), the device memory of the pool.
Every form draws its sample indices and its windows from the same seeds.

    python tools/data_path_probe.py [--batches 200] [--warmup 20] [--json out.json] [--md out.md]

The kernel's own time: one run under ``rocprofv3 --kernel-trace --stats -- python tools/data_path_probe.py``."""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from esrganplus_amd import data as D  # noqa: E402

SIZES = ((480, 320), (320, 480), (480, 320), (448, 336), (336, 448), (480, 320), (320, 480), (464, 304))
B, LR_SIZE, SCALE = 16, 32, 4
STEP_MS = (6.1, 6.3)          # a full ESRGAN+ train step at 16 x 32^2 LR


def pool():
    out = []
    for k, (h, w) in enumerate(SIZES):
        rs = np.random.RandomState(900 + k)
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        base = np.stack([128 + 100 * np.sin(yy / 17.0), 128 + 100 * np.cos(xx / 23.0), 255 * (yy + xx) / (h + w)], axis=2)
        out.append(np.clip(base + rs.uniform(-20, 20, size=(h, w, 3)), 0, 255).astype(np.uint8))
    return out


def timed(fn, batches, warmup):
    """-> (host ms per batch, device ms per batch)"""
    random.seed(1)
    rs = np.random.RandomState(2)
    ids = [rs.randint(0, len(SIZES), size=B).tolist() for _ in range(batches + warmup)]
    for k in range(warmup):
        fn(ids[k])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    for k in range(warmup, warmup + batches):
        out = fn(ids[k])
    host = (time.perf_counter() - t0) / batches
    e1.record()
    torch.cuda.synchronize()
    assert tuple(out[0].shape) == (B, 3, LR_SIZE, LR_SIZE) and tuple(out[1].shape) == (B, 3, LR_SIZE * SCALE, LR_SIZE * SCALE)
    return host * 1e3, e0.elapsed_time(e1) / batches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--json')
    ap.add_argument('--md')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the GPU'
    dev = torch.device('cuda:0')
    hr_u8 = pool()
    # the LR side of forms (a) and (c): imresize of the whole images, once
    hr_f32 = [torch.from_numpy(np.transpose(im.astype(np.float32) / np.float32(255), (2, 0, 1)).copy()).to(dev) for im in hr_u8]
    lr_f32 = [D.imresize(x, 1.0 / SCALE) for x in hr_f32]
    lr_u8 = [(t.clamp(0, 1) * 255).round().byte().permute(1, 2, 0).cpu().numpy() for t in lr_f32]
    res = {'batches': a.batches, 'warmup': a.warmup, 'device': torch.cuda.get_device_name(0), 'B': B, 'lr_size': LR_SIZE,
           'scale': SCALE, 'sizes': ['%dx%d' % s for s in SIZES]}

    ts_a = D.TrainSet(hr_u8, lr_u8, scale=SCALE, lr_size=LR_SIZE, device=dev)
    ts_b = D.TrainSet(hr_u8, None, scale=SCALE, lr_size=LR_SIZE, device=dev)
    tables_b = sum(w.numel() * 4 + i.numel() * 4 for w, i, _ in ts_b._tables.values())

    # (c): the images of one size stacked into an NCHW pool per size
    groups = {}
    for k, s in enumerate(SIZES):
        groups.setdefault(s, []).append(k)
    where = {k: (s, j) for s, ks in groups.items() for j, k in enumerate(ks)}
    pools_c = {s: (torch.stack([lr_f32[k] for k in ks]), torch.stack([hr_f32[k] for k in ks])) for s, ks in groups.items()}
    bytes_c = sum(l.numel() * 4 + h.numel() * 4 for l, h in pools_c.values())

    def form_c(ids):
        outl, outh = [], []
        by = {}
        for i in ids:
            s, j = where[i]
            by.setdefault(s, []).append(j)
        for s, js in by.items():
            lp, hp = pools_c[s]
            l, h = D.crop_and_augment(lp[js], hp[js], LR_SIZE, SCALE)
            outl.append(l)
            outh.append(h)
        return torch.cat(outl), torch.cat(outh)

    forms = (('a', 'TrainSet.batch, LR given (uint8 pool)', ts_a.batch, ts_a.pool_bytes),
             ('b', 'TrainSet.batch, LR generated (uint8 pool)', ts_b.batch, ts_b.pool_bytes + tables_b),
             ('c', 'float32 pool, imresize once, crop_and_augment per size group', form_c, bytes_c))
    for tag, name, fn, nbytes in forms:
        host, devms = timed(fn, a.batches, a.warmup)
        res[tag] = {'name': name, 'host_ms_per_batch': host, 'device_ms_per_batch': devms, 'pool_bytes': int(nbytes)}
        print(tag, json.dumps(res[tag]), flush=True)
    lines = ['| form | host ms / batch | device ms / batch | pool on the device, MB | host share of a %.1f - %.1f ms step |' % STEP_MS,
             '|---|---|---|---|---|']
    for tag, name, _, _ in forms:
        r = res[tag]
        lines.append('| (%s) %s | %.3f | %.3f | %.2f | %.1f - %.1f %% |' % (tag, name, r['host_ms_per_batch'], r['device_ms_per_batch'],
                                                                           r['pool_bytes'] / 1e6, 100 * r['host_ms_per_batch'] / STEP_MS[1],
                                                                           100 * r['host_ms_per_batch'] / STEP_MS[0]))
    md = '\n'.join(lines)
    res['fused_faster_on_the_host'] = bool(max(res['a']['host_ms_per_batch'], res['b']['host_ms_per_batch']) < res['c']['host_ms_per_batch'])
    print(md)
    print('the fused path is faster on the host than (c):', res['fused_faster_on_the_host'])
    if a.json:
        json.dump(res, open(a.json, 'w'), indent=1)
    if a.md:
        open(a.md, 'w').write(md + '\n')


if __name__ == '__main__':
    main()
