#!/usr/bin/env python
"""``train.PSNRStep`` against the generator loop it packages (profiles/psnr_step.md): the nb = 23 net in fp16 with loss
scale 1024 on bench.py's three generator-training buckets (16 x 128^2, 8 x 192^2, 4 x 256^2 LR per step), l1, lr 1e-4.

A = ``bench.measure_gtrain`` — the hand-written loop, imported from bench.py as it stands, neither copied nor edited;
B = the same buckets through ``PSNRStep.step(sync_log=False)``, timed the way the loop times itself: one HIP event in front
of every bucket's step and one behind the last, per-bucket time = the distance of neighbouring events, averaged over the
timed steps.  Both in ONE process, in the order A - B - A: the two A runs give the run-to-run spread the B figure is
read against.  Expectation: the step is no slower than the loop, i.e. B - mean(A) lies within |A1 - A2|.
``--serial`` appends B0 - A: the step with ESR_TRAIN_OVERLAP=0 (no side stream: nothing runs next to the forward), to
tell what the side stream costs or buys at the measured shapes.  ``--buckets 16x32`` measures other shapes (the
reference's train_sr.json crops are 16 x 32^2 LR).

    python tools/psnr_step_probe.py [--steps 20] [--warmup 5] [--serial] [--buckets NxS,...] [--json out.json] [--md out.md]"""
import argparse
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402


def loop(dev, steps, warmup):
    args = argparse.Namespace(precision='fp16')
    dt, per, lr_pix = bench.measure_gtrain(args, 1, 0, dev, None, steps, warmup, data_parallel=False)
    return {'ms_per_step': dt * 1e3, 'buckets_ms': per, 'lr_pixels': lr_pix}


def step_object(dev, steps, warmup):
    from esrganplus_amd import architecture as arch, synth, train
    netG = arch.RRDBNet(3, 3, 64, bench.NB).to(dev).train().set_precision('fp16')
    netG.load_state_dict(synth.rrdbnet_state_dict(bench.NB, 0, gain=0.5))
    st = train.PSNRStep(netG, lr_G=1e-4, pixel_criterion='l1', loss_scale=1024.0, data_parallel=False)
    assert st._manual_ok()
    buckets = []
    for k, (n, sz) in enumerate(bench.GTRAIN_BUCKETS):          # measure_gtrain's data, rank 0
        buckets.append((synth.image_batch(400 + k, n, 3, sz, sz, name='bench.glr').to(dev),
                        synth.image_batch(500 + k, n, 3, 4 * sz, 4 * sz, name='bench.ghr').to(dev)))
    marks = []

    def one(timed=False):
        for lr, hr in buckets:
            if timed:
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                marks.append(e)
            log = st.step(lr, hr, sync_log=False)
        if timed:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            marks.append(e)
        return log['l_pix']

    for _ in range(max(warmup, 1)):
        one()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = one(True)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    assert torch.isfinite(loss).all()
    nbk = len(buckets) + 1
    per = [0.0] * len(buckets)
    for s in range(steps):
        ev = marks[s * nbk:(s + 1) * nbk]
        for k in range(len(buckets)):
            per[k] += ev[k].elapsed_time(ev[k + 1]) / steps
    return {'ms_per_step': dt * 1e3, 'buckets_ms': per,
            'lr_pixels': sum(l.shape[0] * l.shape[2] * l.shape[3] for l, _ in buckets)}


def _release():
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def table(res, b='B', a1='A1', a2='A2'):
    head = '| bucket | %s loop ms | %s PSNRStep ms | %s loop ms | B - mean(A) ms | A spread ms | within spread |' % (a1, b, a2)
    a1, b, a2 = res[a1], res[b], res[a2]
    names = ['%dx%d^2' % bk for bk in bench.GTRAIN_BUCKETS] + ['step (wall)']
    rows = [(a1['buckets_ms'][k], b['buckets_ms'][k], a2['buckets_ms'][k]) for k in range(len(bench.GTRAIN_BUCKETS))]
    rows.append((a1['ms_per_step'], b['ms_per_step'], a2['ms_per_step']))
    out = [head, '|---|---|---|---|---|---|---|']
    verdicts = []
    for name, (x1, y, x2) in zip(names, rows):
        diff, spread = y - 0.5 * (x1 + x2), abs(x1 - x2)
        ok = diff <= spread
        verdicts.append(ok)
        out.append('| %s | %.3f | %.3f | %.3f | %+.3f | %.3f | %s |' % (name, x1, y, x2, diff, spread, 'yes' if ok else 'NO'))
    return '\n'.join(out), all(verdicts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--serial', action='store_true', help='append B0 (ESR_TRAIN_OVERLAP=0) and a third loop run')
    ap.add_argument('--buckets', help='NxS,... LR buckets instead of those of bench.py (sets bench.GTRAIN_BUCKETS)')
    ap.add_argument('--json')
    ap.add_argument('--md')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the GPU'
    dev = torch.device('cuda:0')
    if a.buckets:
        bench.GTRAIN_BUCKETS = tuple(tuple(int(v) for v in b.split('x')) for b in a.buckets.split(','))
    res = {'steps': a.steps, 'warmup': a.warmup, 'device': torch.cuda.get_device_name(0),
           'buckets': ['%dx%d^2' % b for b in bench.GTRAIN_BUCKETS]}
    runs = [('A1', loop), ('B', step_object), ('A2', loop)] + ([('B0', step_object), ('A3', loop)] if a.serial else [])
    for tag, fn in runs:
        saved = os.environ.get('ESR_TRAIN_OVERLAP')
        if tag == 'B0':
            os.environ['ESR_TRAIN_OVERLAP'] = '0'           # read by the step's constructor
        res[tag] = fn(dev, a.steps, a.warmup)
        if tag == 'B0':
            os.environ.pop('ESR_TRAIN_OVERLAP')
            if saved is not None:
                os.environ['ESR_TRAIN_OVERLAP'] = saved
        print(tag, json.dumps(res[tag]), flush=True)
        _release()
    md, ok = table(res)
    res['no_slower_than_the_loop'] = ok
    print(md)
    print('PSNRStep no slower than the loop (every row within the A-A spread):', ok)
    if a.serial:
        md0, ok0 = table(res, 'B0', 'A2', 'A3')
        res['serial_no_slower_than_the_loop'] = ok0
        print(md0)
        md += '\n\n' + md0
    if a.json:
        json.dump(res, open(a.json, 'w'), indent=1)
    if a.md:
        open(a.md, 'w').write(md + '\n')


if __name__ == '__main__':
    main()
