#!/usr/bin/env python
"""Eval-forward time of the nb = 23 fp16 generator at every supported scale (profiles/scales.md): 16 x 128 x 128 LR at
x1, x2, x3 and x4 — the x4 line is bench.py's default shape and must sit inside the README's box spread — and
4 x 128 x 128 at x8 (16 images would need 2 GiB per 64-channel HR buffer).  Per scale, in ONE process: warm-up forwards,
then >= 20 samples, each a hipEvent pair around a few back-to-back ``net(x)`` calls (what bench.py times, per call),
median and spread.  For x3 also the folded up-conv's own share: the 64 -> 576 conv and the 3x shuffle from a per-op
timed replay of the plan (esr_run_ops_timed), against the sum of all ops of the same replay.  Nothing here is a gate.

    python tools/scales_probe.py [--reps 30] [--md profiles/scales.md]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from esrganplus_amd import _lib as L
from esrganplus_amd import architecture as arch
from esrganplus_amd import engine as E
from esrganplus_amd import synth

NB = 23
CASES = ((1, 16), (2, 16), (3, 16), (4, 16), (8, 4))           # (scale, batch) at 128 x 128 LR
PER_SAMPLE = 4


def sample(net, x, reps):
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(PER_SAMPLE):
            net(x)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / PER_SAMPLE)
    return np.array(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=12)
    ap.add_argument('--md', default=None)
    a = ap.parse_args()
    assert a.reps >= 20
    dev = torch.device('cuda:0')
    lines = ['| scale | LR batch | output | ms / forward (median) | min | p90 | HR-Mpix/s |', '|---|---|---|---|---|---|---|']
    extra = []
    with torch.no_grad():
        for s, B in CASES:
            net = arch.RRDBNet(3, 3, 64, NB, upscale=s).to(dev).eval().set_precision('fp16')
            net.load_state_dict(synth.rrdbnet_state_dict(NB, 0, upscale=s), strict=True)
            x = synth.image_batch(100, B, 3, 128, 128, name='bench.x').to(dev)
            for _ in range(a.warmup):
                y = net(x)
            torch.cuda.synchronize()
            assert torch.isfinite(y).all() and tuple(y.shape) == (B, 3, 128 * s, 128 * s)
            ms = sample(net, x, a.reps)
            med = float(np.median(ms))
            lines.append('| x%d | %d x 128 x 128 | %d x %d | %.3f | %.3f | %.3f | %.1f |'
                         % (s, B, 128 * s, 128 * s, med, ms.min(), np.percentile(ms, 90), B * (128 * s) ** 2 / 1e6 / (med * 1e-3)))
            print('[scales_probe]', lines[-1], flush=True)
            if s == 3:
                (plan,) = net._plans.values()
                arr = plan.ops.array()
                out = torch.empty(plan.out_shape, dtype=torch.float32, device=dev)
                E.set_nchw(arr[plan.in_op], x.data_ptr())
                E.set_nchw(arr[plan.out_op], out.data_ptr())
                fold = [i for i, o in enumerate(plan.ops.ops) if o.kind == L.OP_CONV and o.u.conv.cout_blocks == 18]
                shuf = [i for i, o in enumerate(plan.ops.ops) if o.kind == L.OP_POOL]
                assert len(fold) == 1 and len(shuf) == 1
                tot, f_, s_ = [], [], []
                for _ in range(a.reps):
                    t = plan.ops.run_timed(E.current_stream())
                    tot.append(sum(t))
                    f_.append(t[fold[0]])
                    s_.append(t[shuf[0]])
                tot, f_, s_ = float(np.median(tot)), float(np.median(f_)), float(np.median(s_))
                extra.append('x3, per-op timed replay of the plan (median of %d): all ops %.3f ms; folded 64 -> 576 conv %.3f ms, '
                             '3x shuffle %.3f ms: together %.1f %% of the forward.' % (a.reps, tot, f_, s_, 100 * (f_ + s_) / tot))
                print('[scales_probe]', extra[-1], flush=True)
            del net
            torch.cuda.empty_cache()
    text = '\n'.join(['Box: %s, torch %s.  nb = %d, fp16, eval forward; %d samples of %d back-to-back forwards after %d warm-up '
                      'forwards.' % (torch.cuda.get_device_name(0), torch.__version__, NB, a.reps, PER_SAMPLE, a.warmup), '']
                     + lines + [''] + extra)
    print(text)
    if a.md:
        with open(a.md, 'w') as f:
            f.write('# RRDBNet eval forward by scale (tools/scales_probe.py)\n\n' + text + '\n')


if __name__ == '__main__':
    main()
