#!/usr/bin/env python
"""Tiled inference against the whole-image forward (profiles/tiled_inference.md): the nb = 23 net with synthetic weights.
Every step runs in a child process of its own, under its own time limit, so that peak memory and first-call times start
from a fresh allocator and one failed step ends the run:

* ``time:<prec>``  339 x 510: ``net(x)`` and ``net.forward_tiled(x, tile, pad)`` for the default window and the other
  settings of SETTINGS, interleaved in one process, hipEvent-timed (warm-up, then >= 20 repetitions, median / min / p90,
  a synchronisation after every repetition), and per setting the max-abs difference and the PSNR
  (``metrics.device_psnr_ssim``) of the tiled against the whole-image output: what the pad costs in fidelity.
* ``first:<prec>:<form>``  one form (``whole`` or ``tiled``) alone in a process: wall time of the first call on 339 x 510
  (cold: weight packing and plan build), of the first call on each further image size (the plan build the shared tiled
  plan removes) and of the call after it, and ``torch.cuda.max_memory_allocated`` on 339 x 510 and on 678 x 1020.

    python tools/tiled_probe.py [--reps 20] [--json out.json] [--limit 240]"""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SETTINGS = ((96, 16), (112, 8), (64, 32))            # (tile, pad): the default 128 x 128 window first
BIG = (339, 510)
SIZES = ((339, 510), (321, 481), (256, 384), (678, 1020))
STEPS = ['time:fp16', 'time:fp32'] + ['first:%s:%s' % (p, f) for p in ('fp16', 'fp32') for f in ('whole', 'tiled')]


def _net(prec):
    import torch
    from esrganplus_amd import architecture as arch, synth
    net = arch.RRDBNet(3, 3, 64, 23).to(torch.device('cuda:0')).eval()
    net.load_state_dict(synth.rrdbnet_state_dict(23, 0), strict=True)
    net.max_cached_plans = 8
    return net.set_precision(prec)


def _image(H, W):
    import torch
    from esrganplus_amd import synth
    return synth.image_batch(1, 1, 3, H, W, name='tiled.probe').to(torch.device('cuda:0'))


def _timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def _stats(ms):
    import numpy as np
    ms = np.array(ms)
    return {'median_ms': float(np.median(ms)), 'min_ms': float(ms.min()), 'p90_ms': float(np.percentile(ms, 90)), 'n': len(ms)}


def step_time(prec, reps, warmup):
    import torch
    from esrganplus_amd import metrics
    net, x = _net(prec), _image(*BIG)
    with torch.no_grad():
        forms = [('whole', lambda: net(x))] + [('tile %d pad %d' % s, lambda s=s: net.forward_tiled(x, *s)) for s in SETTINGS]
        whole = net(x)
        res = {'out_abs_max': whole.abs().max().item()}
        for name, fn in forms:
            for _ in range(warmup):
                fn()
        ms = {name: [] for name, _ in forms}
        for _ in range(reps):                            # interleaved: every form sees the same clocks
            for name, fn in forms:
                ms[name].append(_timed(fn))
        for name, fn in forms:
            r = _stats(ms[name])
            if name != 'whole':
                y = fn()
                r['max_abs_diff'] = (y - whole).abs().max().item()
                r['psnr_db'] = metrics.device_psnr_ssim(y[0], whole[0])[0]
            res[name] = r
    return res


def step_first(prec, form, _reps, _warmup):
    import torch
    net = _net(prec)
    fn = (lambda x: net(x)) if form == 'whole' else (lambda x: net.forward_tiled(x))
    res = {}
    with torch.no_grad():
        for H, W in SIZES:
            x = _image(H, W)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            wall = []
            for _ in range(2):
                t0 = time.perf_counter()
                y = fn(x)
                torch.cuda.synchronize()
                wall.append(1e3 * (time.perf_counter() - t0))
                del y
            res['%dx%d' % (H, W)] = {'first_call_ms': wall[0], 'next_call_ms': wall[1], 'plans': len(net._plans),
                                     'peak_mib': torch.cuda.max_memory_allocated() / 2 ** 20, 'held_before_mib': base / 2 ** 20}
    return res


def run_step(step, reps, warmup):
    kind, *args = step.split(':')
    return {'time': step_time, 'first': step_first}[kind](*args, reps, warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--json', default=None)
    ap.add_argument('--limit', type=int, default=240, help='seconds per step')
    ap.add_argument('--step', default=None, help='run this one step in this process and print its JSON line')
    a = ap.parse_args()
    assert a.reps >= 20
    if a.step:
        print('[tiled_probe] ' + json.dumps({a.step: run_step(a.step, a.reps, a.warmup)}), flush=True)
        return
    res = {}
    for step in STEPS:
        cmd = ['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__), '--step', step,
               '--reps', str(a.reps), '--warmup', str(a.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        line = next((l for l in r.stdout.splitlines() if l.startswith('[tiled_probe] ')), None)
        if r.returncode != 0 or line is None:            # a failed step ends the run: nothing more is started
            print(r.stdout[-2000:], r.stderr[-4000:], sep='\n')
            sys.exit('tiled_probe: step %s ended with status %d' % (step, r.returncode))
        res.update(json.loads(line[len('[tiled_probe] '):]))
        print(step, json.dumps(res[step]), flush=True)
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, 'w') as f:
                json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
