#!/usr/bin/env python
"""The tiled x8 self-ensemble against what exists without it (profiles/tiled_x8.md): the nb = 23 net with synthetic
weights, B = 1.  tools/tiled_probe.py's method: every step runs in a child process of its own, under its own time limit,
so that peak memory and first-call times start from a fresh allocator and one failed step ends the run:

* ``time:<prec>``  339 x 510: ``net.forward_tiled_x8(x)`` at the defaults against (a) eight ``forward_tiled`` calls
  composed with torch flips and transposes, ``x8_reference(lambda v: net.forward_tiled(v), x)``, and (b)
  ``net.forward_x8(x)``; interleaved in one process, hipEvent-timed (warm-up, then >= 20 repetitions, median / min / p90,
  a synchronisation after every repetition); the max-abs difference of the tiled ensemble to ``forward_x8`` at pad 16
  and pad 32; and the two new kernels' own times from a per-op timed replay of one pass of the plan.
* ``mem:<prec>:<form>``  678 x 1020, one form alone in a process: ``torch.cuda.max_memory_allocated`` of
  ``forward_tiled_x8(x)`` (``tiled_x8``) or of ``forward_x8(x, slots_per_pass=1)``, its leanest setting (``x8``).
* ``first:<prec>:<form>``  one form alone in a process: wall time of the first call on 339 x 510 (cold: weight packing
  and plan build), then of the first call and the call after it on a second image size, 321 x 481 — the plan rebuild
  (``x8``) against the shared plan (``tiled_x8``).

    python tools/tiled_x8_probe.py [--reps 20] [--json out.json] [--limit 300]"""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BIG, SECOND, HUGE = (339, 510), (321, 481), (678, 1020)
PRECS = ('fp16', 'fp32')
STEPS = (['time:%s' % p for p in PRECS] + ['mem:%s:%s' % (p, f) for p in PRECS for f in ('tiled_x8', 'x8')] +
         ['first:%s:%s' % (p, f) for p in PRECS for f in ('tiled_x8', 'x8')])


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
    return synth.image_batch(1, 1, 3, H, W, name='tiled_x8.probe').to(torch.device('cuda:0'))


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
    from esrganplus_amd import engine as E, functional as F
    net, x = _net(prec), _image(*BIG)
    with torch.no_grad():
        forms = [('tiled_x8', lambda: net.forward_tiled_x8(x)),
                 ('eight_forward_tiled', lambda: F.x8_reference(lambda v: net.forward_tiled(v), x)),
                 ('forward_x8', lambda: net.forward_x8(x))]
        for name, fn in forms:
            for _ in range(warmup):
                fn()
        ms = {name: [] for name, _ in forms}
        for _ in range(reps):                            # interleaved: every form sees the same clocks
            for name, fn in forms:
                ms[name].append(_timed(fn))
        res = {name: _stats(ms[name]) for name, _ in forms}
        whole = net.forward_x8(x)
        res['out_abs_max'] = whole.abs().max().item()
        res['max_abs_diff_pad16'] = (net.forward_tiled_x8(x, 96, 16) - whole).abs().max().item()
        res['max_abs_diff_pad32'] = (net.forward_tiled_x8(x, 96, 32) - whole).abs().max().item()
        res['ratio_eight_over_tiled_x8'] = res['eight_forward_tiled']['median_ms'] / res['tiled_x8']['median_ms']
        res['ratio_tiled_x8_over_x8'] = res['tiled_x8']['median_ms'] / res['forward_x8']['median_ms']
        # the two new kernels: a per-op timed replay of the last pass the default plan was bound to
        keep = net.forward_tiled_x8(x)                   # the replay writes into this result
        plan = next(v for k, v in net._plans.items() if k[0] == 'tiled_x8').plans[0]
        torch.cuda.synchronize()
        per_op = [plan.ops.run_timed(E.current_stream()) for _ in range(5)]
        res['gather_import_ms'] = sorted(t[plan.in_op] for t in per_op)[2]
        res['stitch_reduce_ms'] = sorted(t[plan.out_op] for t in per_op)[2]
        res['pass_ms'] = sorted(sum(t) for t in per_op)[2]
        del keep
    return res


def _form(net, form):
    return (lambda x: net.forward_tiled_x8(x)) if form == 'tiled_x8' else (lambda x: net.forward_x8(x, slots_per_pass=1))


def step_mem(prec, form, _reps, _warmup):
    import torch
    net = _net(prec)
    fn = _form(net, form)
    with torch.no_grad():
        x = _image(*HUGE)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        y = fn(x)
        torch.cuda.synchronize()
        wall = 1e3 * (time.perf_counter() - t0)
        del y
    return {'peak_mib': torch.cuda.max_memory_allocated() / 2 ** 20, 'held_before_mib': base / 2 ** 20, 'first_call_ms': wall}


def step_first(prec, form, _reps, _warmup):
    import torch
    net = _net(prec)
    fn = (lambda x: net.forward_tiled_x8(x)) if form == 'tiled_x8' else (lambda x: net.forward_x8(x))
    res = {}
    with torch.no_grad():
        for H, W in (BIG, SECOND):
            x = _image(H, W)
            torch.cuda.synchronize()
            wall = []
            for _ in range(2):
                t0 = time.perf_counter()
                y = fn(x)
                torch.cuda.synchronize()
                wall.append(1e3 * (time.perf_counter() - t0))
                del y
            res['%dx%d' % (H, W)] = {'first_call_ms': wall[0], 'next_call_ms': wall[1], 'plans': len(net._plans)}
    return res


def run_step(step, reps, warmup):
    kind, *args = step.split(':')
    return {'time': step_time, 'mem': step_mem, 'first': step_first}[kind](*args, reps, warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--json', default=None)
    ap.add_argument('--limit', type=int, default=300, help='seconds per step')
    ap.add_argument('--step', default=None, help='run this one step in this process and print its JSON line')
    ap.add_argument('--steps', default=None, help='comma-separated subset of the steps, in the given order')
    a = ap.parse_args()
    assert a.reps >= 20
    if a.step:
        print('[tiled_x8_probe] ' + json.dumps({a.step: run_step(a.step, a.reps, a.warmup)}), flush=True)
        return
    res = {}
    for step in (a.steps.split(',') if a.steps else STEPS):
        cmd = ['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__), '--step', step,
               '--reps', str(a.reps), '--warmup', str(a.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        line = next((l for l in r.stdout.splitlines() if l.startswith('[tiled_x8_probe] ')), None)
        if r.returncode != 0 or line is None:            # a failed step ends the run: nothing more is started
            print(r.stdout[-2000:], r.stderr[-4000:], sep='\n')
            sys.exit('tiled_x8_probe: step %s ended with status %d' % (step, r.returncode))
        res.update(json.loads(line[len('[tiled_x8_probe] '):]))
        print(step, json.dumps(res[step]), flush=True)
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, 'w') as f:
                json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
