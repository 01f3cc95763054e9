#!/usr/bin/env python
"""Scoring an image set in one device pass against the per-pair route it replaces (profiles/set_metrics.md).  Metrics
only: no network weights are needed for the first two steps.  tools/image_io_probe.py's method: every step runs in a
child process of its own, under its own time limit, and one failed step ends the run.

* ``sets``     two sets of seeded uint8 image pairs on the device — (a) the x4 sizes of the five bundled LR images of
  tests/golden/sr_infer.npz, (b) 8 pairs of 1356 x 2040, the HR size of the 339 x 510 case — each scored by
  ``metrics.device_set_metrics(...).read()`` (the set route) and by the per-pair route: per image, uint8 -> float CHW on
  the device and ``device_psnr_ssim`` twice (RGB, then Y).  Wall time per set, the two routes alternated after a
  warm-up: median, min, max and the interquartile range of the repetitions.  Peak device memory of each route over what
  is allocated before it, and a check that both give the same numbers to 1e-9.
* ``trace``    device time: each route of set (b) in a child of its own under ``rocprofv3 --kernel-trace``, the summed
  kernel durations per scored set, by kernel.
* ``forward``  what scoring adds to ``forward_images``: the nb = 23 net with synthetic weights, fp16, 8 seeded 339 x 510
  LR images, ``forward_images`` + synchronise against ``evaluate_images`` + ``read()``, alternated in one process.

    python tools/set_metrics_probe.py [--reps 20] [--json out.json] [--limit 240] [--trace-dir DIR]"""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = ['sets', 'trace', 'forward']
CROP = 4
TRACE_RUNS = 4


def _pairs(sizes, seed):
    """Seeded uint8 pairs on the device: hr uniform, sr = hr plus noise of a few grey levels (a ~30 dB operating point)."""
    import numpy as np
    import torch
    rng = np.random.RandomState(seed)
    dev = torch.device('cuda:0')
    sr, hr = [], []
    for h, w in sizes:
        b = rng.randint(0, 256, (h, w, 3)).astype(np.int16)
        a = np.clip(b + np.rint(rng.standard_normal((h, w, 3)) * 8).astype(np.int16), 0, 255)
        sr.append(torch.from_numpy(a.astype(np.uint8)).to(dev))
        hr.append(torch.from_numpy(b.astype(np.uint8)).to(dev))
    return sr, hr


def _sizes(which):
    import numpy as np
    if which == 'b':
        return [(1356, 2040)] * 8
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'sr_infer.npz'))
    return [(4 * g['lr_' + n].shape[0], 4 * g['lr_' + n].shape[1]) for n in sorted(str(n) for n in g['names'])]


def _set_route(sr, hr):
    from esrganplus_amd import metrics as M
    return M.device_set_metrics(sr, hr, CROP, bgr=True).read()


def _pair_route(sr, hr):
    """The route before the set kernel: per image, the uint8 BGR images back to float RGB CHW on the device, then the
    per-pair kernel twice; each call reads its doubles back."""
    import numpy as np
    from esrganplus_amd import metrics as M
    rows = []
    for a, b in zip(sr, hr):
        fa, fb = a.flip(2).permute(2, 0, 1).float().div(255.0), b.flip(2).permute(2, 0, 1).float().div(255.0)
        rows.append(M.device_psnr_ssim(fa, fb, crop=CROP) + M.device_psnr_ssim(fa, fb, crop=CROP, y_only=True))
    return np.array(rows, dtype=np.float64)


ROUTES = [('set', _set_route), ('pair', _pair_route)]


def _spread(ms):
    import numpy as np
    a = np.array(ms)
    return {'median_ms': float(np.median(a)), 'min_ms': float(a.min()), 'max_ms': float(a.max()),
            'iqr_ms': float(np.percentile(a, 75) - np.percentile(a, 25)), 'n': len(ms)}


def step_sets(reps, warmup):
    import numpy as np
    import torch
    res = {}
    for which in ('a', 'b'):
        sizes = _sizes(which)
        sr, hr = _pairs(sizes, 20241020)
        out, ms = {}, {n: [] for n, _ in ROUTES}
        for name, fn in ROUTES:
            for _ in range(warmup):
                out[name] = fn(sr, hr)
        for _ in range(reps):                            # alternated: both routes see the same clocks and host load
            for name, fn in ROUTES:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(sr, hr)
                ms[name].append(1e3 * (time.perf_counter() - t0))
        r = {'sizes': [list(s) for s in sizes], 'pixels': int(sum(h * w for h, w in sizes)),
             'largest_difference': float(np.nanmax(np.abs(out['set'] - out['pair']))), 'set_numbers_first_pair': out['set'][0].tolist()}
        for name, fn in ROUTES:
            r[name] = _spread(ms[name])
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            fn(sr, hr)
            torch.cuda.synchronize()
            r[name]['peak_bytes_over_base'] = int(torch.cuda.max_memory_allocated() - base)
            r[name]['base_bytes'] = int(base)
        res[which] = r
    return res


def step_trace_child(route):
    """Runs under rocprofv3: TRACE_RUNS scorings of set (b) by one route; every kernel of the process belongs to them."""
    sr, hr = _pairs(_sizes('b'), 20241020)
    fn = dict(ROUTES)[route]
    for _ in range(TRACE_RUNS):
        fn(sr, hr)


def _short(n):
    n = re.sub(r'\(anonymous namespace\)::', '', n)
    n = re.sub(r'void at::native::', 'at::', n)
    return re.sub(r'\(.*', '', n)[:60]


def step_trace(_reps, _warmup, trace_dir, limit):
    res = {}
    for route, _ in ROUTES:
        d = os.path.join(trace_dir, route)
        os.makedirs(d, exist_ok=True)
        cmd = ['timeout', '-k', '10', str(limit), 'rocprofv3', '--kernel-trace', '--output-format', 'csv', '-d', d, '-o', 'tr',
               '--', sys.executable, os.path.abspath(__file__), '--step', 'trace_child', '--route', route]
        r = subprocess.run(cmd, capture_output=True, text=True)
        files = glob.glob(os.path.join(d, '**', '*kernel_trace.csv'), recursive=True)
        if r.returncode != 0 or not files:
            print(r.stdout[-2000:], r.stderr[-4000:], sep='\n')
            sys.exit('set_metrics_probe: the traced run of route %s ended with status %d' % (route, r.returncode))
        agg = {}
        for row in csv.DictReader(open(files[0])):
            k = _short(row['Kernel_Name'])
            v = agg.setdefault(k, [0, 0])
            v[0] += 1
            v[1] += int(row['End_Timestamp']) - int(row['Start_Timestamp'])
        res[route] = {'device_ms_per_set': sum(v[1] for v in agg.values()) / 1e6 / TRACE_RUNS,
                      'launches_per_set': sum(v[0] for v in agg.values()) / TRACE_RUNS,
                      'kernels': {k: {'launches_per_set': v[0] / TRACE_RUNS, 'ms_per_set': v[1] / 1e6 / TRACE_RUNS}
                                  for k, v in sorted(agg.items(), key=lambda kv: -kv[1][1])}}
    return res


def step_forward(reps, warmup):
    import numpy as np
    import torch
    from esrganplus_amd import architecture as arch, synth
    dev = torch.device('cuda:0')
    net = arch.RRDBNet(3, 3, 64, 23).to(dev).eval()
    net.load_state_dict(synth.rrdbnet_state_dict(23, 0), strict=True)
    net.set_precision('fp16')
    rng = np.random.RandomState(20241020)
    lr = [torch.from_numpy(rng.randint(0, 256, (339, 510, 3)).astype(np.uint8)).to(dev) for _ in range(8)]
    hr = [torch.from_numpy(rng.randint(0, 256, (1356, 2040, 3)).astype(np.uint8)).to(dev) for _ in range(8)]

    def forward():
        net.forward_images(lr)
        torch.cuda.synchronize()

    def evaluate():
        net.evaluate_images(lr, hr)[1].read()

    forms = [('forward_images', forward), ('evaluate_images', evaluate)]
    ms = {n: [] for n, _ in forms}
    with torch.no_grad():
        for _ in range(warmup):
            for _, f in forms:
                f()
        for _ in range(reps):
            for n, f in forms:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                ms[n].append(1e3 * (time.perf_counter() - t0))
    res = {n: _spread(v) for n, v in ms.items()}
    res['added_ms_median'] = res['evaluate_images']['median_ms'] - res['forward_images']['median_ms']
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--json', default=None)
    ap.add_argument('--limit', type=int, default=240, help='seconds per step')
    ap.add_argument('--trace-dir', default=None, help='where the two kernel traces go (default: a temporary directory)')
    ap.add_argument('--step', default=None, help='run this one step in this process and print its JSON line')
    ap.add_argument('--route', default=None)
    a = ap.parse_args()
    if a.trace_dir is None and a.step in (None, 'trace'):
        a.trace_dir = tempfile.mkdtemp(prefix='set_metrics_trace_')
    if a.step == 'trace_child':
        return step_trace_child(a.route)
    if a.step:
        if a.step == 'trace':
            out = step_trace(a.reps, a.warmup, a.trace_dir, a.limit)
        elif a.step == 'forward':                        # a forward over the set takes seconds: fewer repetitions
            out = step_forward(min(a.reps, 8), 2)
        else:
            out = step_sets(a.reps, a.warmup)
        print('[set_metrics_probe] ' + json.dumps({a.step: out}), flush=True)
        return
    res = {}
    for step in STEPS:
        cmd = ['timeout', '-k', '10', str(2 * a.limit + 30 if step == 'trace' else a.limit), sys.executable, os.path.abspath(__file__),
               '--step', step, '--reps', str(a.reps), '--warmup', str(a.warmup), '--trace-dir', a.trace_dir, '--limit', str(a.limit)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        line = next((l for l in r.stdout.splitlines() if l.startswith('[set_metrics_probe] ')), None)
        if r.returncode != 0 or line is None:            # a failed step ends the run: nothing more is started
            print(r.stdout[-2000:], r.stderr[-4000:], sep='\n')
            sys.exit('set_metrics_probe: step %s ended with status %d' % (step, r.returncode))
        res.update(json.loads(line[len('[set_metrics_probe] '):]))
        print(step, json.dumps(res[step]), flush=True)
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, 'w') as f:
                json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
