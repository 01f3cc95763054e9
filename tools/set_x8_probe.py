#!/usr/bin/env python
"""The x8 self-ensemble of an image set, with 8-bit ends, against the only route there was without it
(profiles/set_x8.md): the nb = 23 net with synthetic weights, fp16, one device.  tools/tiled_many_probe.py's method: every
step runs in a child process of its own, under its own time limit, and one failed step ends the run.  Inside a step
the two routes alternate in one process after a warm-up, each repetition hipEvent-timed and followed by a
synchronisation (median / min / p90 of >= 20).

* route A   ``net.forward_images(images, x8=True, bgr=True)`` on the uint8 HWC device images.
* route B   per image ``net.forward_tiled_x8(x)`` on the float NCHW tensor and ``metrics.device_tensor2img`` of its
  result: what a caller had to write.  Timed twice: ``resident`` with the float tensors already on the device (the
  device work alone), and ``from_uint8`` with the division and the permutation of every image inside the timed region
  (torch ops on the device, in the place of the host's numpy).

Steps: ``small16`` 16 x 128 x 128 at the defaults (tile 96: four windows of 128 x 128 per image, equal pass counts);
``single16`` the same images at tile 128, pad 0, one window each: 8 passes of 2 windows x 8 slots against 16 passes of
1 x 8, the derived gain of packing; ``folder8`` 8 x 339 x 510 at the defaults (equal pass counts: the gain is the ends);
``bundled`` the five LR images of tests/golden/sr_infer.npz.  Every step reports the pass counts, the host time of one
call of either route (wall time from entry to return, the device idle at entry), and how far the routes' 8-bit results
are apart.  Nothing is a gate.

    python tools/set_x8_probe.py [--reps 20] [--json out.json] [--md profiles/set_x8.md] [--limit 240]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PREC = 'fp16'
STEPS = ['small16', 'single16', 'folder8', 'bundled']
TAG = '[set_x8_probe] '


def _net():
    import torch
    from esrganplus_amd import architecture as arch, synth
    net = arch.RRDBNet(3, 3, 64, 23).to(torch.device('cuda:0')).eval()
    net.load_state_dict(synth.rrdbnet_state_dict(23, 0), strict=True)
    net.max_cached_plans = 16
    return net.set_precision(PREC)


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


def _host_ms(fn, reps):
    import numpy as np
    import torch
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        y = fn()
        out.append(1e3 * (time.perf_counter() - t0))
        torch.cuda.synchronize()
        del y
    return float(np.median(out))


def _passes(sizes, tile, pad):
    """Plan runs of either route: windows passes x k passes."""
    from esrganplus_amd import functional as F
    a = sum(len(p) * (8 // s) for _, _, s, _, p in F.tiled_many_x8_passes(sizes, tile, pad))
    b = 0
    for H, W in sizes:
        t, p, P, s = F._tiled_x8_args(1, H, W, tile, pad, None, None)
        n = -(-H // t) * -(-W // t)
        b += -(-n // P) * (8 // s)
    return {'plan_runs_A': a, 'plan_runs_B': b}


def _set_step(u8, tile, pad, reps, warmup):
    import torch
    from esrganplus_amd import metrics as M
    net = _net()
    dev = torch.device('cuda:0')
    u8 = [x.to(dev) for x in u8]
    sizes = [tuple(x.shape[:2]) for x in u8]

    def to_float(x):                                     # BGR bytes -> RGB float NCHW, as the reference's script
        return (x.flip(2).permute(2, 0, 1).float() / 255.0).unsqueeze(0).contiguous()

    floats = [to_float(x) for x in u8]
    with torch.no_grad():
        route_a = lambda: net.forward_images(u8, tile, pad, bgr=True, x8=True)
        route_b = lambda: [M.device_tensor2img(net.forward_tiled_x8(x, tile, pad)) for x in floats]
        route_b8 = lambda: [M.device_tensor2img(net.forward_tiled_x8(to_float(x), tile, pad)) for x in u8]
        forms = [('A_forward_images_x8', route_a), ('B_loop_resident', route_b), ('B_loop_from_uint8', route_b8)]
        for _, fn in forms:
            for _ in range(warmup):
                fn()
        ms = {name: [] for name, _ in forms}
        for _ in range(reps):                            # interleaved: every route sees the same clocks
            for name, fn in forms:
                ms[name].append(_timed(fn))
        res = {name: _stats(v) for name, v in ms.items()}
        res.update(_passes(sizes, tile, pad))
        res['sizes'], res['tile'], res['pad'] = [list(s) for s in sizes], tile, pad
        res['ratio_A_over_B_resident'] = res['A_forward_images_x8']['median_ms'] / res['B_loop_resident']['median_ms']
        res['ratio_A_over_B_from_uint8'] = res['A_forward_images_x8']['median_ms'] / res['B_loop_from_uint8']['median_ms']
        res['host_ms_A'] = _host_ms(route_a, reps)
        res['host_ms_B_resident'] = _host_ms(route_b, reps)
        ya, yb = route_a(), route_b()
        torch.cuda.synchronize()
        d = [(a.int() - b.int()).abs() for a, b in zip(ya, yb)]
        res['max_lsb_A_vs_B'] = max(int(v.max()) for v in d)
        res['differing_share_A_vs_B'] = float(sum(int((v > 0).sum()) for v in d)) / sum(v.numel() for v in d)
        res['bytes_resident_per_lr_pixel'] = {'A': 3 + 48, 'B': 12 + 192 + 48}
        res['plans'] = sorted(str(k[:5]) for k in net._plans)
    return res


def _random_u8(sizes):
    import torch
    g = torch.Generator().manual_seed(1)
    return [torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8) for H, W in sizes]


def step_small16(reps, warmup):
    return _set_step(_random_u8([(128, 128)] * 16), 96, 16, reps, warmup)


def step_single16(reps, warmup):
    return _set_step(_random_u8([(128, 128)] * 16), 128, 0, reps, warmup)


def step_folder8(reps, warmup):
    return _set_step(_random_u8([(339, 510)] * 8), 96, 16, reps, warmup)


def step_bundled(reps, warmup):
    import numpy as np
    import torch
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'sr_infer.npz'))
    return _set_step([torch.from_numpy(g['lr_' + n][:, :, ::-1].copy()) for n in sorted(str(n) for n in g['names'])], 96, 16,
                     reps, warmup)


def _markdown(res, reps):
    rows = ['# The x8 self-ensemble over an image set: `forward_images(x8=True)` against the per-image loop', '',
            'Written by `tools/set_x8_probe.py` (nb = 23, synthetic weights, fp16, one MI355X, one process per step, the',
            'routes alternating, %d repetitions each, hipEvent time of a whole call; median / min / p90 in ms).' % reps, '',
            'Route A: `forward_images(images, x8=True, bgr=True)` on uint8 HWC device images.  Route B: per image',
            '`forward_tiled_x8` on a float NCHW tensor, then `device_tensor2img`; "resident": the float tensors are on the',
            'device already; "from uint8": the division and permutation of every image (torch, on the device) are timed too.', '',
            '| set | tile, pad | plan runs A / B | A | B resident | B from uint8 | A / B resident | host ms A / B | max LSB, differing share A vs B |',
            '|---|---|---|---|---|---|---|---|---|']
    for step in STEPS:
        if step not in res:
            continue
        r = res[step]
        f = lambda s: '%.2f / %.2f / %.2f' % (s['median_ms'], s['min_ms'], s['p90_ms'])
        sizes = r['sizes']
        name = '%d x %dx%d' % (len(sizes), sizes[0][0], sizes[0][1]) if len({tuple(s) for s in sizes}) == 1 else \
            'bundled: ' + ', '.join('%dx%d' % tuple(s) for s in sizes)
        rows.append('| %s (`%s`) | %d, %d | %d / %d | %s | %s | %s | %.3f | %.2f / %.2f | %d, %.4f |'
                    % (name, step, r['tile'], r['pad'], r['plan_runs_A'], r['plan_runs_B'], f(r['A_forward_images_x8']),
                       f(r['B_loop_resident']), f(r['B_loop_from_uint8']), r['ratio_A_over_B_resident'], r['host_ms_A'],
                       r['host_ms_B_resident'], r['max_lsb_A_vs_B'], r['differing_share_A_vs_B']))
    rows += ['', 'A plan run is one launch of the inference plan at a batch of 16 entries (8 slots x 2 windows for square windows).',
             'Derived expectation: the ratio of plan runs where they differ (`single16`: 8 against 16 runs, and B\'s runs hold',
             'a batch of 8); where they are equal the difference is the ends and the per-image launches.  Resident bytes per LR',
             'pixel outside the plan: 3 + 48 (A) against 12 + 192 floats plus the 48 of the 8-bit copy (B).', '',
             'Not measured: fp32, other `windows_per_pass` / `slots_per_pass`, the upload of the images from the host, more than one box.',
             'One box, one session: the absolute times carry that box\'s clocks; the ratios are the result.', '']
    return '\n'.join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--json', default=None)
    ap.add_argument('--md', default=None, help='write the table there (profiles/set_x8.md)')
    ap.add_argument('--limit', type=int, default=240, help='seconds per step')
    ap.add_argument('--step', default=None, help='run this one step in this process and print its JSON line')
    a = ap.parse_args()
    assert a.reps >= 20
    if a.step:
        print(TAG + json.dumps({a.step: globals()['step_' + a.step](a.reps, a.warmup)}), flush=True)
        return
    res = {}
    for step in STEPS:
        cmd = ['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__), '--step', step,
               '--reps', str(a.reps), '--warmup', str(a.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        line = next((l for l in r.stdout.splitlines() if l.startswith(TAG)), None)
        if r.returncode != 0 or line is None:            # a failed step ends the run: nothing more is started
            print(r.stdout[-2000:], r.stderr[-4000:], sep='\n')
            sys.exit('set_x8_probe: step %s ended with status %d' % (step, r.returncode))
        res.update(json.loads(line[len(TAG):]))
        print(step, json.dumps(res[step]), flush=True)
        for path, text in ((a.json, json.dumps(res, indent=1)), (a.md, _markdown(res, a.reps))):
            if path:
                os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
                with open(path, 'w') as f:
                    f.write(text)


if __name__ == '__main__':
    main()
