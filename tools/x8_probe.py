#!/usr/bin/env python
"""x8 self-ensemble timing (profiles/x8_selfensemble.md): the nb = 23 fp16 net on 1x3x128x128 and on a 57x86 image,
(a) ``net.forward_x8`` against (b) what a user could write without it — eight ``net(T_k(x))`` calls with torch flips,
torch inverses, ``cat`` and ``mean`` — in ONE process, interleaved, hipEvent-timed (warm-up, then >= 20 repetitions,
median and spread), plus the two dihedral kernels' own times from a per-op timed replay of the x8 plan.  Every timed
repetition is followed by a synchronisation, so (a) and (b) both start on an idle GPU and include the host's launch
latency: the comparison is of what a caller waits for, not of back-to-back throughput.

    python tools/x8_probe.py [--reps 30] [--json out.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from esrganplus_amd import architecture as arch
from esrganplus_amd import engine as E
from esrganplus_amd import functional as F
from esrganplus_amd import synth


def eight_calls(net, x):
    """The parent-commit route: eight separate forwards, torch transforms between them."""
    ys = [F.x8_inverse(net(F.x8_transform(x, k)), k) for k in range(8)]
    return torch.cat(ys, 0).view(8, *ys[0].shape).mean(0)


def bundled_nonsquare():
    """The non-square bundled LR image (57 x 86) as the inference script feeds it: RGB / 255, NCHW fp32."""
    g = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'sr_infer.npz'))
    img = next(g['lr_' + str(n)] for n in g['names'] if g['lr_' + str(n)].shape[0] != g['lr_' + str(n)].shape[1])
    return torch.from_numpy(np.transpose(img.astype(np.float64) / 255, (2, 0, 1))).float().unsqueeze(0)


def timed(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def stats(ms):
    ms = np.array(ms)
    return {'median_ms': float(np.median(ms)), 'min_ms': float(ms.min()), 'p90_ms': float(np.percentile(ms, 90)), 'n': len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    assert a.reps >= 20
    dev = torch.device('cuda:0')
    net = arch.RRDBNet(3, 3, 64, 23).to(dev).eval()
    net.load_state_dict(synth.rrdbnet_state_dict(23, 0), strict=True)
    net.set_precision('fp16')
    net.max_cached_plans = 8
    res = {}
    with torch.no_grad():
        for tag, shape in (('128x128', (1, 3, 128, 128)), ('57x86', None)):
            x = synth.image_batch(0, *shape, name='x8.probe').to(dev) if tag == '128x128' else bundled_nonsquare().to(dev)
            shape = tuple(x.shape)
            ya, yb = net.forward_x8(x), eight_calls(net, x)
            diff = (ya - yb).abs().max().item()
            for _ in range(a.warmup):
                net.forward_x8(x)
                eight_calls(net, x)
            ta, tb = [], []
            for _ in range(a.reps):                       # interleaved: both see the same clocks
                ta += timed(lambda: net.forward_x8(x), 1)
                tb += timed(lambda: eight_calls(net, x), 1)
            # the plan's own ops, one by one (hipEvents around each; synchronises)
            slots = E.x8_slots(shape[2], shape[3])
            key = ('x8', slots, shape[0], shape[2], shape[3], net.precision, False, False, net._weights(dev).generation)
            xp = net._plans[key]
            ops = {'import': [], 'reduce': [], 'all': []}
            out = torch.zeros(xp.out_shape, dtype=torch.float32, device=dev)
            for _ in range(a.reps):
                tot, imp, red = 0.0, 0.0, 0.0
                for k0, i, accumulate, scale in E.x8_passes(xp.slots):    # every pass with its own range, as X8Plan.run
                    plan = xp.plans[i]
                    plan.bind(k_begin=k0, accumulate=accumulate, scale=scale)
                    arr = plan.ops.array()
                    E.set_nchw(arr[plan.in_op], x.data_ptr())     # (the ops keep the pointers of their last run)
                    E.set_nchw(arr[plan.out_op], out.data_ptr())
                    ms = plan.ops.run_timed(E.current_stream())
                    tot += sum(ms)
                    imp += ms[plan.in_op]
                    red += ms[plan.out_op]
                ops['all'].append(tot)
                ops['import'].append(imp)
                ops['reduce'].append(red)
            r = {'forward_x8': stats(ta), 'eight_calls': stats(tb), 'max_abs_diff': diff,
                 'ops_sum': stats(ops['all']), 'import': stats(ops['import']), 'reduce': stats(ops['reduce'])}
            r['ratio_b_over_a'] = r['eight_calls']['median_ms'] / r['forward_x8']['median_ms']
            r['import_share'] = r['import']['median_ms'] / r['forward_x8']['median_ms']
            r['reduce_share'] = r['reduce']['median_ms'] / r['forward_x8']['median_ms']
            res[tag] = r
            print('[x8_probe] %-8s forward_x8 %.3f ms (min %.3f)  eight calls %.3f ms (min %.3f)  ratio %.2f  '
                  'import %.1f us (%.2f %%)  reduce %.1f us (%.2f %%)  max|a-b| %.2e'
                  % (tag, r['forward_x8']['median_ms'], r['forward_x8']['min_ms'], r['eight_calls']['median_ms'],
                     r['eight_calls']['min_ms'], r['ratio_b_over_a'], 1e3 * r['import']['median_ms'], 100 * r['import_share'],
                     1e3 * r['reduce']['median_ms'], 100 * r['reduce_share'], diff), flush=True)
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
