#!/usr/bin/env python
"""Tiled inference over an image set against what exists without it (profiles/tiled_many.md): the nb = 23 net with
synthetic weights, fp16, one device.  tools/tiled_probe.py's method: every step runs in a child process of its own, under
its own time limit, and one failed step ends the run.  Inside a step the forms are interleaved in one process after a
warm-up, each repetition hipEvent-timed and followed by a synchronisation (median / min / p90 of >= 20).

* ``folder8``   8 x 339 x 510: the loop of ``net.forward_tiled(x)`` (16 passes of 16 windows) against
  ``net.forward_tiled_many(xs)`` (12 passes), both at their defaults; the derived expectation is the pass ratio 0.75.
* ``small16``   16 x 128 x 128 (4 tiles each, every window the whole image): ``forward_tiled_many`` (4 passes of 16)
  against the ``forward_tiled`` loop (16 passes of 4 windows), the ``net(x)`` loop and one ``net(x16)`` batch of the 16
  images, the floor.
* ``bundled``   the five LR images of tests/golden/sr_infer.npz: ``forward_tiled_many`` against the two loops.
* ``kernels``   the two new kernels on one pass of 16 x 128 x 128 windows of a 339 x 510 image next to ``esr_tile_op`` on
  the same windows: hipEvent time over 50 back-to-back launches, per launch.
Every timing step also reports the host time of one ``forward_tiled_many`` call (the call returns without a
synchronisation: wall time from entry to return, the device idle at entry) and the bytes of its slot table, and checks
that the outputs of the forms agree bit for bit where they run the same batches.

    python tools/tiled_many_probe.py [--reps 20] [--json out.json] [--limit 240]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PREC = 'fp16'
STEPS = ['folder8', 'small16', 'bundled', 'kernels']


def _net():
    import torch
    from esrganplus_amd import architecture as arch, synth
    net = arch.RRDBNet(3, 3, 64, 23).to(torch.device('cuda:0')).eval()
    net.load_state_dict(synth.rrdbnet_state_dict(23, 0), strict=True)
    net.max_cached_plans = 16
    return net.set_precision(PREC)


def _images(sizes):
    import torch
    from esrganplus_amd import synth
    return [synth.image_batch(1 + i, 1, 3, H, W, name='tiled_many.probe').to(torch.device('cuda:0')) for i, (H, W) in enumerate(sizes)]


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


def _passes(sizes, tile=96, pad=16, S=16):
    from esrganplus_amd import functional as F
    many = sum(len(p) for _, _, _, p in F.tiled_many_passes(sizes, tile, pad, S))
    loop = 0
    for H, W in sizes:
        n = -(-H // tile) * -(-W // tile)
        loop += -(-n // min(S, n))
    slots = sum(Sg * len(p) for _, _, Sg, p in F.tiled_many_passes(sizes, tile, pad, S))
    return {'passes_many': many, 'passes_loop': loop, 'table_bytes': 2 * 24 * slots}


def _compare(forms, reps, warmup):
    """Interleaved timing of [(name, fn)] -> {name: stats}."""
    for name, fn in forms:
        for _ in range(warmup):
            fn()
    ms = {name: [] for name, _ in forms}
    for _ in range(reps):                                # interleaved: every form sees the same clocks
        for name, fn in forms:
            ms[name].append(_timed(fn))
    return {name: _stats(v) for name, v in ms.items()}


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


def _same(a, b):
    import torch
    return bool(torch.equal(a.reshape(-1).view(torch.int32), b.reshape(-1).view(torch.int32)))


def _set_step(sizes, with_batch, reps, warmup):
    import torch
    net, xs = _net(), _images(sizes)
    with torch.no_grad():
        forms = [('forward_tiled_many', lambda: net.forward_tiled_many(xs)),
                 ('forward_tiled_loop', lambda: [net.forward_tiled(x) for x in xs]),
                 ('forward_loop', lambda: [net(x) for x in xs])]
        if with_batch:
            xb = torch.cat(xs, 0)
            forms.append(('forward_batch', lambda: net(xb)))
        res = _compare(forms, reps, warmup)
        res.update(_passes(sizes))
        res['sizes'] = [list(s) for s in sizes]
        res['ratio_many_over_tiled_loop'] = res['forward_tiled_many']['median_ms'] / res['forward_tiled_loop']['median_ms']
        res['host_ms_forward_tiled_many'] = _host_ms(forms[0][1], reps)
        res['host_ms_forward_tiled_loop'] = _host_ms(forms[1][1], reps)
        ym, yt, yw = forms[0][1](), forms[1][1](), forms[2][1]()
        torch.cuda.synchronize()
        # bit identity holds between equal batches only: the one-image passes of a 16-window image are the same batches
        res['many_equals_tiled_loop_bitwise'] = all(_same(a, b) for a, b in zip(ym, yt))
        res['max_abs_diff_many_vs_forward'] = max((a - b).abs().max().item() for a, b in zip(ym, yw))
        res['max_abs_diff_tiled_loop_vs_forward'] = max((a - b).abs().max().item() for a, b in zip(yt, yw))
        res['plans'] = sorted(str(k[:4]) for k in net._plans)
    return res


def step_folder8(reps, warmup):
    return _set_step([(339, 510)] * 8, False, reps, warmup)


def step_small16(reps, warmup):
    return _set_step([(128, 128)] * 16, True, reps, warmup)


def step_bundled(reps, warmup):
    import numpy as np
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'sr_infer.npz'))
    sizes = [tuple(int(v) for v in g['lr_' + str(n)].shape[:2]) for n in sorted(str(n) for n in g['names'])]
    return _set_step(sizes, False, reps, warmup)


def step_kernels(reps, _warmup):
    """One pass of 16 windows of 128 x 128 (tile 96, pad 16) of a 339 x 510 image, tiles 0..15: the table-driven gather
    and stitch against esr_tile_op's, alternated, 50 back-to-back launches per sample."""
    import numpy as np
    import torch
    from esrganplus_amd import _lib as L, engine as E, functional as F
    dev = torch.device('cuda:0')
    H, W, tile, pad, S, N = 339, 510, 96, 16, 16, 50
    x = _images([(H, W)])[0]
    y = torch.zeros((1, 3, 4 * H, 4 * W), device=dev)
    g = E.G32(S, 3, 128, 128, PREC, dev)
    slots = torch.randn((S, 3, 512, 512), device=dev)
    rec = np.zeros(2 * S, dtype=F._tile_item_dtype())
    for s in range(S):
        rec[s] = (x.data_ptr(), H, W, s, 1)
        rec[S + s] = (y.data_ptr(), H, W, s, 1)
    table = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
    stream = C.c_void_p(E.current_stream())
    lib = L.lib()

    def many(to_g32):
        d = L.esr_tile_many()
        d.dtype, d.to_g32, d.C, d.tile, d.pad, d.scale = g.esr_dtype, to_g32, 3, tile, pad, 1 if to_g32 else 4
        d.th, d.tw, d.n_slots = 128, 128, S
        d.items = table.data_ptr() + (0 if to_g32 else S * 24)
        d.g32, d.slots_nchw = g.view(0, 3), slots.data_ptr()
        return lambda: L.check(lib.esr_tile_many_op(C.byref(d), stream), 'esr_tile_many_op')

    def one(to_g32):
        d = L.esr_tile()
        d.dtype, d.to_g32, d.B, d.C = g.esr_dtype, to_g32, 1, 3
        d.H, d.W = (H, W) if to_g32 else (4 * H, 4 * W)
        d.tile, d.pad, d.scale, d.t_begin, d.t_count = tile, pad, 1 if to_g32 else 4, 0, S
        d.nchw = (x if to_g32 else y).data_ptr()
        d.g32, d.slots_nchw = g.view(0, 3), slots.data_ptr()
        return lambda: L.check(lib.esr_tile_op(C.byref(d), stream), 'esr_tile_op')

    forms = [('many_gather', many(1)), ('tile_gather', one(1)), ('many_stitch', many(0)), ('tile_stitch', one(0))]
    res = _compare([(n, lambda f=f: [f() for _ in range(N)]) for n, f in forms], reps, 2)
    for n, _ in forms:
        for k in ('median_ms', 'min_ms', 'p90_ms'):
            res[n][k.replace('_ms', '_us_per_launch')] = 1e3 * res[n].pop(k) / N
    res['launches_per_sample'] = N
    res['bytes_gather'] = S * 128 * 128 * (3 * 4 + 32)          # fp32 read of 3 channels + one 32-byte group written
    res['bytes_stitch'] = 2 * 4 * 3 * 16 * sum((min((i + 1) * tile, H) - i * tile) * (min((j + 1) * tile, W) - j * tile)
                                                for i in range(4) for j in range(6) if i * 6 + j < S)
    return res


def run_step(step, reps, warmup):
    return globals()['step_' + step](reps, warmup)


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
        print('[tiled_many_probe] ' + json.dumps({a.step: run_step(a.step, a.reps, a.warmup)}), flush=True)
        return
    res = {}
    for step in STEPS:
        cmd = ['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__), '--step', step,
               '--reps', str(a.reps), '--warmup', str(a.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        line = next((l for l in r.stdout.splitlines() if l.startswith('[tiled_many_probe] ')), None)
        if r.returncode != 0 or line is None:            # a failed step ends the run: nothing more is started
            print(r.stdout[-2000:], r.stderr[-4000:], sep='\n')
            sys.exit('tiled_many_probe: step %s ended with status %d' % (step, r.returncode))
        res.update(json.loads(line[len('[tiled_many_probe] '):]))
        print(step, json.dumps(res[step]), flush=True)
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, 'w') as f:
                json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
