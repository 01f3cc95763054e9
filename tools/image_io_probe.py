#!/usr/bin/env python
"""8-bit image-in, image-out inference against the float path around it (profiles/image_io.md): the nb = 23 net with
synthetic weights, fp16, one device, tile 96, pad 16.  tools/tiled_many_probe.py's method: every step runs in a child
process of its own, under its own time limit, and one failed step ends the run.

* ``folder8``   8 seeded 339 x 510 uint8 images, decoded and in host memory: the per-image statements of
  ``tools/sr_infer.py --tile-many`` around ``forward_tiled_many`` (the float path) against those of ``--tile-u8`` around
  ``forward_images``.  Wall time per folder in four parts, a device synchronisation between them so that each part is
  what it says: host pre-processing, upload, device work, download plus host post-processing.  The two paths are
  alternated after a warm-up; median (min) of the repetitions.  Peak device memory of each path over what is allocated
  before it (weights and plans), and a check that both paths give the same uint8 images.
* ``bundled``   the same for the five LR images of tests/golden/sr_infer.npz.
* ``kernels``   the two new kernels on one pass of 16 x 128 x 128 windows of a 339 x 510 image next to
  ``esr_tile_many_op`` on the same windows: hipEvent time over 50 back-to-back launches, per launch.
Decoding and encoding the image files is the same in both paths and is not timed.

    python tools/image_io_probe.py [--reps 10] [--json out.json] [--limit 240]"""
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
TILE, PAD = 96, 16
STEPS = ['folder8', 'bundled', 'kernels']
PARTS = ('pre_ms', 'upload_ms', 'device_ms', 'down_post_ms')


def _net():
    import torch
    from esrganplus_amd import architecture as arch, synth
    net = arch.RRDBNet(3, 3, 64, 23).to(torch.device('cuda:0')).eval()
    net.load_state_dict(synth.rrdbnet_state_dict(23, 0), strict=True)
    net.max_cached_plans = 16
    return net.set_precision(PREC)


def _float_path(net, arrs, dev):
    """--tile-many's statements -> (uint8 HWC arrays, the four wall times in ms)."""
    import numpy as np
    import torch
    t = [time.perf_counter()]
    host = [torch.from_numpy(np.transpose(a.astype(np.float64) / 255, (2, 0, 1))).float().unsqueeze(0) for a in arrs]
    t.append(time.perf_counter())
    xs = [h.to(dev) for h in host]
    torch.cuda.synchronize()
    t.append(time.perf_counter())
    ys = net.forward_tiled_many(xs, TILE, PAD)
    torch.cuda.synchronize()
    t.append(time.perf_counter())
    outs = [y.data.squeeze().float().cpu().clamp_(0, 1).numpy() for y in ys]
    outs = [(np.transpose(o, (1, 2, 0)) * 255.0).round().astype(np.uint8) for o in outs]
    t.append(time.perf_counter())
    return outs, [1e3 * (b - a) for a, b in zip(t, t[1:])]


def _u8_path(net, arrs, dev):
    """--tile-u8's statements -> (uint8 HWC arrays, the four wall times in ms)."""
    import torch
    t = [time.perf_counter()]
    host = [torch.from_numpy(a) for a in arrs]
    t.append(time.perf_counter())
    xs = [h.to(dev) for h in host]
    torch.cuda.synchronize()
    t.append(time.perf_counter())
    ys = net.forward_images(xs, TILE, PAD)
    torch.cuda.synchronize()
    t.append(time.perf_counter())
    outs = [y.cpu().numpy() for y in ys]
    t.append(time.perf_counter())
    return outs, [1e3 * (b - a) for a, b in zip(t, t[1:])]


def _folder_step(arrs, reps, warmup):
    import numpy as np
    import torch
    dev = torch.device('cuda:0')
    net = _net()
    paths = [('float', _float_path), ('u8', _u8_path)]
    res = {'sizes': [list(a.shape[:2]) for a in arrs], 'lr_pixels': int(sum(a.shape[0] * a.shape[1] for a in arrs)),
           'torch_threads': torch.get_num_threads()}
    with torch.no_grad():
        outs = {}
        for name, fn in paths:
            for _ in range(warmup):
                outs[name] = fn(net, arrs, dev)[0]
        res['same_uint8_images'] = all(np.array_equal(a, b) for a, b in zip(outs['float'], outs['u8']))
        del outs
        ms = {name: [] for name, _ in paths}
        for _ in range(reps):                            # alternated: both paths see the same clocks and host load
            for name, fn in paths:
                ms[name].append(fn(net, arrs, dev)[1])
        for name, _ in paths:
            a = np.array(ms[name])
            res[name] = {k: {'median': float(np.median(a[:, i])), 'min': float(a[:, i].min())} for i, k in enumerate(PARTS)}
            tot = a.sum(1)
            res[name]['total_ms'] = {'median': float(np.median(tot)), 'min': float(tot.min())}
        for name, fn in paths:                           # peak device memory of one folder over weights and plans
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            fn(net, arrs, dev)
            torch.cuda.synchronize()
            res[name]['peak_bytes_over_base'] = int(torch.cuda.max_memory_allocated() - base)
            res[name]['base_bytes'] = int(base)
    res['n'] = reps
    return res


def step_folder8(reps, warmup):
    import numpy as np
    rng = np.random.RandomState(20241020)
    return _folder_step([rng.randint(0, 256, (339, 510, 3)).astype(np.uint8) for _ in range(8)], reps, warmup)


def step_bundled(reps, warmup):
    import numpy as np
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'sr_infer.npz'))
    return _folder_step([np.ascontiguousarray(g['lr_' + n]) for n in sorted(str(n) for n in g['names'])], reps, warmup)


def step_kernels(_reps, _warmup):
    """One pass of 16 windows of 128 x 128 (tile 96, pad 16) of a 339 x 510 image, tiles 0..15: esr_tile_img_op's gather
    and stitch against esr_tile_many_op's, alternated, 50 back-to-back launches per sample, 20 samples."""
    import numpy as np
    import torch
    from esrganplus_amd import _lib as L, engine as E, functional as F
    dev = torch.device('cuda:0')
    H, W, S, N = 339, 510, 16, 50
    x8 = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev)
    xf = torch.rand((1, 3, H, W), device=dev)
    y8 = torch.zeros((4 * H, 4 * W, 3), dtype=torch.uint8, device=dev)
    yf = torch.zeros((1, 3, 4 * H, 4 * W), device=dev)
    g = E.G32(S, 3, 128, 128, PREC, dev)
    slots = torch.randn((S, 3, 512, 512), device=dev) * 0.6 + 0.5
    rec = np.zeros(4 * S, dtype=F._tile_item_dtype())
    for k, t in enumerate((xf, yf, x8, y8)):
        for s in range(S):
            rec[k * S + s] = (t.data_ptr(), H, W, s, 1)
    table = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
    stream = C.c_void_p(E.current_stream())
    lib = L.lib()

    def op(img, to_g32):
        d = L.esr_tile_img() if img else L.esr_tile_many()
        d.dtype, d.to_g32, d.C, d.tile, d.pad, d.scale = g.esr_dtype, to_g32, 3, TILE, PAD, 1 if to_g32 else 4
        d.th, d.tw, d.n_slots = 128, 128, S
        d.items = table.data_ptr() + ((2 if img else 0) + (0 if to_g32 else 1)) * S * 24
        d.g32, d.slots_nchw = g.view(0, 3), slots.data_ptr()
        name = 'esr_tile_img_op' if img else 'esr_tile_many_op'
        return lambda: L.check(getattr(lib, name)(C.byref(d), stream), name)

    forms = [('img_gather', op(1, 1)), ('many_gather', op(0, 1)), ('img_stitch', op(1, 0)), ('many_stitch', op(0, 0))]
    ms = {n: [] for n, _ in forms}
    for rep in range(22):
        for n, f in forms:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(N):
                f()
            b.record()
            torch.cuda.synchronize()
            if rep >= 2:
                ms[n].append(1e3 * a.elapsed_time(b) / N)
    res = {n: {'median_us_per_launch': float(np.median(v)), 'min_us_per_launch': float(min(v)),
               'p90_us_per_launch': float(np.percentile(v, 90)), 'n': len(v)} for n, v in ms.items()}
    owned = sum((min((i + 1) * TILE, H) - i * TILE) * (min((j + 1) * TILE, W) - j * TILE)
                for i in range(4) for j in range(6) if i * 6 + j < S)
    res['launches_per_sample'] = N
    res['bytes_gather'] = {'img': S * 128 * 128 * (3 + 32), 'many': S * 128 * 128 * (12 + 32)}
    res['bytes_stitch'] = {'img': 16 * owned * (12 + 3), 'many': 16 * owned * (12 + 12)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--json', default=None)
    ap.add_argument('--limit', type=int, default=240, help='seconds per step')
    ap.add_argument('--step', default=None, help='run this one step in this process and print its JSON line')
    a = ap.parse_args()
    if a.step:
        print('[image_io_probe] ' + json.dumps({a.step: globals()['step_' + a.step](a.reps, a.warmup)}), flush=True)
        return
    res = {}
    for step in STEPS:
        cmd = ['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__), '--step', step,
               '--reps', str(a.reps), '--warmup', str(a.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        line = next((l for l in r.stdout.splitlines() if l.startswith('[image_io_probe] ')), None)
        if r.returncode != 0 or line is None:            # a failed step ends the run: nothing more is started
            print(r.stdout[-2000:], r.stderr[-4000:], sep='\n')
            sys.exit('image_io_probe: step %s ended with status %d' % (step, r.returncode))
        res.update(json.loads(line[len('[image_io_probe] '):]))
        print(step, json.dumps(res[step]), flush=True)
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, 'w') as f:
                json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
