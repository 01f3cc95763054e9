#!/usr/bin/env python
"""Scoring a generator from HR images alone, against the only route there was without it (profiles/hr_only_eval.md): the
nb = 23 net with synthetic weights, fp16, one device, 8 HR images of 1356 x 2040 (LR 339 x 510: 24 windows of 128 x 128
each at tile 96, pad 16, 12 passes of 16).  The two routes alternate in one process after a warm-up, each repetition
hipEvent-timed and followed by a synchronisation (median / min / p90 of >= 20).  Report only: nothing is a gate.

* route A   ``net.evaluate_hr_images(hr, bgr=True)`` on the uint8 HWC device images: the LR is made in the gather.
* route B   what the functions without it allow: per image uint8 -> float CHW (a true division, through the 256-entry
  table of ``functional.images_reference``), ``data.imresize(x, 1 / 4)``; ``net.forward_tiled_many`` on the float LR
  images, ``metrics.device_tensor2img`` per result, ``metrics.device_set_metrics``.

Recorded per route: the time of a whole call, the host time of a call (entry to return, the device idle at entry), the
launches of the library per call (C entries and the ops of every plan run) and the torch kernels of route B's
conversions, the peak of device memory over what is resident before the call (weights, plans, the HR images), and whether
the two routes' bytes and tables agree.  The ends alone: one pass of 16 windows through ``esr_tile_hr_op``'s gather and
through ``esr_tile_img_op``'s gather on the stored LR image, hipEvent time per launch over 50 launches.

    python tools/hr_eval_probe.py [--reps 20] [--json out.json] [--md profiles/hr_only_eval.md]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PREC, NB, TILE, PAD, S = 'fp16', 23, 96, 16, 16
HR_SIZE, N_IMAGES = (1356, 2040), 8


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


def _peak_mb(fn):
    """Peak of allocated device memory during one call over what was allocated at its entry, in MB."""
    import torch
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    y = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    del y
    return (peak - base) / 1e6


def _gather_us(net, hr, n=50):
    """One pass of 16 windows of image 0: (esr_tile_hr_op's gather, esr_tile_img_op's gather on the stored LR) in us."""
    import numpy as np
    import torch
    from esrganplus_amd import _lib as L, data as D, engine as E, functional as F, metrics as M
    dev = hr[0].device
    x = hr[0]
    H, W = x.shape[0] // 4, x.shape[1] // 4
    th = tw = TILE + 2 * PAD
    lut = (torch.arange(256, dtype=torch.float32) / 255.0).to(dev)
    lr8 = M.device_tensor2img(D.imresize(lut[x.flip(2).permute(2, 0, 1).long()], 0.25))       # the stored 8-bit LR
    (wy, iy, _), (wx, ix, _) = D.device_tables(4 * H, 0.25, dev), D.device_tables(4 * W, 0.25, dev)
    items = np.zeros(S, dtype=F._tile_item_dtype())
    desc = np.zeros(1, dtype=F._hr_desc_dtype())
    desc[0] = (x.data_ptr(), wy.data_ptr(), iy.data_ptr(), wx.data_ptr(), ix.data_ptr(), x.shape[1], 4 * H, 4 * W,
               wy.shape[1], wx.shape[1], 0)
    table = torch.empty(items.nbytes + desc.nbytes, dtype=torch.uint8, device=dev)
    for k in range(S):
        items[k] = (table.data_ptr() + items.nbytes, H, W, k, 1)
    table.copy_(torch.from_numpy(np.concatenate([items.view(np.uint8), desc.view(np.uint8)])))
    items['nchw'] = lr8.data_ptr()
    table8 = torch.from_numpy(items.view(np.uint8).copy()).to(dev)
    g = E.G32(S, 3, th, tw, PREC, dev)
    out = []
    for st, name, tab in ((L.esr_tile_hr(), 'esr_tile_hr_op', table), (L.esr_tile_img(), 'esr_tile_img_op', table8)):
        st.dtype, st.to_g32, st.C, st.tile, st.pad, st.scale = g.esr_dtype, 1, 3, TILE, PAD, 1
        st.th, st.tw, st.n_slots, st.bgr, st.items, st.g32 = th, tw, S, 1, tab.data_ptr(), g.view(0, 3)
        call = lambda: L.check(getattr(L.lib(), name)(C.byref(st), C.c_void_p(E.current_stream())), name)
        call()
        out.append(1e3 * _timed(lambda: [call() for _ in range(n)]) / n)
    return out


def run(reps, warmup):
    import torch
    from esrganplus_amd import architecture as arch, data as D, functional as F, metrics as M, synth
    dev = torch.device('cuda:0')
    net = arch.RRDBNet(3, 3, 64, NB).to(dev).eval()
    net.load_state_dict(synth.rrdbnet_state_dict(NB, 0), strict=True)
    net.max_cached_plans = 16
    net.set_precision(PREC)
    g = torch.Generator().manual_seed(1)
    hr = [torch.randint(0, 256, HR_SIZE + (3,), generator=g, dtype=torch.uint8).to(dev) for _ in range(N_IMAGES)]
    lut = (torch.arange(256, dtype=torch.float32) / 255.0).to(dev)

    def route_a():
        return net.evaluate_hr_images(hr, TILE, PAD, S, bgr=True)

    def route_b():
        lrs = [D.imresize(lut[x.flip(2).permute(2, 0, 1).long()], 0.25) for x in hr]
        sr = [M.device_tensor2img(y) for y in net.forward_tiled_many(lrs, TILE, PAD, S)]
        return sr, M.device_set_metrics(sr, hr, 4, True)

    res = {}
    with torch.no_grad():
        forms = [('A_evaluate_hr_images', route_a), ('B_composition', route_b)]
        for _, fn in forms:
            for _ in range(warmup):
                fn()
        ms = {name: [] for name, _ in forms}
        for _ in range(reps):                            # interleaved: every route sees the same clocks
            for name, fn in forms:
                ms[name].append(_timed(fn))
        for name, fn in forms:
            res[name] = _stats(ms[name])
            res[name]['host_ms'] = _host_ms(fn, reps)
            res[name]['peak_mb'] = _peak_mb(fn)
        (sa, ra), (sb, rb) = route_a(), route_b()
        torch.cuda.synchronize()
        res['bytes_agree'] = all(torch.equal(a, b) for a, b in zip(sa, sb))
        res['tables_agree'] = bool((ra.read() == rb.read()).all())
        res['averages'] = list(ra.averages())
        sizes = [(x.shape[0] // 4, x.shape[1] // 4) for x in hr]
        passes = sum(len(p) for _, _, _, p in F.tiled_many_passes(sizes, TILE, PAD, S))
        ops = {k[0]: len(v.plan.ops.ops) for k, v in net._plans.items()}
        res['passes'], res['plan_ops'] = passes, ops
        # C entries of the library per call: every plan run's ops, the set metric's one entry (two launches), and in
        # route B two resample passes and one tensor2img per image; torch kernels of B's conversions per image: flip,
        # the copy to int64 (with the permutation) and the table look-up
        res['A_evaluate_hr_images']['library_launches'] = passes * ops['tiled_hr'] + 2
        res['B_composition']['library_launches'] = passes * ops['tiled_many'] + 2 + 3 * len(hr)
        res['B_composition']['torch_kernels'] = 3 * len(hr)
        res['A_evaluate_hr_images']['torch_kernels'] = 0
        res['gather_us'] = dict(zip(('tile_hr', 'tile_img'), _gather_us(net, hr)))
        res['ratio_A_over_B'] = res['A_evaluate_hr_images']['median_ms'] / res['B_composition']['median_ms']
    return res


def _markdown(r, reps):
    f = lambda s: '%.2f / %.2f / %.2f' % (s['median_ms'], s['min_ms'], s['p90_ms'])
    a, b = r['A_evaluate_hr_images'], r['B_composition']
    rows = ['# Scoring from HR images alone: `evaluate_hr_images` against the composition of the existing functions', '',
            'Written by `tools/hr_eval_probe.py` (nb = %d, synthetic weights, %s, one MI355X, one process, the routes' % (NB, PREC),
            'alternating, %d repetitions each, hipEvent time of a whole call; median / min / p90 in ms).  %d HR images of' % (reps, N_IMAGES),
            '%d x %d, tile %d, pad %d, %d windows per pass: %d passes.  Report only.' % (HR_SIZE + (TILE, PAD, S, r['passes'])), '',
            'Route A: `evaluate_hr_images(hr, bgr=True)`.  Route B: per image uint8 -> float CHW (table look-up), `data.imresize`;',
            '`forward_tiled_many`, `device_tensor2img` per result, `device_set_metrics`.', '',
            '| route | whole call | host ms | library launches | torch kernels | peak MB over resident |', '|---|---|---|---|---|---|',
            '| A | %s | %.2f | %d | %d | %.1f |' % (f(a), a['host_ms'], a['library_launches'], a['torch_kernels'], a['peak_mb']),
            '| B | %s | %.2f | %d | %d | %.1f |' % (f(b), b['host_ms'], b['library_launches'], b['torch_kernels'], b['peak_mb']), '',
            'A / B, median of a whole call: %.4f.  The two routes\' bytes agree: %s; their tables agree: %s (averages %s).'
            % (r['ratio_A_over_B'], r['bytes_agree'], r['tables_agree'], ', '.join('%.6f' % v for v in r['averages'])), '',
            'The ends alone, one pass of %d windows of 128 x 128 (hipEvent time per launch over 50 launches): the new gather' % S,
            '(`esr_tile_hr_op`) %.1f us, `esr_tile_img_op`\'s gather on the stored 8-bit LR %.1f us.  A pass of the nb = %d plan takes'
            % (r['gather_us']['tile_hr'], r['gather_us']['tile_img'], NB),
            'about %.1f ms, so the gather is %.2f %% of it.  What bounds the gather: every LR pixel of the H pass reads taps_y'
            % (a['median_ms'] / r['passes'], 100 * r['gather_us']['tile_hr'] / (1e3 * a['median_ms'] / r['passes'])),
            '(16) weights, indices and HR bytes per channel triple, and a 16 x 16 tile stages up to 77 columns where it writes 16:',
            '4.8 H-pass sums per LR pixel against one W-pass sum; the table reads per tap are not hoisted.  Not tuned here.', '',
            'Not measured: fp32, other window counts, the upload of the images from the host, more than one box.  One box, one',
            'session: the absolute times carry that box\'s clocks; the ratios are the result.', '']
    return '\n'.join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--json', default=None)
    ap.add_argument('--md', default=None, help='write the table there (profiles/hr_only_eval.md)')
    a = ap.parse_args()
    assert a.reps >= 20
    res = run(a.reps, a.warmup)
    print(json.dumps(res), flush=True)
    for path, text in ((a.json, json.dumps(res, indent=1)), (a.md, _markdown(res, a.reps))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, 'w') as f:
                f.write(text)


if __name__ == '__main__':
    main()
