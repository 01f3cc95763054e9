#!/usr/bin/env python
"""``train.SRGANStep`` against ``train.ESRGANPlusStep`` (profiles/srgan_step.md): the nb = 23 net in fp16 with loss scale
1024 on 16 x 32^2 LR per step (the reference's crop size), the pipelined form ``step(sync_log=False)``, synthetic weights
and data, the default weights of both steps (l1 pixel x 1e-2, l1 feature x 1, GAN x 5e-3).

A = ``ESRGANPlusStep``, B = ``SRGANStep`` ('vanilla', G moves every iteration), both in ONE process in the order
A1 - B - A2: the two A runs give the run-to-run spread the B figure is read against.  Each run: fresh networks, warm-up
steps, then one HIP event in front of the first timed step and one behind the last (``finish()`` first), enough steps
to pass a second; ms per step = their distance / steps, next to the host's wall time.  Every run is armed with its own
time limit (SIGALRM ends the process: nothing more is started on the GPU).  ``--serial`` appends A0: the yardstick with
ESR_TRAIN_OVERLAP=0, everything on one stream.

    python tools/srgan_step_probe.py [--steps 200] [--warmup 20] [--limit 120] [--serial] [--json out.json]"""
import argparse
import gc
import json
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

NB, BATCH, LR_SIZE = 23, 16, 32


def _nets(dev):
    from esrganplus_amd import architecture as arch, synth
    netG = arch.RRDBNet(3, 3, 64, NB).to(dev).train().set_precision('fp16')
    netD = arch.Discriminator_VGG_128(3, 64).to(dev).train().set_precision('fp16')
    netF = arch.VGGFeatureExtractor(34, False, True, dev).to(dev).eval().set_precision('fp16')
    netG.load_state_dict(synth.rrdbnet_state_dict(NB, 0, gain=0.5))
    netD.load_state_dict(synth.discriminator_state_dict(seed=1))
    netF.load_state_dict(synth.vgg19_state_dict(6, 34), strict=False)
    return netG, netD, netF


def measure(make_step, dev, steps, warmup, limit):
    from esrganplus_amd import synth
    signal.alarm(limit)                       # this run's own time limit
    netG, netD, netF = _nets(dev)
    st = make_step(netG, netD, netF)
    assert st._manual_ok()
    lr = synth.image_batch(400, BATCH, 3, LR_SIZE, LR_SIZE, name='probe.lr').to(dev)
    hr = synth.image_batch(500, BATCH, 3, 4 * LR_SIZE, 4 * LR_SIZE, name='probe.hr').to(dev)
    for _ in range(max(warmup, 1)):
        st.step(lr, hr, sync_log=False)
    st.finish()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(steps):
        log = st.step(lr, hr, sync_log=False)
    st.finish()
    e1.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / steps
    signal.alarm(0)
    assert all(bool(torch.isfinite(v)) for v in log.values())
    res = {'ms_per_step': e0.elapsed_time(e1) / steps, 'wall_ms_per_step': wall * 1e3, 'timed_s': wall * steps,
           'log': {k: float(v) for k, v in log.items()}}
    del st, netG, netD, netF
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--limit', type=int, default=120, help='seconds each run may take')
    ap.add_argument('--serial', action='store_true', help='append A0: ESRGANPlusStep under ESR_TRAIN_OVERLAP=0')
    ap.add_argument('--json')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the GPU'
    from esrganplus_amd import train
    dev = torch.device('cuda:0')
    esr = lambda G, D, F_: train.ESRGANPlusStep(G, D, F_, loss_scale=1024.0, data_parallel=False)
    srg = lambda G, D, F_: train.SRGANStep(G, D, F_, loss_scale=1024.0, data_parallel=False)
    runs = [('A1', esr, None), ('B', srg, None), ('A2', esr, None)]
    if a.serial:
        runs.append(('A0', esr, '0'))
    res = {'steps': a.steps, 'warmup': a.warmup, 'device': torch.cuda.get_device_name(0),
           'shape': '%dx%d^2 LR, nb %d, fp16' % (BATCH, LR_SIZE, NB)}
    for tag, make, overlap in runs:
        saved = os.environ.get('ESR_TRAIN_OVERLAP')
        if overlap is not None:
            os.environ['ESR_TRAIN_OVERLAP'] = overlap       # read by the step's constructor
        res[tag] = measure(make, dev, a.steps, a.warmup, a.limit)
        if overlap is not None:
            os.environ.pop('ESR_TRAIN_OVERLAP')
            if saved is not None:
                os.environ['ESR_TRAIN_OVERLAP'] = saved
        print(tag, json.dumps(res[tag]), flush=True)
    am = 0.5 * (res['A1']['ms_per_step'] + res['A2']['ms_per_step'])
    res['ratio_B_over_A'] = res['B']['ms_per_step'] / am
    res['A_spread_ms'] = abs(res['A1']['ms_per_step'] - res['A2']['ms_per_step'])
    print('| run | ms / step (HIP events) | ms / step (host wall) |\n|---|---|---|')
    for tag, _, _ in runs:
        print('| %s | %.3f | %.3f |' % (tag, res[tag]['ms_per_step'], res[tag]['wall_ms_per_step']))
    print('B / mean(A) = %.4f (expected <= 1.05); A spread %.3f ms' % (res['ratio_B_over_A'], res['A_spread_ms']))
    if a.json:
        json.dump(res, open(a.json, 'w'), indent=1)


if __name__ == '__main__':
    main()
