#!/usr/bin/env python
"""Pins the tiled x8 self-ensemble against the reference's own ``SRModel.test_x8`` (codes/models/SR_model.py:82-120) on an
image that the tiled form really cuts into windows: writes tests/golden/tiled_x8.npz.  Needs the reference checkout
(oracle.ref_import), CPU only:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_tiled_x8_golden.py

The route is tools/gen_x8_golden.py's: ``test_x8`` is called as an unbound function on a stand-in object that carries
what it reads.  Input and weights are regenerated from the recorded seeds and names (esrganplus_amd.synth), so the file
holds the output, the shape, the seeds and the names only."""
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np
import torch

from esrganplus_amd import synth
from gen_x8_golden import sr_model_class
from oracle import ref_import as RI

# weights: synth.rrdbnet_state_dict(NB, SD_SEED); input: synth.image_batch(X_SEED, *SHAPE, name=NAME)
NB, SD_SEED, X_SEED, SHAPE, NAME = 1, 81, 2, (1, 3, 45, 70), 'tiled'


def main():
    assert RI.available(), 'the reference checkout is needed (ESRGAN_REFERENCE)'
    SRModel = sr_model_class()
    net = RI.build_rrdbnet(NB, 'codes')
    net.load_state_dict(synth.rrdbnet_state_dict(nb=NB, seed=SD_SEED), strict=True)
    net.train()                                         # test_x8 switches to eval itself (and back)
    m = types.SimpleNamespace(netG=net, var_L=synth.image_batch(X_SEED, *SHAPE, name=NAME), device=torch.device('cpu'))
    SRModel.test_x8(m)
    assert net.training and tuple(m.fake_H.shape) == (1, 3, 4 * SHAPE[2], 4 * SHAPE[3])
    res = {'nb': np.int64(NB), 'sd_seed': np.int64(SD_SEED), 'x_seed': np.int64(X_SEED),
           'shape': np.array(SHAPE, dtype=np.int64), 'name': np.array(NAME),
           'y': m.fake_H.detach().numpy().astype(np.float32)}
    out = os.path.join(ROOT, 'tests', 'golden', 'tiled_x8.npz')
    np.savez_compressed(out, **res)
    print('done ->', out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
