#!/usr/bin/env python
"""Pins the geometric self-ensemble against the reference's own ``SRModel.test_x8`` (codes/models/SR_model.py:82-120):
writes tests/golden/x8.npz.  Needs the reference checkout (oracle.ref_import), CPU only:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_x8_golden.py

``test_x8`` is called as an unbound function on a stand-in object that carries what it reads — ``netG``, ``var_L``,
``device`` — and receives its ``fake_H``.  Inputs and weights are regenerated from the recorded seeds and names
(esrganplus_amd.synth), so the file holds the outputs, the shapes, the seeds and the names only."""
import importlib
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from esrganplus_amd import synth
from oracle import ref_import as RI

# (tag, nb, (B, C, H, W)); weights: synth.rrdbnet_state_dict(nb, SD_SEED + nb); input: synth.image_batch(X_SEED, ..., 'x8.x.<tag>')
CASES = (('a', 2, (1, 3, 13, 21)), ('b', 1, (1, 3, 16, 16)), ('c', 1, (1, 3, 33, 20)))
SD_SEED, X_SEED = 80, 8


def sr_model_class():
    """codes/models/SR_model.py of the reference.  Its module-level imports (models.networks -> the whole model zoo) are
    not needed by test_x8: ``models.networks`` is stood in for by an empty module while SR_model is imported."""
    RI.codes_arch()                                     # puts <reference>/codes on sys.path, stubs torchvision
    saved = sys.modules.get('models.networks')
    sys.modules['models.networks'] = types.ModuleType('models.networks')
    try:
        mod = importlib.import_module('models.SR_model')
    finally:
        if saved is None:
            sys.modules.pop('models.networks', None)
        else:
            sys.modules['models.networks'] = saved
    return mod.SRModel


def main():
    assert RI.available(), 'the reference checkout is needed (ESRGAN_REFERENCE)'
    SRModel = sr_model_class()
    res = {'sd_seed': np.int64(SD_SEED), 'x_seed': np.int64(X_SEED), 'tags': np.array([c[0] for c in CASES])}
    for tag, nb, shape in CASES:
        net = RI.build_rrdbnet(nb, 'codes')
        net.load_state_dict(synth.rrdbnet_state_dict(nb=nb, seed=SD_SEED + nb), strict=True)
        net.train()                                     # test_x8 switches to eval itself (and back)
        m = types.SimpleNamespace(netG=net, var_L=synth.image_batch(X_SEED, *shape, name='x8.x.' + tag),
                                  device=torch.device('cpu'))
        SRModel.test_x8(m)
        assert net.training and tuple(m.fake_H.shape) == (1, 3, 4 * shape[2], 4 * shape[3])
        res[tag + '_nb'] = np.int64(nb)
        res[tag + '_shape'] = np.array(shape, dtype=np.int64)
        res[tag + '_name'] = np.array('x8.x.' + tag)
        res[tag + '_y'] = m.fake_H.detach().numpy().astype(np.float32)
        print('[gen_x8_golden]', tag, nb, shape, '->', tuple(m.fake_H.shape))
    out = os.path.join(ROOT, 'tests', 'golden', 'x8.npz')
    np.savez_compressed(out, **res)
    print('done ->', out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
