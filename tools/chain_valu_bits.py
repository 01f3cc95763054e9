#!/usr/bin/env python3
"""SHA-256 of what the fp16 dense-block chains store for cases a and d of tests/test_gpu_chain_valu.py:

    python tools/chain_valu_bits.py [out.json]

  a  one RRDB (3 dense blocks) at (1, 64, 48, 96), 16-row tiles: the regular chain's output and the general chain's
  d  training forward + backward of an RRDB at (2, 64, 32, 32), noise off and on, 4-row and 16-row tiles: every buffer
     of the plan the chains write (the saved slices S, the gradient slices Q, the block exits), halo rings included

Run from two trees (a parent and a change of csrc/rdb_chain_kernel.h) the two lists are equal exactly when the chains
store the same bits.  One JSON object {name: digest}; also written to out.json when given."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


def main(argv):
    from tests import chain_stage_refs as R
    from tests import test_gpu_chain_stages as ST
    from tests.test_gpu_chain_variants import Chain
    dev = torch.device('cuda:0')
    out = {}
    os.environ['ESR_RDB_ROWS'] = '4'
    mod = R.block_module('rrdb').to(dev).eval().set_precision('fp16')
    x = R.randn((1, 64, 48, 96), 161).to(dev)
    c = Chain(mod, 1, 48, 96, dev)
    out['a.regular'] = digest(c.run(x)[0])
    out['a.general'] = digest(c.run(x, general=True)[0])
    from esrganplus_amd import _lib as L
    L.lib().esr_debug_chain_force_general(-1)
    os.environ['ESR_RDB_TRAIN_CHAIN'] = '1'
    for kind, train in (('rrdb', False), ('rrdb_ti', True)):
        for rows in (None, '4'):
            if rows is None:
                os.environ.pop('ESR_RDB_ROWS', None)
            else:
                os.environ['ESR_RDB_ROWS'] = rows
            m = R.block_module(kind).to(dev).train(train).set_precision('fp16')
            bld = ST.build(m, 'rrdb', 64, 64, 2, 32, 32, dev, train)
            ST.step(bld, R.randn((2, 64, 32, 32), 164).to(dev), R.randn((2, 64, 32, 32), 165).to(dev), train)
            tag = 'd.%s.rows%s' % ('noise' if train else 'plain', rows or 'auto')
            for j in range(3):
                out['%s.S%d' % (tag, j)] = digest(bld.S[0][j].t)
                out['%s.exit%d' % (tag, j)] = digest(bld.block_exit(0, j).dst.t)
            for n, q in enumerate(bld.Qs):
                out['%s.Q%d' % (tag, n)] = digest(q.t)
            out['%s.XF' % tag] = digest(bld.XF.t)
    print(json.dumps(out, indent=1))
    if argv:
        with open(argv[0], 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main(sys.argv[1:])
