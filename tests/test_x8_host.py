"""x8 self-ensemble, host side: the pure-torch restatement against the reference's own ``SRModel.test_x8`` (pinned in
tests/golden/x8.npz by tools/gen_x8_golden.py), the transform table, and the ctypes mirror of the new op."""
import ctypes as C

import numpy as np
import pytest
import torch

from esrganplus_amd import functional as F
from esrganplus_amd import synth

CASES = ('a', 'b', 'c')


def x8_case(g, tag):
    """(nb, state dict, input) of one pinned case, regenerated from the recorded seeds and names."""
    nb, shape = int(g[tag + '_nb']), tuple(int(v) for v in g[tag + '_shape'])
    sd = synth.rrdbnet_state_dict(nb=nb, seed=int(g['sd_seed']) + nb)
    return nb, sd, synth.image_batch(int(g['x_seed']), *shape, name=str(g[tag + '_name']))


@pytest.mark.parametrize('tag', CASES)
def test_x8_reference_matches_the_references_test_x8(golden, tag):
    from oracle import ref_torch as RT
    g = golden('x8')
    nb, sd, x = x8_case(g, tag)
    with torch.no_grad():
        y = F.x8_reference(lambda t: RT.rrdbnet_forward(t, sd, nb), x)
    err = np.abs(y.numpy() - g[tag + '_y']).max()
    print('x8_reference vs test_x8 [%s]: max abs %.3e' % (tag, err))
    assert y.shape == g[tag + '_y'].shape
    assert err <= 2e-6            # the bound of tests/test_oracle.py::test_rrdbnet_small forwards


@pytest.mark.parametrize('shape', [(2, 3, 5, 7), (1, 2, 6, 6), (1, 1, 1, 9)])
def test_transform_table(shape):
    """R_k(T_k(src)) == src for every k, the slot sizes, and the index maps of include/esrgan_hip.h spelled out."""
    src = synth.normal_like(5, 'x8.table', shape)
    H, W = shape[2:]
    for k in range(8):
        t = F.x8_transform(src, k)
        assert tuple(t.shape[2:]) == ((W, H) if k & 4 else (H, W))
        assert torch.equal(F.x8_inverse(t, k), src)
        ys = [H - 1 - i if k & 2 else i for i in range(H)]
        xs = [W - 1 - j if k & 1 else j for j in range(W)]
        want = src[:, :, ys][:, :, :, xs]                    # want[y][x] = src[ys(y)][xs(x)]
        assert torch.equal(t, want.transpose(2, 3) if k & 4 else want)
        # the inverse uses the same map: R_k(o)[y][x] = o[ys(y)][xs(x)]  /  o[xs(x)][ys(y)]
        o = synth.normal_like(6, 'x8.table.o%d' % k, tuple(t.shape))
        oo = o.transpose(2, 3) if k & 4 else o
        assert torch.equal(F.x8_inverse(o, k), oo[:, :, ys][:, :, :, xs])


def test_x8_reference_is_per_image():
    x = synth.image_batch(9, 2, 3, 4, 6, name='x8.perimage')
    fn = lambda t: t * 2.0 + t.roll(1, 3)                    # not equivariant: the transforms matter
    both = F.x8_reference(fn, x)
    for b in range(2):
        assert torch.equal(both[b:b + 1], F.x8_reference(fn, x[b:b + 1]))


def test_lib_mirrors_the_dihedral_op():
    from esrganplus_amd import _lib as L
    assert L.OP_DIHEDRAL == 15
    assert 'esr_dihedral_op' in L.EXPORTS
    names = [f[0] for f in L.esr_dihedral._fields_]
    assert names == ['dtype', 'to_g32', 'B', 'C', 'H', 'W', 'nchw', 'g32', 'k_begin', 'k_count', 'accumulate', 'scale',
                     'slots_nchw']
    assert C.sizeof(L.esr_dihedral) == 24 + 8 + C.sizeof(L.esr_g32) + 16 + 8
    assert 'dihedral' in [f[0] for f in L._op_union._fields_]
    assert C.sizeof(L.esr_dihedral) <= C.sizeof(L.esr_conv)  # the union, and with it sizeof(esr_op), did not grow
    lib = L.lib()                                            # loads the library: symbol present, sizeof(esr_op) agrees
    assert lib.esr_abi_version() == 6
    assert hasattr(lib, 'esr_dihedral_op')
