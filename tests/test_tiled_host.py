"""Tiled inference, host side: the geometry contract of include/esrgan_hip.h (esr_tile) over a sweep of image sizes,
tiles and pads, the pure-torch ``tiled_reference`` against the whole-image forward of the CPU oracle, and the ctypes
mirror of the new op."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from esrganplus_amd import functional as F
from esrganplus_amd import synth

SIZES = (1, 13, 24, 33, 45, 70)


@pytest.mark.parametrize('tile,pad', list(itertools.product((1, 16, 32), (0, 4, 19))))
def test_geometry_partitions_the_image_and_keeps_the_margin(tile, pad):
    for H, W in itertools.product(SIZES, SIZES):
        th, tw, ny, nx, tiles = F.tiled_geometry(H, W, tile, pad)
        assert (th, tw) == (min(tile + 2 * pad, H), min(tile + 2 * pad, W))
        assert (ny, nx) == (-(-H // tile), -(-W // tile)) and len(tiles) == ny * nx
        owned = np.zeros((H, W), dtype=np.int32)
        for t, (y0, y1, x0, x1, wy, wx) in enumerate(tiles):
            i, j = divmod(t, nx)
            assert (y0, x0) == (i * tile, j * tile) and y0 < y1 <= H and x0 < x1 <= W
            owned[y0:y1, x0:x1] += 1
            # the window lies inside the image and holds the owned rectangle ...
            assert 0 <= wy and wy + th <= H and 0 <= wx and wx + tw <= W
            assert wy <= y0 and y1 <= wy + th and wx <= x0 and x1 <= wx + tw
            # ... and an edge of it that is not an image edge is at least `pad` away from every owned pixel: `pad`
            # whole pixels between the owned range and the edge
            for lo, hi, w0, win, n in ((y0, y1, wy, th, H), (x0, x1, wx, tw, W)):
                assert w0 == 0 or lo - w0 >= pad, (H, W, t)
                assert w0 + win == n or w0 + win - hi >= pad, (H, W, t)
        assert (owned == 1).all(), (H, W)


def test_tiled_reference_is_the_whole_image_forward_with_enough_margin():
    from oracle import ref_torch as RT
    nb = 1
    sd = synth.rrdbnet_state_dict(nb=nb, seed=81)
    x = synth.image_batch(2, 1, 3, 24, 40, name='tiled')
    fn = lambda t: RT.rrdbnet_forward(t, sd, nb)
    with torch.no_grad():
        whole = fn(x)
        exact = F.tiled_reference(fn, x, 16, 15 * nb + 4, 4)
        none = F.tiled_reference(fn, x, 16, 0, 4)
    e_exact, e_none = (exact - whole).abs().max().item(), (none - whole).abs().max().item()
    print('tiled_reference vs whole image, tile 16: pad 19 %.3e, pad 0 %.3e (output abs-max %.3f)'
          % (e_exact, e_none, whole.abs().max().item()))
    assert exact.shape == whole.shape
    assert e_exact <= 1e-6
    assert e_none > 1e-2
    # at 24 x 40 the window of pad 19 is the whole image; 45 x 70 has windows of 45 x 54 that really cut it
    x = synth.image_batch(2, 1, 3, 45, 70, name='tiled')
    with torch.no_grad():
        whole = fn(x)
        errs = [(F.tiled_reference(fn, x, 16, pad) - whole).abs().max().item() for pad in (19, 0)]
    print('the same on 45 x 70: pad 19 %.3e, pad 0 %.3e' % tuple(errs))
    assert errs[0] <= 1e-6 and errs[1] > 1e-2


def test_tiled_reference_passes_and_argument_checks():
    """``fn`` always sees P B windows of one shape, a tail pass included, and the result does not depend on P for a
    per-sample ``fn``."""
    x = synth.image_batch(3, 2, 3, 13, 21, name='tiled.args')
    seen = []

    def fn(t):
        seen.append(tuple(t.shape))
        return torch.nn.functional.interpolate(t, scale_factor=4, mode='nearest')

    want = fn(x)
    for P in (1, 2, 5, None):
        del seen[:]
        assert torch.equal(F.tiled_reference(fn, x, 8, 2, P), want)
        n = min(6 if P is None else P, 6)                     # 2 x 3 tiles, default P = 16 // B = 8
        assert seen == [(n * 2, 3, 12, 12)] * -(-6 // n)
    for bad in (dict(tile=0), dict(pad=-1), dict(tiles_per_pass=0), dict(tile=2.5), dict(pad=None), dict(tile=True)):
        kw = dict(tile=8, pad=2, tiles_per_pass=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            F.tiled_reference(fn, x, **kw)


def test_lib_mirrors_the_tile_op():
    from esrganplus_amd import _lib as L
    assert L.OP_TILE == 16
    assert 'esr_tile_op' in L.EXPORTS
    names = [f[0] for f in L.esr_tile._fields_]
    assert names == ['dtype', 'to_g32', 'B', 'C', 'H', 'W', 'tile', 'pad', 'scale', 't_begin', 't_count', 'nchw', 'g32',
                     'slots_nchw']
    assert 'tile' in [f[0] for f in L._op_union._fields_]
    assert C.sizeof(L.esr_tile) <= C.sizeof(L.esr_conv)       # the union, and with it sizeof(esr_op), did not grow
    lib = L.lib()                                             # loads the library: symbol present, sizeof(esr_op) agrees
    assert lib.esr_abi_version() == 6
    assert hasattr(lib, 'esr_tile_op')
