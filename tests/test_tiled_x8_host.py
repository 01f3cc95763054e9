"""Tiled x8 self-ensemble, host side: the pure-torch ``tiled_x8_reference`` against the composition of the two existing
restatements (``tiled_reference`` over ``x8_reference``), against the whole-image ensemble of the CPU oracle, and the
ctypes mirror of the new op."""
import ctypes as C

import pytest
import torch

from esrganplus_amd import functional as F
from esrganplus_amd import synth

# (LR shape, tile, pad, tiles per pass)
CASE_A = ((1, 3, 40, 52), 16, 4, 5)       # 3 x 4 tiles of square 24 x 24 windows: 8 slots a pass; the last pass has 2 tiles
CASE_B = ((2, 3, 33, 70), 32, 8, 4)       # 2 x 3 tiles of 33 x 48 windows: two shapes of 4 slots; the last tile row owns 1 row


def _ramp_fn(seen=None):
    """Per-sample and not equivariant under any flip or transpose: nearest x4 plus a ramp over the OUTPUT position.
    With inputs on a 1/64 grid every value is a small dyadic number, so fp32 sums of eight of them are exact."""
    def fn(t):
        if seen is not None:
            seen.append(tuple(t.shape))
        y = torch.nn.functional.interpolate(t, scale_factor=4, mode='nearest')
        ry = torch.arange(y.shape[2], dtype=torch.float32).view(1, 1, -1, 1) / 64
        rx = torch.arange(y.shape[3], dtype=torch.float32).view(1, 1, 1, -1) / 1024
        return y + ry + rx
    return fn


def _dyadic_image(seed, shape, name):
    return torch.round(synth.image_batch(seed, *shape, name=name) * 64) / 64


@pytest.mark.parametrize('case,pairs', [(CASE_A, [(5, 8), (5, None), (1, 4), (12, 2), (None, 1), (7, 8)]),
                                        (CASE_B, [(4, 4), (4, None), (4, 8), (1, 2), (None, 1), (6, 4)])])
def test_tiled_x8_reference_is_tiled_reference_over_x8_reference(case, pairs):
    shape, tile, pad, _ = case
    B, C_, H, W = shape
    x = _dyadic_image(4, shape, 'tiled_x8.host')
    th, tw, ny, nx, _ = F.tiled_geometry(H, W, tile, pad)
    plain = _ramp_fn()
    assert not torch.equal(F.x8_reference(plain, x), plain(x))            # the transforms matter to this fn
    for P, slots in pairs:
        seen = []
        got = F.tiled_x8_reference(_ramp_fn(seen), x, tile, pad, P, slots)
        want = F.tiled_reference(lambda w: F.x8_reference(plain, w), x, tile, pad, P)
        assert got.dtype == torch.float32 and tuple(got.shape) == (B, C_, 4 * H, 4 * W)
        assert torch.equal(got, want), (P, slots)
        # the batches fn saw: slots x P x B windows, th x tw for k < 4 and tw x th for k >= 4, the tail pass included
        n = (8 if th == tw else 4) if slots is None else min(slots, 8 if th == tw else 4)
        p = min(max(1, 16 // (n * B)) if P is None else P, ny * nx)
        one_pass = [(n * p * B, C_, th, tw) if k0 < 4 else (n * p * B, C_, tw, th) for k0 in range(0, 8, n)]
        assert seen == one_pass * -(-ny * nx // p), (P, slots, seen)


def test_tiled_x8_reference_is_per_image_and_checks_its_arguments():
    shape, tile, pad, P = CASE_B
    x = _dyadic_image(5, shape, 'tiled_x8.host.b')
    fn = _ramp_fn()
    both = F.tiled_x8_reference(fn, x, tile, pad, P)
    for b in range(shape[0]):
        assert torch.equal(both[b:b + 1], F.tiled_x8_reference(fn, x[b:b + 1], tile, pad, P))
    for bad in (dict(tile=0), dict(pad=-1), dict(tiles_per_pass=0), dict(tile=2.5), dict(pad=None), dict(tile=True),
                dict(slots_per_pass=3), dict(slots_per_pass=0), dict(slots_per_pass=16)):
        kw = dict(tile=8, pad=2, tiles_per_pass=None, slots_per_pass=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            F.tiled_x8_reference(fn, x, **kw)


def test_tiled_x8_reference_is_the_whole_image_ensemble_with_enough_margin():
    from oracle import ref_torch as RT
    nb = 1
    sd = synth.rrdbnet_state_dict(nb=nb, seed=81)
    x = synth.image_batch(2, 1, 3, 45, 70, name='tiled')
    fn = lambda t: RT.rrdbnet_forward(t, sd, nb)
    with torch.no_grad():
        whole = F.x8_reference(fn, x)
        e_exact = (F.tiled_x8_reference(fn, x, 16, 15 * nb + 4) - whole).abs().max().item()
        e_none = (F.tiled_x8_reference(fn, x, 16, 0) - whole).abs().max().item()
        e_plain = (fn(x) - whole).abs().max().item()
    print('tiled_x8_reference vs x8_reference, 45 x 70, tile 16, nb 1: pad 19 %.3e, pad 0 %.3e; x8_reference vs the plain '
          'forward %.3e (output abs-max %.3f)' % (e_exact, e_none, e_plain, whole.abs().max().item()))
    assert e_exact <= 1e-6
    assert e_none > 1e-2
    assert e_plain > 1e-2         # the synthetic weights are not flip-equivariant: the ensemble is not the plain forward


def test_lib_mirrors_the_tile_x8_op():
    from esrganplus_amd import _lib as L
    assert L.OP_TILE_X8 == 17
    assert 'esr_tile_x8_op' in L.EXPORTS
    names = [f[0] for f in L.esr_tile_x8._fields_]
    assert names == [f[0] for f in L.esr_tile._fields_] + ['k_begin', 'k_count', 'accumulate', 'mean_scale']
    assert dict(L.esr_tile_x8._fields_)['mean_scale'] is C.c_float
    assert C.sizeof(L.esr_tile_x8) == C.sizeof(L.esr_tile) + 16
    assert 'tile_x8' in [f[0] for f in L._op_union._fields_]
    assert C.sizeof(L.esr_tile_x8) <= C.sizeof(L.esr_conv)    # the union, and with it sizeof(esr_op), did not grow
    lib = L.lib()                                             # loads the library: symbol present, sizeof(esr_op) agrees
    assert lib.esr_abi_version() == 6
    assert hasattr(lib, 'esr_tile_x8_op')
