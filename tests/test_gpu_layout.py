"""to_g32_kernel / from_g32_kernel (csrc/aux_kernels.hip) on their own: esr_convert_layout called directly on
engine.G32 buffers, against tests/fp64_refs.to_g32_ref / from_g32_ref.  Every other GPU test uploads and downloads
through these two kernels, which covers the plain copy inside whole-network tolerances; here the copy is bit-exact, what
lies outside the converted region must keep a sentinel, and the folded input normalisation (``use_affine``, channels
< 4) and the adding download (``accumulate``) are held to their rounding counts (U = 2^-24)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import fp64_refs as R

pytestmark = pytest.mark.gpu

U = R.U
SENTINEL = -77.25               # exact in fp16 and fp32
# C = 1 (one lane of a group), 9 and 17 (a second group of ONE channel in fp32 / fp16) next to the recipe's 3
SHAPES = [(2, 3, 5, 63), (1, 4, 3, 64), (2, 5, 2, 65), (1, 40, 4, 130), (2, 1, 3, 33), (1, 9, 2, 66), (2, 17, 3, 34)]
MEAN = [float(np.float32(v)) for v in (0.485, 0.456, 0.406, 0.25)]
INV_STD = [float(np.float32(v)) for v in (1 / 0.229, 1 / 0.224, 1 / 0.225, 3.0)]
GUARD = 96


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _buffer(dev, shape, prec, fill=None, seed=0):
    """A G32 buffer with two groups more than C needs (they lie beyond the view's ngroups), filled with the sentinel
    or — fill='random' — with random values everywhere, halo included."""
    from esrganplus_amd import engine as E
    B, C_, H, W = shape
    cpg = 16 if prec == 'fp16' else 8
    g = E.G32(B, C_ + 2 * cpg, H, W, prec, dev)
    assert (g.Hp, g.Wp, g.cpg) == R.g32_geometry(H, W, 2 if prec == 'fp16' else 4)
    if fill == 'random':
        gen = torch.Generator().manual_seed(seed)
        g.t.copy_(torch.randn(g.t.shape, generator=gen).to(g.t.dtype))
    else:
        g.t.fill_(SENTINEL)
    return g


def _convert(g, shape, nchw, to_g32, affine=False, accumulate=0):
    from esrganplus_amd import _lib as L, engine as E
    B, C_, H, W = shape
    lo = L.esr_layout()
    lo.dtype, lo.to_g32, lo.B, lo.C, lo.H, lo.W = g.esr_dtype, to_g32, B, C_, H, W
    lo.nchw, lo.g32, lo.accumulate = nchw.data_ptr(), g.view(0, C_), accumulate
    assert lo.g32.ngroups == (C_ + g.cpg - 1) // g.cpg
    if affine:
        lo.use_affine = 1
        for i in range(4):
            lo.mean_c[i], lo.inv_std_c[i] = MEAN[i], INV_STD[i]
    L.check(L.lib().esr_convert_layout(C.byref(lo), C.c_void_p(E.current_stream())), 'esr_convert_layout')
    torch.cuda.synchronize()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


def _interior(g, shape):
    """(the whole buffer as numpy, its written region [B][ngroups][H][W][cpg], a mask of everything else)."""
    B, C_, H, W = shape
    ng = (C_ + g.cpg - 1) // g.cpg
    t = g.t.cpu().numpy()
    mask = np.ones(t.shape, dtype=bool)
    mask[:, :ng, 1:H + 1, 1:W + 1, :] = False
    return t, t[:, :ng, 1:H + 1, 1:W + 1, :], mask


def _half_ulp16(r):
    """Half an fp16 ulp at magnitude r (fp16 subnormals below 2^-14: half of 2^-24)."""
    e = np.floor(np.log2(np.maximum(np.abs(r), 2.0 ** -14)))
    return 2.0 ** (e - 11)


def _x(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize('affine', [False, True])
@pytest.mark.parametrize('prec', ['fp32', 'fp16'])
@pytest.mark.parametrize('shape', SHAPES)
def test_to_g32_values_padding_and_untouched_surroundings(dev, shape, prec, affine):
    """NCHW -> G32.  Plain: fp32 bit-exact, fp16 bit-exact against x.half(); the channels past C of the last group are
    +0; every byte outside the H x W interior of the C-channel groups — the one-pixel ring and the rows / columns
    beyond it, the other groups — still holds the sentinel.  With use_affine channels < 4 are (x - mean) * inv_std:
    two fp32 roundings, (2 U + U^2) |r|, and for fp16 half an fp16 ulp of the result on top; channels >= 4 pass
    through unchanged."""
    B, C_, H, W = shape
    x = _x(shape, sum(shape))
    xd = x.to(dev)
    g = _buffer(dev, shape, prec)
    _convert(g, shape, xd, 1, affine=affine)
    t, inner, mask = _interior(g, shape)
    sent = np.array(SENTINEL, dtype=t.dtype)
    assert (_bits(t[mask]) == _bits(sent)).all()
    xs = x.half() if prec == 'fp16' else x
    want = R.to_g32_ref(xs, g.cpg).astype(t.dtype)                      # exact: the values are of that type already
    if not affine:
        assert (_bits(inner) == _bits(want)).all()
        return
    # channel c of group 0 is element c
    same = np.ones(inner.shape, dtype=bool)
    same[:, 0, :, :, :min(4, C_)] = False
    assert (_bits(inner[same]) == _bits(want[same])).all()
    ref = R.to_g32_ref(x, g.cpg, MEAN, INV_STD)
    r, got = ref[~same], inner[~same].astype(np.float64)
    tol = (2 * U + U * U) * np.abs(r) + 2.0 ** -149
    if prec == 'fp16':
        tol = tol + _half_ulp16(np.abs(r) + tol)
    ratio = float((np.abs(got - r) / tol).max())
    print('to_g32 affine %s %s: measured / bound %.3f' % (shape, prec, ratio))
    assert ratio <= 1.0


@pytest.mark.parametrize('affine', [False, True])
@pytest.mark.parametrize('prec', ['fp32', 'fp16'])
@pytest.mark.parametrize('shape', SHAPES)
def test_from_g32_values_adjoint_affine_and_accumulate(dev, shape, prec, affine):
    """G32 -> NCHW from a buffer that is random everywhere (halo and spare groups included).  accumulate = 0 over a
    sentinel-filled output overwrites all of [0, C) x H x W and nothing around it: the exact widening of the stored
    values, with use_affine times inv_std for channels < 4 only (the adjoint of the normalisation: one rounding,
    U |r|).  accumulate = 1, run twice: each run leaves previous + value, to one fp32 rounding of the sum (plus the
    product's with use_affine)."""
    B, C_, H, W = shape
    n = B * C_ * H * W
    g = _buffer(dev, shape, prec, fill='random', seed=sum(shape) + 1)
    stored = g.t.cpu().numpy()[:, :(C_ + g.cpg - 1) // g.cpg, 1:H + 1, 1:W + 1, :]
    val = R.from_g32_ref(stored, C_, INV_STD if affine else None)
    exact = np.ones(shape, dtype=bool)
    if affine:
        exact[:, :4] = False
    flat = torch.full((n + 2 * GUARD,), SENTINEL, device=dev)
    out = flat[GUARD:GUARD + n].view(shape)
    _convert(g, shape, out, 0, affine=affine)
    assert (flat[:GUARD] == SENTINEL).all() and (flat[GUARD + n:] == SENTINEL).all()
    got = out.cpu().numpy()
    assert (_bits(got[exact]) == _bits(val[exact].astype(np.float32))).all()
    worst = 0.0
    if affine:
        worst = float((np.abs(got[~exact] - val[~exact]) / (U * np.abs(val[~exact]) + 2.0 ** -149)).max())
        assert worst <= 1.0
    # accumulate
    prev = _x(shape, 5).to(dev)
    flat[GUARD:GUARD + n] = prev.view(-1)
    wa = 0.0
    for _ in range(2):
        before = R.f64(out)
        _convert(g, shape, out, 0, affine=affine, accumulate=1)
        s = before + val
        tol = U * np.abs(s) + (U * np.abs(val) * ~exact) + 2.0 ** -149
        wa = max(wa, float((np.abs(R.f64(out) - s) / tol).max()))
        assert (R.f64(out) != before).mean() > 0.9                      # it really adds
    assert (flat[:GUARD] == SENTINEL).all() and (flat[GUARD + n:] == SENTINEL).all()
    print('from_g32 %s %s affine=%d: measured / bound  affine %.3f  accumulate %.3f' % (shape, prec, affine, worst, wa))
    assert wa <= 1.0


@pytest.mark.parametrize('shape', SHAPES)
def test_layout_affine_kernels_are_adjoint(dev, shape):
    """<to_g32_affine(u) - to_g32_affine(0), v> == <u, from_g32_affine(v)> for random u (NCHW) and v (G32, fp32), the
    inner products taken in fp64: ties the two kernels' handling of the normalisation together without either
    restatement.  Each to_g32 value carries two roundings and each from_g32 value one, so the two sides may differ by
    sum |v| 2 U (|T(u)| + |T(0)|) + sum |u| U |F(v)|."""
    B, C_, H, W = shape
    u = _x(shape, 77)
    gu, g0 = _buffer(dev, shape, 'fp32'), _buffer(dev, shape, 'fp32')
    _convert(gu, shape, u.to(dev), 1, affine=True)
    _convert(g0, shape, torch.zeros(shape, device=dev), 1, affine=True)
    Tu, T0 = R.f64(_interior(gu, shape)[1]), R.f64(_interior(g0, shape)[1])
    gv = _buffer(dev, shape, 'fp32', fill='random', seed=78)
    v = R.f64(_interior(gv, shape)[1])
    Fv = torch.full(shape, SENTINEL, device=dev)
    _convert(gv, shape, Fv, 0, affine=True)
    Fv, u = R.f64(Fv), R.f64(u)
    lhs, rhs = ((Tu - T0) * v).sum(), (u * Fv).sum()
    tol = (np.abs(v) * 2 * U * (np.abs(Tu) + np.abs(T0))).sum() + (np.abs(u) * U * np.abs(Fv)).sum()
    print('layout adjoint %s: |lhs - rhs| / bound %.3f (lhs %.6f)' % (shape, abs(lhs - rhs) / tol, lhs))
    assert abs(lhs - rhs) <= tol
