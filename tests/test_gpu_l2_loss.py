"""The fused MSE criterion (csrc/loss_kernels.hip: esr_l2_loss_forward; losses.l2_raw / l2_loss — nn.MSELoss as
cri_pix / cri_fea 'l2', SR_model.py:28-34, SRRaGAN_model.py:31-53) against a plain fp64 restatement: values,
gradients, the scratch it shares with the l1 kernel, misaligned views, magnitude, argument checks."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.fp64_refs import U, f64

pytestmark = pytest.mark.gpu

W32 = float(np.float32(0.37))          # the weight as the kernel sees it
SENTINEL = -77.25
SCALINGS = [(1.0, None), (1024.0, None), (1.0, 0.125), (1024.0, 0.125)]      # (grad_scale, scale_dev): L1_SCALINGS
ESR_ERR_INVALID = -1


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def l2_ref(a, b, weight, scale=1.0):
    """(loss, grad_a) = (weight * mean (a - b)^2, scale * weight * 2 (a - b) / n) in fp64."""
    d = f64(a) - f64(b)
    return float(weight) * (d * d).mean(), float(scale) * float(weight) * 2.0 * d / d.size


def _scratch_is_clean(dev):
    from esrganplus_amd import losses as LS
    s = LS._scratch[dev].cpu()
    assert s[0].item() == 0.0 and s.view(torch.int64)[1].item() == 0, s


def _l2_check(name, loss, grad, a, b, scale):
    """Loss within 5 * 2^-24 and gradient within 6 * 2^-24 relative of l2_ref, the zeros of exact ties exact.  Returns
    the measured maxima in units of 2^-24."""
    l_ref, g_ref = l2_ref(a, b, W32, scale)
    el = abs(float(loss) - l_ref) / l_ref if l_ref else abs(float(loss))
    assert el <= 5 * U, (name, el / U)
    eg = 0.0
    if grad is not None:
        g = f64(grad)
        nz = g_ref != 0
        assert (g[~nz] == 0).all(), name
        if nz.any():
            eg = float((np.abs(g[nz] - g_ref[nz]) / np.abs(g_ref[nz])).max())
        assert eg <= 6 * U, (name, eg / U)
    return el / U, eg / U


def _pair(n, seed):
    g = torch.Generator().manual_seed(seed)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    if n > 1:
        b[::7] = a[::7]                                   # exact ties: gradient exactly 0
    return a, b


@pytest.mark.parametrize('n', [1, 3, 4, 5, 4095, 4096, 4097, 4 * 1024 * 1024 + 5])
def test_l2_raw_and_l2_loss_against_fp64(dev, n):
    """l2_raw (every grad_scale / scale_dev combination, and grad_out=None) and l2_loss on flat tensors of n elements;
    4 Mi + 5 is past the launcher's 1024 workgroups x 4096 elements, so the grid-stride loop runs a second pass that
    ends in the scalar tail.

    Tolerance, from the operation count.  Loss: the kernel rounds d = a - b once (relative 2^-24), which counts twice
    in d^2 (formed and summed in fp64: no further fp32 rounding), rounds the mean to fp32 and rounds its product with
    the weight: 4 roundings, held to 5 * 2^-24 relative of l2_ref given the fp32-rounded weight.  Gradient:
    fl(a - b), three roundings in ((2 weight / n) * grad_scale) * scale_dev (2 weight is exact, n < 2^24 converts
    exactly, fp32 division is correctly rounded) and one product: 5 roundings, held to 6 * 2^-24.  The zeros of exact
    ties are exact.  After every call the fp64 scratch reads back as [0.0, 0], also when l1 and l2 calls alternate."""
    from esrganplus_amd import losses as LS
    a, b = _pair(n, n)
    ties = slice(0, n if n > 1 else 0, 7)
    ad, bd = a.to(dev), b.to(dev)
    worst = [0.0, 0.0]
    l1_first = LS.l1_raw(ad, bd, 0.37).item()
    for gs, sd in SCALINGS:
        out = torch.full((n,), SENTINEL, device=dev)
        sdev = None if sd is None else torch.tensor([sd], device=dev)
        loss = LS.l2_raw(ad, bd, 0.37, grad_out=out, grad_scale=gs, scale_dev=sdev)
        _scratch_is_clean(dev)
        assert (out[ties] == 0).all()
        e = _l2_check('l2_raw gs=%g sd=%s' % (gs, sd), loss.item(), out, a, b, gs * (sd or 1.0))
        worst = [max(w, v) for w, v in zip(worst, e)]
        assert LS.l1_raw(ad, bd, 0.37).item() == l1_first          # the shared scratch, l1 behind l2
        _scratch_is_clean(dev)
    # grad_out=None: the loss alone; a buffer the caller might have passed is not touched
    cand = torch.full((n,), SENTINEL, device=dev)
    first = LS.l2_raw(ad, bd, 0.37, grad_out=None, grad_scale=1024.0).item()
    _scratch_is_clean(dev)
    assert (cand == SENTINEL).all()
    _l2_check('l2_raw grad_out=None', first, None, a, b, 1.0)
    for _ in range(2):                                    # the scratch is left clean: same answer again
        assert LS.l2_raw(ad, bd, 0.37).item() == first
    # the autograd face of the same kernel
    ag = ad.clone().requires_grad_(True)
    loss = LS.l2_loss(ag, bd, 0.37)
    _scratch_is_clean(dev)
    (loss * 1024.0).backward()
    e = _l2_check('l2_loss', loss.item(), ag.grad, a, b, 1024.0)       # the upstream factor is a power of two: exact
    assert loss.item() == first
    worst = [max(w, v) for w, v in zip(worst, e)]
    print('l2 n=%d: max relative error loss %.2f (bound 5), gradient %.2f (bound 6) x 2^-24' % (n, worst[0], worst[1]))


@pytest.mark.parametrize('which', ['a', 'b', 'grad_out', 'all'])
@pytest.mark.parametrize('k', [1, 2, 3])
def test_l2_raw_misaligned_views(dev, which, k):
    """Views base[k : k + n] whose data pointer is 4k bytes off a 16-byte boundary, for a, b, grad_out and all three:
    the kernel's scalar path gives the aligned call's bits and writes nothing outside the view (n = 4097: if the
    alignment test were wrong the vector body would run on 1024 of the quads)."""
    from esrganplus_amd import losses as LS
    n = 4097
    a, b = _pair(n, 100 + k)

    def place(t, off):
        base = torch.full((n + 8,), SENTINEL, device=dev)
        base[off:off + n] = t.to(dev)
        return base, base[off:off + n]

    ka, kb, kg = (k if which in ('a', 'all') else 0), (k if which in ('b', 'all') else 0), (k if which in ('grad_out', 'all') else 0)
    (_, av), (_, bv) = place(a, ka), place(b, kb)
    gbase, gv = place(torch.full((n,), SENTINEL), kg)
    for t, off in ((av, ka), (bv, kb), (gv, kg)):
        assert t.data_ptr() % 16 == 4 * off and t.is_contiguous()
    loss = LS.l2_raw(av, bv, 0.37, grad_out=gv, grad_scale=1024.0)
    _scratch_is_clean(dev)
    _l2_check('misaligned %s k=%d' % (which, k), loss.item(), gv, a, b, 1024.0)
    assert (gbase[:kg] == SENTINEL).all() and (gbase[kg + n:] == SENTINEL).all()      # nothing outside the view
    aligned = torch.empty(n, device=dev)
    loss_al = LS.l2_raw(a.to(dev), b.to(dev), 0.37, grad_out=aligned, grad_scale=1024.0)
    assert aligned.data_ptr() % 16 == 0
    assert loss.item() == loss_al.item() and torch.equal(gv, aligned)


def test_l2_large_difference_stays_finite(dev):
    """One pair with a - b = 3e20: its square, 9e40, is past fp32's range, but the kernel squares and sums in fp64 and
    the mean over 4096 elements (times the weight) is representable — finite, and within the loss bound."""
    from esrganplus_amd import losses as LS
    a, b = _pair(4096, 7)
    a[1], b[1] = 3e20, 0.0
    out = torch.empty(4096, device=dev)
    loss = LS.l2_raw(a.to(dev), b.to(dev), 0.37, grad_out=out)
    _scratch_is_clean(dev)
    assert np.isfinite(loss.item()) and torch.isfinite(out).all()
    _l2_check('3e20', loss.item(), out, a, b, 1.0)


def test_l2_refuses_what_l1_refuses(dev):
    """The operand checks of l1_raw / l1_loss, and the C entry's argument check."""
    from esrganplus_amd import losses as LS, _lib as L
    a, b = torch.randn(8, device=dev), torch.randn(8, device=dev)
    with pytest.raises(L.HipExtensionError):
        LS.l2_raw(a.cpu(), b.cpu(), 1.0)
    with pytest.raises(L.HipExtensionError):
        LS.l2_raw(a, b[:4], 1.0)
    with pytest.raises(L.HipExtensionError):
        LS.l2_raw(a.double(), b.double(), 1.0)
    with pytest.raises(L.HipExtensionError):
        LS.l2_loss(a, b.clone().requires_grad_(True))             # a target that requires a gradient
    h = LS.l2_loss(a.half().requires_grad_(True), b.half())          # fp16 operands are upcast
    assert h.dtype == torch.float32 and h.item() == LS.l2_raw(a.half().float(), b.half().float(), 1.0).item()
    assert L.lib().esr_l2_loss_forward(None, None) == ESR_ERR_INVALID
    assert b'esr_l2_loss_forward' in L.lib().esr_last_error()
    p = L.esr_l1_loss()
    p.a, p.b, p.n = a.data_ptr(), b.data_ptr(), 8                   # no loss / scratch pointers
    assert L.lib().esr_l2_loss_forward(C.byref(p), None) == ESR_ERR_INVALID
    assert L.lib().esr_abi_version() == 6
