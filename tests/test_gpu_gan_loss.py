"""The fused GANLoss kernel (csrc/loss_kernels.hip: esr_gan_loss_forward; losses.gan_raw / gan_loss / gan_pair_loss /
GANLoss — loss.py:6-38 as the standard-GAN step calls it, SRGAN_model.py:129-146) against the fp64 restatement of
tests/gan_refs.py with bounds from the operation count, and against torch's own criteria on the GPU."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import gan_refs as G
from tests.fp64_refs import U, f64

pytestmark = pytest.mark.gpu

WEIGHT = 5e-3
W32 = float(np.float32(WEIGHT))        # the weight as the kernel sees it
SENTINEL = -77.25
ESR_ERR_INVALID = -1
SIZES = [1, 4, 16, 255, 257, 1000]     # either side of the workgroup's 256 threads, several trips of its loop
LABELS = [(1.0, 0.0), (0.9, 0.1)]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _ratio(err, bound):
    """err / bound; an exact result passes under any bound, an inexact one under a zero bound does not."""
    if err == 0.0:
        return 0.0
    return err / bound if bound > 0.0 else float('inf')


def _check(name, kind, loss, aux, ops, weight, scale):
    """ops: [(x cpu, label, grad or None)] for one or two operands.  Every figure divided by its bound; returns the
    worst ratio (asserted <= 1 by the caller after printing)."""
    worst = 0.0
    terms, tb = [], []
    for i, (x, t, grad) in enumerate(ops):
        term, mean, g_ref = G.gan_ref(x, t, kind, weight, scale)
        b = G.term_bound(x, t, kind)
        terms.append(term), tb.append(b)
        # the term: the unrounded mean within b, then one rounding to fp32
        worst = max(worst, _ratio(abs(float(aux[i]) - term), b + U * abs(term)))
        # the mean of the logits: an fp64 sum of fp32 values, rounded once
        worst = max(worst, _ratio(abs(float(aux[2 + i]) - mean), U * abs(mean) + 1e-12 * np.abs(f64(x)).mean() + G.TINY))
        if grad is not None:
            err, gb = np.abs(f64(grad).reshape(-1) - g_ref), G.grad_bound(x, t, kind, weight, scale)
            worst = max(worst, max(_ratio(float(e), float(b_)) for e, b_ in zip(err, gb)))
    if len(ops) == 1:
        assert float(aux[1]) == 0.0 and float(aux[3]) == 0.0, name
    # the loss: the fp64 sum of the terms rounded to fp32, times the weight: 2 roundings
    ref = weight * sum(terms)
    worst = max(worst, _ratio(abs(float(loss) - ref), abs(weight) * sum(tb) + 2 * U * abs(ref)))
    return worst


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('kind', ['vanilla', 'lsgan'])
def test_gan_raw_and_gan_loss_against_fp64(dev, kind, n):
    """gan_raw with one and two operands, labels (1, 0) and (0.9, 0.1), weight 5e-3, grad_scale 1024 with and without
    scale_dev, and without gradient buffers; gan_loss / gan_pair_loss (autograd) on the same logits: N(0, 3) with 0,
    +-90 and +-1e-7 planted (exp(90) overflows fp32: the stable form must not).  Bounds: tests/gan_refs.py."""
    from esrganplus_amd import losses as LS
    x, y = G.planted_logits(n, n), G.planted_logits(n, 1000 + n).flip(0)
    xd, yd = x.to(dev).view(n, 1), y.to(dev).view(n, 1)
    worst = 0.0
    for real, fake in LABELS:
        tr, tf = G.label32(real), G.label32(fake)
        for sd in (None, 0.125):
            sdev = None if sd is None else torch.tensor([sd], device=dev)
            scale = 1024.0 * (sd or 1.0)
            kw = dict(grad_scale=1024.0, scale_dev=sdev, real_label_val=real, fake_label_val=fake)
            gx, gy = torch.full((n,), SENTINEL, device=dev), torch.full((n,), SENTINEL, device=dev)
            loss, aux = LS.gan_raw(xd, True, kind, WEIGHT, grad_x=gx, **kw)
            worst = max(worst, _check('one', kind, loss.item(), aux.cpu(), [(x, tr, gx)], W32, scale))
            assert (gy == SENTINEL).all()
            loss2, aux2 = LS.gan_raw(xd, True, kind, WEIGHT, grad_x=gx, y=yd, y_is_real=False, grad_y=gy, **kw)
            worst = max(worst, _check('two', kind, loss2.item(), aux2.cpu(), [(x, tr, gx), (y, tf, gy)], W32, scale))
            assert aux2[0].item() == aux[0].item() and aux2[2].item() == aux[2].item()
        # no gradient buffers: the loss alone, the same bits
        cand = torch.full((n,), SENTINEL, device=dev)
        loss3, aux3 = LS.gan_raw(xd, True, kind, WEIGHT, y=yd, y_is_real=False, grad_scale=1024.0,
                                 real_label_val=real, fake_label_val=fake)
        assert loss3.item() == loss2.item() and torch.equal(aux3, aux2) and (cand == SENTINEL).all()
        # the autograd faces
        xa, ya = xd.clone().requires_grad_(True), yd.clone().requires_grad_(True)
        la = LS.gan_loss(xa, True, kind, WEIGHT, real, fake)
        (la * 1024.0).backward()              # a power of two: exact
        worst = max(worst, _check('gan_loss', kind, la.item(), [aux[0].item(), 0.0, aux[2].item(), 0.0],
                                  [(x, tr, xa.grad)], W32, 1024.0))
        assert xa.grad.shape == xa.shape
        xa.grad = None
        lp, auxp = LS.gan_pair_loss(xa, True, ya, False, kind, WEIGHT, real, fake)
        assert not auxp.requires_grad
        (lp * 1024.0).backward()
        worst = max(worst, _check('gan_pair_loss', kind, lp.item(), auxp.cpu(), [(x, tr, xa.grad), (y, tf, ya.grad)],
                                  W32, 1024.0))
        assert lp.item() == loss2.item()
    print('gan %s n=%d: worst error / bound = %.3f' % (kind, n, worst))
    assert worst <= 1.0


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('kind', ['vanilla', 'lsgan'])
def test_gan_loss_equals_torch(dev, kind, n):
    """``GANLoss`` (the module, reference constructor) against F.binary_cross_entropy_with_logits / F.mse_loss on the
    GPU, at test_l1_loss_and_gradient's tolerances: loss 1e-6 * max(1, |loss|), gradient rtol 1e-6.  vanilla: both
    sides form sigmoid(x) - t from a sigmoid that is within 6 U of the exact one, so where the difference cancels the
    gradients may differ by 12 U times the factor 1024 / n: that, and nothing else, is the absolute allowance."""
    from esrganplus_amd import losses as LS
    x0 = G.planted_logits(n, 2000 + n).to(dev).view(n, 1)
    for real, fake in LABELS:
        cri = LS.GANLoss(kind.upper(), real, fake)
        for is_real in (True, False):
            t = real if is_real else fake
            res = []
            for fn in ((lambda v: F.binary_cross_entropy_with_logits(v, torch.full_like(v, t))) if kind == 'vanilla'
                       else (lambda v: F.mse_loss(v, torch.full_like(v, t))), lambda v: cri(v, is_real)):
                v = x0.clone().requires_grad_(True)
                loss = fn(v)
                (loss * 1024.0).backward()
                res.append((loss.detach(), v.grad))
            (l0, g0), (l1, g1) = res
            assert abs(l0.item() - l1.item()) <= 1e-6 * max(1.0, abs(l0.item())), (real, fake, is_real)
            atol = 12 * U * 1024.0 / n if kind == 'vanilla' else 0.0
            assert torch.allclose(g0, g1, rtol=1e-6, atol=atol), (real, fake, is_real, (g0 - g1).abs().max().item())


@pytest.mark.parametrize('kind', ['vanilla', 'lsgan'])
def test_gan_raw_views_offset_by_one_float(dev, kind):
    """Operands and gradient buffers that are views base[1 : 1 + n] (4 bytes off a 16-byte boundary), n_x != n_y: the
    aligned call's bits, and nothing written outside the views."""
    from esrganplus_amd import losses as LS
    nx, ny = 257, 16
    x, y = G.planted_logits(nx, 5), G.planted_logits(ny, 6)

    def place(t):
        base = torch.full((t.numel() + 8,), SENTINEL, device=dev)
        base[1:1 + t.numel()] = t.to(dev)
        return base, base[1:1 + t.numel()]

    (_, xv), (_, yv) = place(x), place(y)
    gxb, gxv = place(torch.full((nx,), SENTINEL))
    gyb, gyv = place(torch.full((ny,), SENTINEL))
    for t in (xv, yv, gxv, gyv):
        assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    loss, aux = LS.gan_raw(xv, True, kind, WEIGHT, grad_x=gxv, y=yv, y_is_real=False, grad_y=gyv, grad_scale=1024.0)
    assert (gxb[:1] == SENTINEL).all() and (gxb[1 + nx:] == SENTINEL).all()
    assert (gyb[:1] == SENTINEL).all() and (gyb[1 + ny:] == SENTINEL).all()
    gx, gy = torch.empty(nx, device=dev), torch.empty(ny, device=dev)
    loss_al, aux_al = LS.gan_raw(x.to(dev), True, kind, WEIGHT, grad_x=gx, y=y.to(dev), y_is_real=False, grad_y=gy,
                                 grad_scale=1024.0)
    assert loss.item() == loss_al.item() and torch.equal(aux, aux_al) and torch.equal(gx, gxv) and torch.equal(gy, gyv)
    worst = _check('views', kind, loss.item(), aux.cpu(), [(x, 1.0, gxv), (y, 0.0, gyv)], W32, 1024.0)
    print('gan %s views, n_x %d n_y %d: worst error / bound = %.3f' % (kind, nx, ny, worst))
    assert worst <= 1.0


@pytest.mark.parametrize('kind', ['vanilla', 'lsgan'])
def test_gan_raw_repeats_bit_for_bit(dev, kind):
    """Ten successive calls give the same bits (the kernel keeps no scratch between calls), also with an l1 / l2 call
    in between."""
    from esrganplus_amd import losses as LS
    x, y = G.planted_logits(300, 7).to(dev), G.planted_logits(16, 8).to(dev)
    first = None
    for i in range(10):
        gx, gy = torch.empty(300, device=dev), torch.empty(16, device=dev)
        loss, aux = LS.gan_raw(x, True, kind, WEIGHT, grad_x=gx, y=y, y_is_real=False, grad_y=gy, grad_scale=1024.0)
        cur = (loss.item(), aux.cpu(), gx.cpu(), gy.cpu())
        if first is None:
            first = cur
        assert cur[0] == first[0] and all(torch.equal(a, b) for a, b in zip(cur[1:], first[1:])), i
        (LS.l1_raw if i % 2 else LS.l2_raw)(x, x.flip(0), 0.37)


def test_gan_entry_refusals_leave_outputs_untouched(dev):
    """The C entry's refusals (null struct, null x, n_x < 1, y with n_y < 1, unknown kind, null loss): ESR_ERR_INVALID
    with the entry's name, before any launch — the sentinel-filled outputs stay as they were.  And the Python face's."""
    from esrganplus_amd import losses as LS, _lib as L
    lib = L.lib()
    x, y = torch.randn(8, device=dev), torch.randn(8, device=dev)
    out = torch.full((5 + 8 + 8,), SENTINEL, device=dev)

    def args(**kw):
        p = L.esr_gan_loss()
        p.x, p.y, p.n_x, p.n_y, p.kind, p.weight = x.data_ptr(), y.data_ptr(), 8, 8, 0, 1.0
        base = out.data_ptr()
        p.loss, p.term_x, p.term_y, p.mean_x, p.mean_y = (base + 4 * i for i in range(5))
        p.grad_x, p.grad_y = base + 20, base + 52
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    assert lib.esr_gan_loss_forward(None, None) == ESR_ERR_INVALID
    assert b'esr_gan_loss_forward' in lib.esr_last_error()
    for bad in (dict(x=None), dict(n_x=0), dict(n_x=-3), dict(n_y=0), dict(kind=2), dict(kind=-1), dict(loss=None)):
        lib.esr_l2_loss_forward(None, None)                  # (another entry's message in between)
        assert lib.esr_gan_loss_forward(C.byref(args(**bad)), C.c_void_p(torch.cuda.current_stream().cuda_stream)) \
            == ESR_ERR_INVALID, bad
        assert b'esr_gan_loss_forward' in lib.esr_last_error(), bad
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    # y absent: n_y is not looked at
    assert lib.esr_gan_loss_forward(C.byref(args(y=None, n_y=0, grad_y=None)),
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    assert (out[13:] == SENTINEL).all() and (out[:13] != SENTINEL).all()
    assert lib.esr_abi_version() == 6
    # the Python face: no fallback
    with pytest.raises(L.HipExtensionError):
        LS.gan_raw(x.cpu(), True, 'vanilla', 1.0)
    with pytest.raises(L.HipExtensionError):
        LS.gan_raw(x.double(), True, 'vanilla', 1.0)
    with pytest.raises(L.HipExtensionError):
        LS.gan_raw(x, True, 'vanilla', 1.0, grad_x=torch.empty(4, device=dev))
    with pytest.raises(L.HipExtensionError):
        LS.gan_loss(x.cpu().requires_grad_(True), True)
    with pytest.raises(NotImplementedError):
        LS.gan_raw(x, True, 'wgan-gp', 1.0)
    h = LS.gan_loss(x.half().requires_grad_(True), True, 'lsgan')           # fp16 logits are upcast
    assert h.dtype == torch.float32 and h.item() == LS.gan_raw(x.half().float(), True, 'lsgan', 1.0)[0].item()
