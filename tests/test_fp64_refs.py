"""The fp64 restatements of tests/fp64_refs.py against torch's own float64 implementations on the CPU, to 1e-12
relative: what makes them trustworthy as references for the GPU tests (test_gpu_losses / test_gpu_optim /
test_gpu_layout).  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import fp64_refs as R

RTOL = 1e-12


def _close(got, want, cancelling=False):
    """|got - want| <= 1e-12 |want| element by element; ``cancelling``: the value is a sum of terms of either sign
    (a gradient minus its mean share, a first moment), where 1e-12 is taken of the array's largest magnitude."""
    got, want = np.asarray(got, dtype=np.float64), R.f64(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all() and np.isfinite(want).all()
    tol = RTOL * (np.abs(want).max() if cancelling else np.abs(want))
    assert (np.abs(got - want) <= tol).all(), float(np.abs(got - want).max())


@pytest.mark.parametrize('n', [1, 5, 4097])
def test_l1_ref_is_torch_l1_loss_in_float64(n):
    g = torch.Generator().manual_seed(n)
    a = torch.randn(n, generator=g)
    b = torch.randn(n, generator=g)
    b[::7] = a[::7]
    a64 = a.double().requires_grad_(True)
    loss = 0.37 * F.l1_loss(a64, b.double())
    (loss * 1024.0).backward()
    l, gr = R.l1_ref(a, b, 0.37, 1024.0)
    _close(l, loss)
    _close(gr, a64.grad)
    assert (gr[::7] == 0.0).all()


def _torch_ragan(x, y, tx, ty, w):
    x64, y64 = x.double().requires_grad_(True), y.double().requires_grad_(True)
    lx = F.binary_cross_entropy_with_logits(x64 - y64.mean(), torch.full_like(x64, tx))
    ly = F.binary_cross_entropy_with_logits(y64 - x64.mean(), torch.full_like(y64, ty))
    loss = w * (lx + ly) / 2
    loss.backward()
    return loss, torch.stack([x64.mean(), y64.mean(), lx, ly]), x64.grad, y64.grad


@pytest.mark.parametrize('tx,ty', [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize('n', [1, 16, 37, 257])
def test_ragan_ref_is_autograd_through_bce_with_logits_in_float64(n, tx, ty):
    if n >= 16:
        x, y = R.saturated_logits(n, n)
        assert set(R.SATURATED) <= set(x.tolist()) and set(R.SATURATED) <= set(y.tolist())
    else:
        g = torch.Generator().manual_seed(n)
        x, y = 3 * torch.randn(n, generator=g), 3 * torch.randn(n, generator=g)
    for w in (1.0, 5e-3):
        want = _torch_ragan(x, y, float(tx), float(ty), w)
        assert all(torch.isfinite(t).all() for t in want)          # torch's fp64 BCE stays finite on +-1e4 logits
        loss, aux, gx, gy = R.ragan_ref(x, y, tx, ty, w)
        _close(loss, want[0])
        _close(aux, want[1])
        _close(gx, want[2], cancelling=True)
        _close(gy, want[3], cancelling=True)


@pytest.mark.parametrize('wd', [0.0, 1e-2])
@pytest.mark.parametrize('eps', [1e-8, 1e-3])
@pytest.mark.parametrize('betas', [(0.9, 0.999), (0.8, 0.99)])
def test_adam_ref_is_torch_adam_in_float64(betas, eps, wd):
    g = torch.Generator().manual_seed(3)
    shapes = [(1,), (257,), (8, 3, 3, 3)]
    init = [torch.randn(s, generator=g) for s in shapes]
    ps = [torch.nn.Parameter(t.double()) for t in init]
    opt = torch.optim.Adam(ps, lr=1e-3, betas=betas, eps=eps, weight_decay=wd)
    ref = R.adam_ref(init, lr=1e-3, betas=betas, eps=eps, weight_decay=wd)
    for it in range(12):
        grads = [torch.randn(s, generator=g) * (0.1 + it) for s in shapes]
        grads[1][:40] = 0.0
        grads[1][40:80] *= 1e-20
        for p, gr in zip(ps, grads):
            p.grad = gr.double()
        opt.step()
        ref.step([gr * 1024.0 for gr in grads], grad_scale=1.0 / 1024.0)
        if it == 5:
            opt.param_groups[0]['lr'] = ref.lr = 5e-4
        for k, p in enumerate(ps):
            _close(ref.p[k], p)
            _close(ref.m[k], opt.state[p]['exp_avg'], cancelling=True)
            _close(ref.v[k], opt.state[p]['exp_avg_sq'])
            assert (ref.mag[k] >= np.abs(ref.m[k])).all()
    assert ref.t == 12 and float(opt.state[ps[0]]['step']) == 12.0


def test_layout_refs_are_inverse_permutations_and_adjoint():
    """to_g32_ref puts channel c at [c // cpg][..][c % cpg] and pads with zeros; from_g32_ref reads it back; with
    the affine the two are adjoint up to the constant to_g32_ref(0)."""
    rng = np.random.default_rng(0)
    mean, inv = [0.485, 0.456, 0.406, 0.1], [1 / 0.229, 1 / 0.224, 1 / 0.225, 3.0]
    for cpg in (8, 16):
        x = rng.standard_normal((2, 21, 3, 5))
        g = R.to_g32_ref(x, cpg)
        assert g.shape == (2, (21 + cpg - 1) // cpg, 3, 5, cpg)
        assert g[1, 20 // cpg, 2, 4, 20 % cpg] == x[1, 20, 2, 4] and (g[:, -1, :, :, 21 % cpg:] == 0).all()
        assert (R.from_g32_ref(g, 21) == x).all()
        ga = R.to_g32_ref(x, cpg, mean, inv)
        _close(ga[0, 0, 1, 2, 3], (x[0, 3, 1, 2] - mean[3]) * inv[3])
        assert ga[0, 0, 1, 2, 4] == x[0, 4, 1, 2]
        v = rng.standard_normal(g.shape)
        lhs = ((ga - R.to_g32_ref(np.zeros_like(x), cpg, mean, inv)) * v).sum()
        rhs = (x * R.from_g32_ref(v, 21, inv)).sum()
        assert abs(lhs - rhs) <= 1e-12 * np.abs(x * R.from_g32_ref(v, 21, inv)).sum()
