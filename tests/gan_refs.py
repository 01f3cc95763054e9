"""Plain fp64 restatement of ``GANLoss`` (codes/models/modules/loss.py:6-38: 'vanilla' = BCE with logits against a
constant label, 'lsgan' = MSE against it) with its gradient, and the error bounds the fused kernel
(csrc/loss_kernels.hip: gan_loss_kernel) is held to, derived from its operation count in units of U = 2^-24.  Pure
functions on CPU tensors / numpy arrays."""
import numpy as np

from tests.fp64_refs import U, f64, sigmoid, softplus

LIBM = 4                   # expf / log1pf taken as accurate to 2 ulp = 4 U relative (tests/test_gpu_losses.py)
TINY = 2.0 ** -126         # results below fp32's normal range (exp(-90)) may be flushed: absolute error up to this
PLANTED = (0.0, 90.0, -90.0, 1e-7, -1e-7)


def label32(v):
    """The label value as the kernel sees it (a float argument)."""
    return float(np.float32(v))


def gan_ref(x, t, kind, weight=1.0, scale=1.0):
    """(term, mean, grad) of one operand: term = l(x, t) unweighted, grad = scale * weight * d term / d x."""
    x = f64(x).reshape(-1)
    n = x.size
    if kind == 'vanilla':
        return (softplus(x) - x * t).mean(), x.mean(), scale * weight * (sigmoid(x) - t) / n
    d = x - t
    return (d * d).mean(), x.mean(), scale * weight * 2.0 * d / n


def term_bound(x, t, kind):
    """Absolute bound on the kernel's UNROUNDED mean of the elements (the fp64 sum adds nothing visible).
    vanilla, per element: e = expf(-|x|) (LIBM U relative); lp = log1pf(e): LIBM U of its own plus e's error through
    d log1p / de = 1 / (1 + e), e / (1 + e) <= log1p(e): 2 LIBM U lp (+ TINY where e is subnormal); x t, max(x, 0) - x t
    and the sum with lp round once each, every one on a magnitude <= |x| (1 + |t|) + lp: 3 U of that.
    lsgan: d = fl(x - t), U relative, counts twice in d^2 (formed in fp64): 2 U d^2."""
    x = f64(x).reshape(-1)
    if kind == 'vanilla':
        lp = np.log1p(np.exp(-np.abs(x)))
        return (U * (3.0 * (np.abs(x) * (1.0 + abs(t)) + lp) + 2 * LIBM * lp) + TINY).mean()
    d = x - t
    return (2.0 * U * d * d).mean()


def grad_bound(x, t, kind, weight, scale):
    """Per-element absolute bound on the gradient.  The factor gw = ((k weight / n) grad_scale) scale_dev rounds three
    times (k = 1 or 2: exact; n converts exactly; fp32 division is correctly rounded) and its product with the
    element's d once: 4 U |g|.  vanilla: d = sigmoid(x) - t with sigmoid = (1 or e) / (1 + e): e LIBM U relative, the
    sum and the quotient round once each: 6 U sigmoid (+ TINY: a subnormal e), and the subtraction rounds once: U |d|.
    lsgan: d = fl(x - t): U |d|."""
    x = f64(x).reshape(-1)
    gw = abs(scale * weight) / x.size
    if kind == 'vanilla':
        s = sigmoid(x)
        return gw * ((LIBM + 2) * U * s + TINY + 5.0 * U * np.abs(s - t))
    return 2.0 * gw * 5.0 * U * np.abs(x - t)


def planted_logits(n, seed):
    """n float32 logits from N(0, 3) with the PLANTED values spread over them (as many as fit)."""
    import torch
    g = torch.Generator().manual_seed(seed)
    x = 3 * torch.randn(n, generator=g)
    for k, v in enumerate(PLANTED[:n]):
        x[(k * n) // min(n, len(PLANTED))] = v
    return x
