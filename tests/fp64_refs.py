"""Plain fp64 restatements of the train step's scalar tail, for the GPU tests to compare the HIP kernels with:
the two losses (csrc/loss_kernels.hip), fused Adam (csrc/nn_kernels.hip) and the NCHW <-> G32 layout conversion
(csrc/aux_kernels.hip).  Pure functions on CPU tensors / numpy arrays, no GPU; tests/test_fp64_refs.py pins them to
torch's own float64 implementations."""
import numpy as np

U = 2.0 ** -24            # unit roundoff of fp32: one correctly rounded operation errs by at most U relative


def f64(t):
    """A torch tensor / array / scalar as a float64 numpy array (exact for fp16 and fp32 inputs)."""
    if hasattr(t, 'detach'):
        t = t.detach().cpu().numpy()
    return np.asarray(t).astype(np.float64)


def sigmoid(z):
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def softplus(z):
    return np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))


def l1_ref(a, b, weight, scale=1.0):
    """(loss, grad_a) = (weight * mean|a - b|, scale * weight * sign(a - b) / n), sign(0) = 0."""
    d = f64(a) - f64(b)
    return float(weight) * np.abs(d).mean(), float(scale) * float(weight) * np.sign(d) / d.size


def ragan_ref(x, y, tx, ty, weight):
    """weight * (BCE(x - mean(y), tx) + BCE(y - mean(x), ty)) / 2 with logits x, y and targets tx, ty in {0, 1}.
    Returns (loss, aux = [mean_x, mean_y, BCE_x, BCE_y], grad_x, grad_y)."""
    x, y = f64(x).reshape(-1), f64(y).reshape(-1)
    n = x.size
    mx, my = x.mean(), y.mean()
    z1, z2 = x - my, y - mx
    lx, ly = (softplus(z1) - tx * z1).mean(), (softplus(z2) - ty * z2).mean()
    d1, d2 = sigmoid(z1) - tx, sigmoid(z2) - ty
    hw = 0.5 * float(weight)
    # x_i enters z1_i directly and every z2_j through mean(x)
    return hw * (lx + ly), np.array([mx, my, lx, ly]), hw / n * (d1 - d2.mean()), hw / n * (d2 - d1.mean())


SATURATED = (30.0, -30.0, 88.0, -88.0, 100.0, -100.0, 1e4, -1e4)     # expf(|z|) overflows fp32 from |z| ~ 88.7 on


def saturated_logits(n, seed):
    """float32 logit vectors (x, y) of n >= 16 entries: 3 * randn with the eight SATURATED values spread over each
    (in a different order for y, so saturated x meet ordinary and saturated y alike)."""
    import torch
    g = torch.Generator().manual_seed(seed)
    x, y = 3 * torch.randn(n, generator=g), 3 * torch.randn(n, generator=g)
    pos = [(i * n) // 8 for i in range(8)]
    for k, i in enumerate(pos):
        x[i] = SATURATED[k]
        y[(i + 1) % n] = SATURATED[(3 * k + 1) % 8]
    return x, y


class adam_ref:
    """torch.optim.Adam (amsgrad off, L2 weight decay) step by step in fp64.  ``p``, ``m``, ``v``: lists of arrays, ``t``
    the steps taken.  For error bounds the last step also leaves ``g`` (the effective gradient grad * grad_scale +
    wd * p), ``gmag`` (|grad * grad_scale| + wd |p|: what g's rounding errors are relative to), ``den`` (sqrt(v / bc2) +
    eps) and ``upd`` (the subtracted update); ``mag`` / ``vmag`` run the recursions of m / v on gmag / gmag^2: what the
    moments' rounding errors are relative to when their sums cancel."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        self.p = [f64(q).copy() for q in params]
        self.m = [np.zeros_like(q) for q in self.p]
        self.v = [np.zeros_like(q) for q in self.p]
        self.mag = [np.zeros_like(q) for q in self.p]
        self.vmag = [np.zeros_like(q) for q in self.p]
        self.lr, self.betas, self.eps, self.wd, self.t = lr, betas, eps, weight_decay, 0

    def step(self, grads, grad_scale=1.0):
        self.t += 1
        b1, b2 = self.betas
        self.bc1, self.bc2 = 1.0 - b1 ** self.t, 1.0 - b2 ** self.t
        self.g, self.gmag, self.den, self.upd = [], [], [], []
        for i, g in enumerate(grads):
            g = f64(g) * grad_scale
            gm = np.abs(g) + self.wd * np.abs(self.p[i])
            g = g + self.wd * self.p[i]
            self.m[i] = b1 * self.m[i] + (1.0 - b1) * g
            self.v[i] = b2 * self.v[i] + (1.0 - b2) * g * g
            self.mag[i] = b1 * self.mag[i] + (1.0 - b1) * gm
            self.vmag[i] = b2 * self.vmag[i] + (1.0 - b2) * gm * gm
            den = np.sqrt(self.v[i]) / np.sqrt(self.bc2) + self.eps
            upd = self.lr / self.bc1 * self.m[i] / den
            self.p[i] = self.p[i] - upd
            self.g.append(g), self.gmag.append(gm), self.den.append(den), self.upd.append(upd)


def g32_geometry(H, W, elem_bytes):
    """(Hp, Wp, cpg): rows and columns of a G32 plane and its channels per 32-byte group."""
    return (H + 31) // 32 * 32 + 6, (W + 31) // 32 * 32 + 2, 32 // elem_bytes


def to_g32_ref(x, cpg, mean=None, inv_std=None):
    """The interior [B][groups][H][W][cpg] of a G32 buffer holding the NCHW array x: channel c is element c % cpg of
    group c // cpg, the channels past C of the last group are zero, channels < 4 are (x - mean[c]) * inv_std[c] when an
    affine is given."""
    x = f64(x).copy()
    B, C_, H, W = x.shape
    if mean is not None:
        for c in range(min(4, C_)):
            x[:, c] = (x[:, c] - float(mean[c])) * float(inv_std[c])
    ng = (C_ + cpg - 1) // cpg
    out = np.zeros((B, ng * cpg, H, W))
    out[:, :C_] = x
    return out.reshape(B, ng, cpg, H, W).transpose(0, 1, 3, 4, 2)


def from_g32_ref(g, C_, inv_std=None):
    """The NCHW array of channels [0, C_) of the G32 interior g ([B][groups][H][W][cpg]); with an affine, channels
    < 4 are multiplied by inv_std[c] (the adjoint of to_g32_ref's normalisation: the mean drops out)."""
    g = f64(g)
    B, ng, H, W, cpg = g.shape
    out = g.transpose(0, 1, 4, 2, 3).reshape(B, ng * cpg, H, W)[:, :C_].copy()
    if inv_std is not None:
        for c in range(min(4, C_)):
            out[:, c] *= float(inv_std[c])
    return out
