"""fp64 restatements of the folded nearest-x3 up-conv (include/esrgan_hip.h: esr_fold3, esr_pool modes 4 / 5), written
from the header's index formulas.  tests/test_scales_host.py pins them against ``interpolate(nearest, 3)`` + ``conv2d``;
tests/test_gpu_scales.py holds the kernels to them."""
import torch


def off(p, k):
    """Low-resolution offset that tap k of output phase p reads: (-1, 0, 0), (0, 0, 0), (0, 0, +1)."""
    return (p + k - 1) // 3


def fold3(w, b=None):
    """w [cout, cin, 3, 3] (+ bias) -> [9 cout, cin, 3, 3] (+ [9 cout]), phase-major: channel (3p + q) cout + co."""
    cout = w.shape[0]
    wf = torch.zeros((9 * cout,) + tuple(w.shape[1:]), dtype=w.dtype)
    for p in range(3):
        for q in range(3):
            blk = wf[(3 * p + q) * cout:(3 * p + q + 1) * cout]
            for kh in range(3):
                for kw in range(3):
                    blk[:, :, off(p, kh) + 1, off(q, kw) + 1] += w[:, :, kh, kw]
    return wf, (b.repeat(9) if b is not None else None)


def unfold3(gwf, gbf=None):
    """The adjoint of fold3: gradients of the folded weights / biases -> those of the 3x3 conv."""
    cout = gwf.shape[0] // 9
    gw = torch.zeros((cout,) + tuple(gwf.shape[1:]), dtype=gwf.dtype)
    for p in range(3):
        for q in range(3):
            blk = gwf[(3 * p + q) * cout:(3 * p + q + 1) * cout]
            for kh in range(3):
                for kw in range(3):
                    gw[:, :, kh, kw] += blk[:, :, off(p, kh) + 1, off(q, kw) + 1]
    return gw, (gbf.view(9, cout).sum(0) if gbf is not None else None)


def shuffle3(z):
    """z [B, 9 C, h, w] -> y [B, C, 3h, 3w] with y[b][c][3h+i][3w+j] = z[b][(3i + j) C + c][h][w]."""
    B, C9, h, w = z.shape
    return z.reshape(B, 3, 3, C9 // 9, h, w).permute(0, 3, 4, 1, 5, 2).reshape(B, C9 // 9, 3 * h, 3 * w)


def unshuffle3(y):
    """The inverse (and adjoint) of shuffle3."""
    B, C_, H, W = y.shape
    return y.reshape(B, C_, H // 3, 3, W // 3, 3).permute(0, 3, 5, 1, 2, 4).reshape(B, 9 * C_, H // 3, W // 3)
