"""Fused train-step losses (csrc/loss_kernels.hip, esrganplus_amd/losses.py) against the torch formulas the
reference uses: nn.L1Loss (cri_pix / cri_fea) and GANLoss('vanilla') on the relativistic-average logits
(codes/models/modules/loss.py:6-38, SRRaGAN_model.py:124-137,150-156) — values and gradients."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import fp64_refs as R
from tests.conftest import checks  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.mark.parametrize('shape', [(16, 3, 128, 128), (16, 512, 8, 8), (3, 5, 7, 11), (1, 1, 1, 3)])
def test_l1_loss_and_gradient(dev, shape):
    from esrganplus_amd import losses as LS
    g = torch.Generator().manual_seed(sum(shape))
    a0 = torch.randn(shape, generator=g).to(dev)
    b = torch.randn(shape, generator=g).to(dev)
    b.view(-1)[::7] = a0.view(-1)[::7]                  # exact ties: sign(0) = 0 like torch
    res = []
    for fn in (lambda a: 0.37 * F.l1_loss(a, b), lambda a: LS.l1_loss(a, b, 0.37)):
        a = a0.clone().requires_grad_(True)
        loss = fn(a)
        (loss * 1024.0).backward()
        res.append((loss.detach(), a.grad))
    (l0, g0), (l1, g1) = res
    assert abs(l0.item() - l1.item()) <= 1e-6 * max(1.0, abs(l0.item()))
    assert torch.allclose(g0, g1, rtol=1e-6, atol=0)
    for _ in range(2):                                  # the scratch is left clean: same answer again
        assert LS.l1_loss(a0, b, 0.37).item() == l1.item()


@pytest.mark.parametrize('n', [16, 1, 37, 300])
@pytest.mark.parametrize('mode', ['g_step', 'd_step'])
def test_ragan_loss_and_gradients(dev, n, mode):
    from esrganplus_amd import losses as LS
    g = torch.Generator().manual_seed(n)
    x0 = (3 * torch.randn(n, 1, generator=g)).to(dev)
    y0 = (3 * torch.randn(n, 1, generator=g)).to(dev)
    w = 5e-3 if mode == 'g_step' else 1.0
    tx, ty = (False, True) if mode == 'g_step' else (True, False)

    def ref(x, y):
        t = lambda v, r: torch.ones_like(v) if r else torch.zeros_like(v)
        lx = F.binary_cross_entropy_with_logits(x - y.mean(), t(x, tx))
        ly = F.binary_cross_entropy_with_logits(y - x.mean(), t(y, ty))
        return w * (lx + ly) / 2, torch.stack([x.detach().mean(), y.detach().mean(), lx.detach(), ly.detach()])

    out = []
    for fn in (ref, lambda x, y: LS.ragan_loss(x, y, tx, ty, w)):
        x = x0.clone().requires_grad_(mode == 'd_step')           # G step: x = pred_d_real, detached
        y = y0.clone().requires_grad_(True)
        loss, aux = fn(x, y)
        (loss * 1024.0).backward()
        out.append((loss.detach(), aux, x.grad, y.grad))
    (l0, a0, gx0, gy0), (l1, a1, gx1, gy1) = out
    assert abs(l0.item() - l1.item()) <= 2e-6 * max(1e-3, abs(l0.item()))
    assert torch.allclose(a0, a1, rtol=1e-5, atol=1e-6)
    assert torch.allclose(gy0, gy1, rtol=1e-4, atol=1e-7 * 1024 * w)
    if mode == 'd_step':
        assert torch.allclose(gx0, gx1, rtol=1e-4, atol=1e-7 * 1024 * w)
    else:
        assert gx1 is None and not a1.requires_grad


# ---------------------------------------------------------------------------------------------------------------------
# The same kernels against plain fp64 (tests/fp64_refs.py, pinned to torch's float64 in tests/test_fp64_refs.py), at
# the sizes where they take another path, through the raw entry points the hand-written train step calls.
# ---------------------------------------------------------------------------------------------------------------------
U = R.U                       # 2^-24
W32 = float(np.float32(0.37))
SENTINEL = -77.25


def _scratch_is_clean(dev):
    from esrganplus_amd import losses as LS
    s = LS._scratch[dev].cpu()
    assert s[0].item() == 0.0 and s.view(torch.int64)[1].item() == 0, s


def _l1_check(name, loss, grad, a, b, scale):
    """Loss and gradient magnitude within 4 * 2^-24 relative of l1_ref, signs exact.  Returns the measured maxima in
    units of 2^-24."""
    l_ref, g_ref = R.l1_ref(a, b, W32, scale)
    el = abs(float(loss) - l_ref) / l_ref if l_ref else abs(float(loss))
    assert el <= 4 * U, (name, el / U)
    eg = 0.0
    if grad is not None:
        g = R.f64(grad)
        assert (np.sign(g) == np.sign(g_ref)).all(), name
        nz = g_ref != 0
        if nz.any():
            eg = float((np.abs(g[nz] - g_ref[nz]) / np.abs(g_ref[nz])).max())
        assert eg <= 4 * U, (name, eg / U)
    return el / U, eg / U


L1_SCALINGS = [(1.0, None), (1024.0, None), (1.0, 0.125), (1024.0, 0.125)]      # (grad_scale, scale_dev)


@pytest.mark.parametrize('n', [1, 3, 4, 5, 4095, 4096, 4097, 4 * 1024 * 1024 + 5])
def test_l1_raw_and_l1_loss_against_fp64(dev, n):
    """l1_raw (every grad_scale / scale_dev combination, and grad_out=None) and l1_loss on flat tensors of n
    elements; 4 Mi + 5 is past the launcher's 1024 workgroups x 4096 elements, so the grid-stride loop runs a second
    pass that ends in the scalar tail.

    Tolerance: the kernel rounds a - b once (relative 2^-24 on each |a - b|, hence on their sum), adds in fp64, rounds
    the mean to fp32 and rounds its product with the weight: 3 roundings on the loss.  The gradient magnitude is
    ((weight / n) * grad_scale) * scale_dev: 3 roundings (n < 2^24 converts exactly, fp32 division is correctly
    rounded).  Both are held to 4 * 2^-24 relative of l1_ref given the fp32-rounded weight; signs, and the zeros of
    exact ties, are exact.  After every call the fp64 scratch reads back as [0.0, 0]."""
    from esrganplus_amd import losses as LS
    g = torch.Generator().manual_seed(n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    if n > 1:
        b[::7] = a[::7]                                   # exact ties: gradient exactly 0
    ties = slice(0, n if n > 1 else 0, 7)
    ad, bd = a.to(dev), b.to(dev)
    worst = [0.0, 0.0]
    for gs, sd in L1_SCALINGS:
        out = torch.full((n,), SENTINEL, device=dev)
        sdev = None if sd is None else torch.tensor([sd], device=dev)
        loss = LS.l1_raw(ad, bd, 0.37, grad_out=out, grad_scale=gs, scale_dev=sdev)
        _scratch_is_clean(dev)
        assert (out[ties] == 0).all()
        e = _l1_check('l1_raw gs=%g sd=%s' % (gs, sd), loss.item(), out, a, b, gs * (sd or 1.0))
        worst = [max(w, v) for w, v in zip(worst, e)]
    # grad_out=None: the loss alone; a buffer the caller might have passed is not touched
    cand = torch.full((n,), SENTINEL, device=dev)
    first = LS.l1_raw(ad, bd, 0.37, grad_out=None, grad_scale=1024.0).item()
    _scratch_is_clean(dev)
    assert (cand == SENTINEL).all()
    _l1_check('l1_raw grad_out=None', first, None, a, b, 1.0)
    for _ in range(2):                                    # the scratch is left clean: same answer again
        assert LS.l1_raw(ad, bd, 0.37).item() == first
    # the autograd face of the same kernel
    ag = ad.clone().requires_grad_(True)
    loss = LS.l1_loss(ag, bd, 0.37)
    _scratch_is_clean(dev)
    (loss * 1024.0).backward()
    e = _l1_check('l1_loss', loss.item(), ag.grad, a, b, 1024.0)       # the upstream factor is a power of two: exact
    assert loss.item() == first
    worst = [max(w, v) for w, v in zip(worst, e)]
    print('l1 n=%d: max relative error loss %.2f, gradient %.2f (bound 4) x 2^-24' % (n, worst[0], worst[1]))


@pytest.mark.parametrize('which', ['a', 'b', 'grad_out', 'all'])
@pytest.mark.parametrize('k', [1, 2, 3])
def test_l1_raw_misaligned_views(dev, which, k):
    """Views base[k : k + n] whose data pointer is 4k bytes off a 16-byte boundary, for a, b, grad_out and all three:
    the kernel's scalar path must give the aligned call's numbers (n = 4097: if the alignment test were wrong the
    vector body would run on 1024 of the quads).  Same bounds as test_l1_raw_and_l1_loss_against_fp64."""
    from esrganplus_amd import losses as LS
    n = 4097
    g = torch.Generator().manual_seed(100 + k)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    b[::7] = a[::7]

    def place(t, off):
        base = torch.full((n + 8,), SENTINEL, device=dev)
        base[off:off + n] = t.to(dev)
        return base, base[off:off + n]

    ka, kb, kg = (k if which in ('a', 'all') else 0), (k if which in ('b', 'all') else 0), (k if which in ('grad_out', 'all') else 0)
    (_, av), (_, bv) = place(a, ka), place(b, kb)
    gbase, gv = place(torch.full((n,), SENTINEL), kg)
    for t, off in ((av, ka), (bv, kb), (gv, kg)):
        assert t.data_ptr() % 16 == 4 * off and t.is_contiguous()
    loss = LS.l1_raw(av, bv, 0.37, grad_out=gv, grad_scale=1024.0)
    _scratch_is_clean(dev)
    e = _l1_check('misaligned %s k=%d' % (which, k), loss.item(), gv, a, b, 1024.0)
    assert (gbase[:kg] == SENTINEL).all() and (gbase[kg + n:] == SENTINEL).all()      # nothing outside the view
    aligned = torch.empty(n, device=dev)
    assert LS.l1_raw(a.to(dev), b.to(dev), 0.37, grad_out=aligned, grad_scale=1024.0).item() == loss.item()
    assert torch.equal(aligned, gv)
    print('l1 misaligned %s k=%d: loss %.2f, gradient %.2f (bound 4) x 2^-24' % (which, k, e[0], e[1]))


# ---- RaGAN ----------------------------------------------------------------------------------------------------------
LIBM = 4          # expf / log1pf are taken as accurate to 2 ulp = 4 * 2^-24 relative


def _ragan_bounds(x, y, tx, ty, n_local=None, extra=0):
    """Error bounds of ragan_loss_kernel's outputs in units of the fp64 reference quantities, from its operation
    count (c = ceil(n / 256) is the length of a thread's add chain, n the logits of ONE launch):

    * a block sum is c chained adds, 6 shuffle steps and 3 adds over the waves: S = c + 9 roundings, each relative to
      at most sum|term|; a mean is that sum times inv = fl(1 / n): 2 more.  k_mean = c + 11.
      -> |mean_x - ref| <= k_mean 2^-24 mean|x| =: dm_x (same for y);
    * z1_i = fl(x_i - mean_y) is off by dz1_i = dm_y + 2^-24 |z1_i|;
    * a BCE term softplus(z) - t z: expf LIBM, log1pf LIBM more on a value <= ln 2, the add to max(z, 0) one, the
      subtraction of t z one (t z is exact): (2 LIBM + 2) 2^-24 (softplus(z) + t |z|) =: 10 2^-24 T_i, and it moves by
      at most dz_i with z (its slope sigmoid(z) - t is within [-1, 1]);
      -> |bce_x - ref| <= (k_mean + 10) 2^-24 mean(T1) + mean(dz1);
      -> loss = hw (t0 + t1) inv: one more add and one more product:
         |loss - ref| <= hw ((k_mean + 12) 2^-24 (mean T1 + mean T2) + mean dz1 + mean dz2);
    * D1_i = sigmoid(z1_i) - tx: expf LIBM, 1 + e and 1 / . one each, the subtraction one: 7 2^-24 absolute (|D| <= 1),
      plus dz1_i / 4 (the sigmoid's slope is at most 1/4);
    * the mean share t3 * ninv: (k_mean 2^-24 mean|D2| + mean(7 2^-24 + dz2 / 4));
    * gs = ((hw inv) grad_scale) scale_dev: 4 roundings with inv's; the subtraction and the product with gs one each:
      |grad_x_i - ref_i| <= |gs| ((14 + k_mean mean|D2|) 2^-24 + (dz1_i + mean dz2) / 4) + 6 2^-24 |ref_i|.

    ``extra`` roundings are added to k_mean where the sums were combined outside the kernel (emulated ranks: the
    host adds the per-shard fp32 sums in fp64 and rounds once to fp32)."""
    x, y = R.f64(x), R.f64(y)
    n = x.size if n_local is None else n_local
    k = -(-n // 256) + 11 + extra
    mx, my = x.mean(), y.mean()
    z1, z2 = x - my, y - mx
    dmx, dmy = k * U * np.abs(x).mean(), k * U * np.abs(y).mean()
    dz1, dz2 = dmy + U * np.abs(z1), dmx + U * np.abs(z2)
    T1, T2 = R.softplus(z1) + tx * np.abs(z1), R.softplus(z2) + ty * np.abs(z2)
    D1, D2 = R.sigmoid(z1) - tx, R.sigmoid(z2) - ty
    return dict(k=k, dmx=dmx, dmy=dmy, dz1=dz1, dz2=dz2, T1=T1, T2=T2, D1=D1, D2=D2)


def _ragan_tols(x, y, tx, ty, hw, gs, shard=None, n_local=None, extra=0):
    """(tolerances of loss, aux[4], grad_x, grad_y) for a launch over the whole of (x, y), or — shard = slice — for
    the BCE means and gradients of that shard of a global batch (x, y) whose means are global.  hw = weight / 2; gs:
    the gradient's whole factor hw / n * grad_scale * scale_dev."""
    q = _ragan_bounds(x, y, tx, ty, n_local, extra)
    s = slice(None) if shard is None else shard
    k = q['k']
    bx = (k + 2 * LIBM + 2) * U * q['T1'][s].mean() + q['dz1'][s].mean()
    by = (k + 2 * LIBM + 2) * U * q['T2'][s].mean() + q['dz2'][s].mean()
    tl = hw * ((k + 2 * LIBM + 4) * U * (q['T1'][s].mean() + q['T2'][s].mean()) + q['dz1'][s].mean() + q['dz2'][s].mean())
    ref_gx, ref_gy = abs(gs) * (q['D1'] - q['D2'].mean()), abs(gs) * (q['D2'] - q['D1'].mean())
    sig = 2 * (LIBM + 3)
    tgx = abs(gs) * ((sig + k * np.abs(q['D2']).mean()) * U + (q['dz1'] + q['dz2'].mean()) / 4) + 6 * U * np.abs(ref_gx)
    tgy = abs(gs) * ((sig + k * np.abs(q['D1']).mean()) * U + (q['dz2'] + q['dz1'].mean()) / 4) + 6 * U * np.abs(ref_gy)
    return tl, np.array([q['dmx'], q['dmy'], bx, by]), tgx[s], tgy[s]


def _ratio(got, want, tol):
    got, want = R.f64(got), np.asarray(want, dtype=np.float64)
    assert np.isfinite(got).all()
    return float((np.abs(got - want) / tol).max())


def _ragan_inputs(n):
    if n >= 16:
        return R.saturated_logits(n, n)
    g = torch.Generator().manual_seed(n)
    return 3 * torch.randn(n, generator=g), 3 * torch.randn(n, generator=g)


@pytest.mark.parametrize('tx,ty', [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize('n', [1, 16, 63, 64, 65, 255, 256, 257, 1000])
def test_ragan_raw_and_ragan_loss_against_fp64(dev, n, tx, ty):
    """ragan_raw (weight x grad_scale x scale_dev, grad_x / grad_y present or absent) and ragan_loss against
    ragan_ref, all four target pairs, n on the wave and block boundaries of the one-workgroup kernel.  From n = 16 the
    logits hold +-30, +-88, +-100 and +-1e4 among 3 * randn: expf overflows there, everything returned must be finite
    and the saturated entries' gradients gs * ((0 or +-1) - mean share).  Bounds: _ragan_bounds (k_mean =
    ceil(n / 256) + 11); the printed figures are measured error / bound."""
    from esrganplus_amd import losses as LS
    x, y = _ragan_inputs(n)
    xd, yd = x.to(dev), y.to(dev)
    worst = {}

    def note(key, r):
        worst[key] = max(worst.get(key, 0.0), r)

    cases = [(1.0, 1.0, None, True, True), (5e-3, 1024.0, None, True, True), (5e-3, 1.0, 0.125, True, False),
             (1.0, 1024.0, 0.125, False, True), (5e-3, 1024.0, 0.125, False, False)]
    for w, gsc, sd, want_gx, want_gy in cases:
        w32 = float(np.float32(w))
        l_ref, aux_ref, gx_ref, gy_ref = R.ragan_ref(x, y, tx, ty, w32)
        f = gsc * (sd or 1.0)
        tl, taux, tgx, tgy = _ragan_tols(x, y, tx, ty, 0.5 * w32, 0.5 * w32 / n * f)
        gx = torch.full((n,), SENTINEL, device=dev) if want_gx else None
        gy = torch.full((n,), SENTINEL, device=dev) if want_gy else None
        sdev = None if sd is None else torch.tensor([sd], device=dev)
        loss, aux = LS.ragan_raw(xd, yd, bool(tx), bool(ty), w, grad_x=gx, grad_y=gy, grad_scale=gsc, scale_dev=sdev)
        note('loss', _ratio(loss, l_ref, tl))
        note('aux', _ratio(aux, aux_ref, taux))
        if want_gx:
            note('grad', _ratio(gx, gx_ref * f, tgx))
        if want_gy:
            note('grad', _ratio(gy, gy_ref * f, tgy))
        if n >= 16 and want_gx and want_gy:
            # saturated entries: sigmoid is 0 or 1 there, so the gradient is gs * ((0 or 1) - t - mean share)
            q = _ragan_bounds(x, y, tx, ty)
            for got, z, t, Dm, tol in ((gx, R.f64(x) - R.f64(y).mean(), tx, q['D2'].mean(), tgx),
                                       (gy, R.f64(y) - R.f64(x).mean(), ty, q['D1'].mean(), tgy)):
                sat = np.abs(z) >= 80
                assert sat.sum() >= 4
                want = 0.5 * w32 / n * f * (((z[sat] > 0) * 1.0 - t) - Dm)
                note('saturated', _ratio(got.cpu()[torch.from_numpy(sat)], want, tol[sat] + 1e-30))
    # the autograd face, both operands differentiable
    xa, ya = xd.clone().requires_grad_(True), yd.clone().requires_grad_(True)
    loss, aux = LS.ragan_loss(xa.view(n, 1), ya.view(n, 1), bool(tx), bool(ty), 5e-3)
    (loss * 1024.0).backward()
    w32 = float(np.float32(5e-3))
    l_ref, aux_ref, gx_ref, gy_ref = R.ragan_ref(x, y, tx, ty, w32)
    tl, taux, tgx, tgy = _ragan_tols(x, y, tx, ty, 0.5 * w32, 0.5 * w32 / n * 1024.0)
    note('loss', _ratio(loss, l_ref, tl))
    note('aux', _ratio(aux, aux_ref, taux))
    note('grad', _ratio(xa.grad, gx_ref * 1024.0, tgx))
    note('grad', _ratio(ya.grad, gy_ref * 1024.0, tgy))
    print('ragan n=%d t=(%d,%d): measured / bound ' % (n, tx, ty) + ', '.join('%s %.3f' % kv for kv in sorted(worst.items())))
    assert all(v <= 1.0 for v in worst.values()), worst


def _ragan_launch(dev, x, y, tx, ty, w, mode, sums=None, ext=None, grads=False):
    """One launch of esr_ragan_loss_forward the way losses.ragan_raw drives it."""
    import ctypes as C
    from esrganplus_amd import _lib as L, engine as E
    n = x.numel()
    loss = torch.full((), SENTINEL, device=dev)
    out = torch.full((4,), SENTINEL, device=dev)
    gx = torch.full((n,), SENTINEL, device=dev) if grads else None
    gy = torch.full((n,), SENTINEL, device=dev) if grads else None
    p = L.esr_ragan_loss()
    p.x, p.y, p.n = x.data_ptr(), y.data_ptr(), n
    p.tx, p.ty, p.weight, p.mode = float(tx), float(ty), float(w), mode
    p.loss, p.mean_x, p.mean_y = loss.data_ptr(), out.data_ptr(), out.data_ptr() + 4
    p.bce_x, p.bce_y = out.data_ptr() + 8, out.data_ptr() + 12
    if sums is not None:
        p.sums = sums.data_ptr()
    if ext is not None:
        p.ext = ext.data_ptr()
    if grads:
        p.grad_x, p.grad_y = gx.data_ptr(), gy.data_ptr()
    L.check(L.lib().esr_ragan_loss_forward(C.byref(p), C.c_void_p(E.current_stream())), 'esr_ragan_loss_forward')
    torch.cuda.synchronize()
    return loss, out, gx, gy


@pytest.mark.parametrize('tx,ty', [(0, 1), (1, 0)])
@pytest.mark.parametrize('n', [1, 16, 37])
def test_ragan_global_mean_modes_with_emulated_ranks(dev, n, tx, ty):
    """Modes 1-3 (the data-parallel "global means" path) on one GPU without a process group: a global batch of
    N = 3 n logits in R = 3 shards, the two all-reduces done by hand (per-shard fp32 sums added in fp64 on the host and
    written back as fp32).  Mode 1 returns the shard's {sum x, sum y}; mode 2 the global means, the shard's BCE means
    against them, and losses whose mean over the shards is ragan_ref of the whole batch; the concatenated mode-3
    gradients are R x the gradient of the whole-batch loss (_RaGANGlobalFn: the ranks' gradients are averaged
    afterwards).  With R = 3 the local 1 / n and the global 1 / N differ by 3, so exchanging them anywhere fails at
    O(1).  Bounds: _ragan_bounds with the shard's n in the chain length and 2 more roundings for the host's sums."""
    Rk, w = 3, 5e-3
    N = Rk * n
    g = torch.Generator().manual_seed(1000 + n)
    x, y = 3 * torch.randn(N, generator=g) + 0.7, 3 * torch.randn(N, generator=g) - 0.4
    w32 = float(np.float32(w))
    shards = [slice(r * n, (r + 1) * n) for r in range(Rk)]
    xs, ys = [x[s].to(dev) for s in shards], [y[s].to(dev) for s in shards]
    worst = {}

    def note(key, r):
        worst[key] = max(worst.get(key, 0.0), r)

    # mode 1: rank-local sums
    c9 = -(-n // 256) + 9
    tot = np.zeros(2)
    for r in range(Rk):
        sums = torch.full((2,), SENTINEL, device=dev)
        _ragan_launch(dev, xs[r], ys[r], tx, ty, w, 1, sums=sums)
        want = np.array([R.f64(x[shards[r]]).sum(), R.f64(y[shards[r]]).sum()])
        tol = c9 * U * np.array([R.f64(x[shards[r]]).__abs__().sum(), R.f64(y[shards[r]]).__abs__().sum()])
        note('mode1 sums', _ratio(sums, want, tol))
        tot += R.f64(sums)
    ext = torch.tensor([tot[0], tot[1], float(N), 0.0, 0.0], dtype=torch.float32, device=dev)
    # mode 2: loss and aux from the global means, rank-local sums of sigmoid(z) - t
    l_ref, aux_ref, gx_ref, gy_ref = R.ragan_ref(x, y, tx, ty, w32)
    q = _ragan_bounds(x, y, tx, ty, n_local=n, extra=2)
    losses, dtot = [], np.zeros(2)
    for r in range(Rk):
        s = shards[r]
        dsum = torch.full((2,), SENTINEL, device=dev)
        loss, out, _, _ = _ragan_launch(dev, xs[r], ys[r], tx, ty, w, 2, sums=dsum, ext=ext)
        tl, taux, _, _ = _ragan_tols(x, y, tx, ty, 0.5 * w32, 0.0, shard=s, n_local=n, extra=2)
        z1, z2 = R.f64(x)[s] - aux_ref[1], R.f64(y)[s] - aux_ref[0]
        bce = [(R.softplus(z1) - tx * z1).mean(), (R.softplus(z2) - ty * z2).mean()]
        note('mode2 aux', _ratio(out, [aux_ref[0], aux_ref[1], bce[0], bce[1]], taux))
        note('mode2 shard loss', _ratio(loss, 0.5 * w32 * (bce[0] + bce[1]), tl))
        # the sums of D = sigmoid(z) - t over the shard: c + 9 roundings on terms good to 7 2^-24 + dz / 4
        want = np.array([q['D1'][s].sum(), q['D2'][s].sum()])
        tol = np.array([c9 * U * np.abs(q['D1'][s]).sum() + (7 * U + q['dz1'][s] / 4).sum(),
                        c9 * U * np.abs(q['D2'][s]).sum() + (7 * U + q['dz2'][s] / 4).sum()])
        note('mode2 dsum', _ratio(dsum, want, tol))
        losses.append(float(loss))
        dtot += R.f64(dsum)
    tl, _, tgx, tgy = _ragan_tols(x, y, tx, ty, 0.5 * w32, 0.5 * w32 / n, n_local=n, extra=2)
    note('mean of mode2 losses', abs(np.mean(losses) - l_ref) / tl)
    # mode 3: gradients from the global means and the global sums
    ext[3:5] = torch.tensor(dtot, dtype=torch.float32)
    gx, gy = [], []
    for r in range(Rk):
        _, _, a, b = _ragan_launch(dev, xs[r], ys[r], tx, ty, w, 3, ext=ext, grads=True)
        gx.append(a.cpu())
        gy.append(b.cpu())
    note('mode3 grad', _ratio(torch.cat(gx), Rk * gx_ref, tgx))
    note('mode3 grad', _ratio(torch.cat(gy), Rk * gy_ref, tgy))
    print('ragan ranks n=%d t=(%d,%d): measured / bound ' % (n, tx, ty) + ', '.join('%s %.3f' % kv for kv in sorted(worst.items())))
    assert all(v <= 1.0 for v in worst.values()), worst
