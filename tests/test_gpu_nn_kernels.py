"""The layer kernels of csrc/nn_kernels.hip called directly through the C ABI: BatchNorm (esr_batchnorm, all modes),
max-pool and pixel shuffle (esr_maxpool2) and Linear (esr_linear_op), each against a float64 torch reference computed
on the same stored values (fp16 inputs are rounded to fp16 first).  The networks reach these kernels only at a few
fixed shapes; here they run at ragged channel counts (partial channel groups), pixel counts that leave partial
256-pixel chunks, reduction chunkings the dispatch heuristic does not divide evenly, 1 / 2 / 4 statistics groups,
odd pooled maps, NaN / inf windows, and linear shapes that run the unrolled main loops with and without their tails.
Every reduction but the BatchNorm fp64 atomics has a fixed order, so repeated runs must agree bit for bit."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SENT = 1234.0          # exactly representable in fp16: marks G32 elements a kernel must not write
GUARD = 16             # sentinel entries behind every per-channel array
SLOPE = 0.2            # ESR_LRELU_SLOPE
MOM, EPS = 0.1, 1e-5   # nn.BatchNorm2d defaults (the plan's BN_MOMENTUM / BN_EPS)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _mods():
    from esrganplus_amd import engine as E, _lib as L
    return E, L


def seed_of(*args):
    return zlib.crc32(repr(args).encode())


def run(*ops):
    E, L = _mods()
    lst = L.OpList()
    for kind, field, st in ops:
        lst.add(kind, field, st)
    lst.run(E.current_stream())
    torch.cuda.synchronize()


def q(t, prec):
    """the values a G32 tensor of this precision stores"""
    return t.half().float() if prec == 'fp16' else t.float()


def g32(dev, prec, B, C_, H, W, fill=None):
    E, _ = _mods()
    b = E.G32(B, C_, H, W, prec, dev)
    if fill is not None:
        b.t.fill_(fill)
    return b


def upload(buf, x):
    """NCHW fp32 -> G32 with an OP_LAYOUT op (to_g32 = 1; channels past C are written as zeros)"""
    _, L = _mods()
    xd = x.float().contiguous().to(buf.t.device)
    lo = L.esr_layout()
    lo.dtype, lo.to_g32 = buf.esr_dtype, 1
    lo.B, lo.C, lo.H, lo.W = (int(s) for s in x.shape)
    lo.nchw, lo.g32 = xd.data_ptr(), buf.view(0, int(x.shape[1]))
    run((L.OP_LAYOUT, 'layout', lo))


def download(buf, C_):
    """G32 -> NCHW fp32 with an OP_LAYOUT op (to_g32 = 0)"""
    _, L = _mods()
    out = torch.empty(buf.B, C_, buf.H, buf.W, device=buf.t.device)
    lo = L.esr_layout()
    lo.dtype, lo.to_g32 = buf.esr_dtype, 0
    lo.B, lo.C, lo.H, lo.W = buf.B, C_, buf.H, buf.W
    lo.nchw, lo.g32 = out.data_ptr(), buf.view(0, C_)
    run((L.OP_LAYOUT, 'layout', lo))
    return out.cpu()


def region(buf, H=None, W=None):
    """all channel lanes of the G32 buffer's pixels [0, H) x [0, W) as NCHW (padding lanes included), and a mask of
    every other element of the buffer (halo, rows / columns past H / W)"""
    H = buf.H if H is None else H
    W = buf.W if W is None else W
    t = buf.t.float().cpu()
    inner = t[:, :, 1:H + 1, 1:W + 1, :].permute(0, 1, 4, 2, 3).reshape(buf.B, buf.ng * buf.cpg, H, W)
    rest = torch.ones(t.shape, dtype=torch.bool)
    rest[:, :, 1:H + 1, 1:W + 1, :] = False
    return inner, t[rest]


def guarded(vals, dtype, dev):
    """device array holding `vals` followed by GUARD sentinel entries (returned whole; check with guard_ok)"""
    full = torch.full((vals.numel() + GUARD,), SENT, dtype=dtype)
    full[:vals.numel()] = vals.reshape(-1).to(dtype)
    return full.to(dev)


def guard_ok(full):
    tail = full[-GUARD:].cpu()
    return bool((tail == SENT).all())


def body(full, n):
    return full[:n].cpu().double()


def act64(v, act):
    _, L = _mods()
    if act == L.ACT_LRELU:
        return F.leaky_relu(v, SLOPE)
    if act == L.ACT_RELU:
        return F.relu(v)
    return v


def act_grad_from_output(y, act):
    """derivative selected by the stored OUTPUT, the kernels' rule (act_bwd): equals the derivative at the
    pre-activation except where that is within round-off of 0, where the two references could disagree"""
    _, L = _mods()
    if act == L.ACT_LRELU:
        return torch.where(y > 0, 1.0, SLOPE).double()
    if act == L.ACT_RELU:
        return (y > 0).double()
    return torch.ones_like(y, dtype=torch.float64)


def assert_within(got, ref, tol, what):
    err = (got.double() - ref.double()).abs()
    bad = err > tol
    worst = (err / tol.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    assert not bad.any(), '%s: %d elements off, worst err %.3e (err/tol %.2f)' % (what, int(bad.sum()), err.max().item(), worst)
    return worst


# ----------------------------------------------------------------------------------------------------------------
# BatchNorm
# ----------------------------------------------------------------------------------------------------------------

def bn_ppt(B, C_, H, W, cpg):
    """bn_dispatch's chunking of the reduction passes (csrc/nn_kernels.hip): (256-pixel chunks, chunks per workgroup)"""
    chunks = (H * W + 255) // 256
    gy = (C_ + cpg - 1) // cpg
    ppt = 1
    while ppt < 16 and ((chunks + 2 * ppt - 1) // (2 * ppt)) * gy * B >= 1024:
        ppt *= 2
    return chunks, ppt


BN_SHAPES = [  # B, C, H, W, groups
    (5, 64, 1, 1, 1), (4, 3, 1, 1, 2), (8, 24, 1, 1, 4),
    (1, 3, 4, 4, 1), (4, 24, 4, 4, 2), (4, 64, 4, 4, 4),
    (6, 64, 7, 9, 2), (16, 3, 7, 9, 4), (3, 24, 7, 9, 1),
    (8, 3, 33, 40, 4), (12, 24, 33, 40, 4), (7, 64, 33, 40, 1),
    (32, 64, 60, 60, 1),                                    # 15 chunks (the last one partial): ppt 2 (fp16) / 4 (fp32)
    (32, 24, 128, 128, 2), (1, 64, 128, 128, 1),            # partial channel group with ppt 4
]
RAGGED_PPT = (32, 64, 60, 60, 1)


def test_bn_shapes_reach_the_ragged_reduction_paths():
    """Pins what the shape list is for, with bn_dispatch's own formula: a later change of the heuristic that drops a
    case fails here instead of silently narrowing the test."""
    for cpg in (16, 8):
        chunks, ppt = bn_ppt(*RAGGED_PPT[:4], cpg)
        B, C_, H, W, _ = RAGGED_PPT
        assert ppt > 1 and chunks % ppt != 0 and (H * W) % 256 != 0, (cpg, chunks, ppt)
    assert any(C_ % 16 and bn_ppt(B, C_, H, W, 8)[1] > 1 for B, C_, H, W, g in BN_SHAPES)
    assert {g for *_, g in BN_SHAPES} == {1, 2, 4}


class BNRig:
    def __init__(self, dev, prec, B, C_, H, W, groups, training, act, x):
        E, L = _mods()
        self.dev, self.prec, self.B, self.C, self.H, self.W = dev, prec, B, C_, H, W
        self.groups, self.training, self.act = groups, training, act
        self.dt = E._dt(prec)[0]
        self.xbuf = g32(dev, prec, B, C_, H, W)
        upload(self.xbuf, x)
        self.scratch = torch.zeros(2 * groups * C_, device=dev)   # mean / invstd for passes that do not use them

    def op(self, mode, **kw):
        _, L = _mods()
        o = L.esr_bn()
        o.dtype, o.mode, o.B, o.C, o.H, o.W = self.dt, mode, self.B, self.C, self.H, self.W
        o.training, o.act, o.momentum, o.eps, o.groups = self.training, self.act, MOM, EPS, self.groups
        o.x = self.xbuf.view(0, self.C)
        o.mean, o.invstd = self.scratch.data_ptr(), self.scratch.data_ptr() + 4 * self.groups * self.C
        for k, v in kw.items():
            if isinstance(v, torch.Tensor):
                v = v.data_ptr()
            elif hasattr(v, 'view') and hasattr(v, 'cpg'):
                v = v.view(0, self.C)
            setattr(o, k, v)
        return (L.OP_BN, 'bn', o)


def bn_stats_ref(x64, groups):
    """per group: mean, biased var, E[x^2], E|x|, sum x, sum x^2, sum |x| over (batch, H, W) — all [C]"""
    out = []
    for xg in x64.chunk(groups):
        m = xg.mean((0, 2, 3))
        out.append(dict(m=m, var=xg.var((0, 2, 3), unbiased=False), ex2=(xg * xg).mean((0, 2, 3)),
                        eabs=xg.abs().mean((0, 2, 3)), s0=xg.sum((0, 2, 3)), s1=(xg * xg).sum((0, 2, 3)),
                        sabs=xg.abs().sum((0, 2, 3))))
    return out


def inv_rel_tol(st):
    """relative invstd error the fp32 partial sums allow: E[x^2] - mean^2 cancels by E[x^2] / var"""
    return 1e-7 + 2e-6 * (st['ex2'] + 2 * st['m'].abs() * st['eabs']) / st['var']


def bn_inputs(seed, prec, B, C_, H, W, offset=2.0):
    rng = np.random.default_rng(seed)
    sd = rng.uniform(0.5, 2.0, C_)
    mu = rng.uniform(-offset, offset, C_) * sd
    x = torch.from_numpy((mu[None, :, None, None] + sd[None, :, None, None] * rng.standard_normal((B, C_, H, W)))).float()
    gamma = torch.from_numpy(rng.uniform(0.5, 1.5, C_) * rng.choice([-1.0, 1.0], C_)).float()
    beta = torch.from_numpy(rng.normal(0, 0.5, C_)).float()
    rm0 = torch.from_numpy(rng.normal(0, 1, C_)).float()
    rv0 = torch.from_numpy(rng.uniform(0.5, 2.0, C_)).float()
    g = torch.from_numpy(rng.standard_normal((B, C_, H, W))).float()
    dg0 = torch.from_numpy(rng.normal(0, 4, C_)).float()
    db0 = torch.from_numpy(rng.normal(0, 4, C_)).float()
    return q(x, prec), gamma, beta, rm0, rv0, q(g, prec), dg0, db0


@pytest.mark.parametrize('training', [1, 0])
@pytest.mark.parametrize('prec', ['fp32', 'fp16'])
@pytest.mark.parametrize('si', range(len(BN_SHAPES)))
def test_batchnorm_against_fp64(dev, si, prec, training):
    E, L = _mods()
    B, C_, H, W, groups = BN_SHAPES[si]
    act = (L.ACT_NONE, L.ACT_LRELU, L.ACT_RELU)[(si + training + (prec == 'fp16')) % 3]
    cpg = E._dt(prec)[2]
    x, gamma, beta, rm0, rv0, g, dg0, db0 = bn_inputs(1000 + 10 * si + 2 * training + (prec == 'fp16'), prec, B, C_, H, W)
    x64, gm64, bt64 = x.double(), gamma.double(), beta.double()
    N = B // groups * H * W
    rig = BNRig(dev, prec, B, C_, H, W, groups, training, act, x)
    gam, bet = gamma.to(dev), beta.to(dev)
    GC = groups * C_
    st = bn_stats_ref(x64, groups) if training else None

    # ---- forward: STATS + FINALIZE + APPLY (route 1) and STATS + FIN_APPLY (route 2), from the same sums
    nbt0 = 7
    sums = guarded(torch.zeros(2 * GC), torch.float64, dev)
    r1 = dict(mean=guarded(torch.zeros(GC), torch.float32, dev), invstd=guarded(torch.zeros(GC), torch.float32, dev),
              running_mean=guarded(rm0, torch.float32, dev), running_var=guarded(rv0, torch.float32, dev),
              num_batches_tracked=torch.full((1,), nbt0, dtype=torch.int64, device=dev), y=g32(dev, prec, B, C_, H, W, SENT))
    r2 = {k: (v.clone() if isinstance(v, torch.Tensor) else g32(dev, prec, B, C_, H, W, SENT)) for k, v in r1.items()}
    com = dict(sums=sums, gamma=gam, beta=bet)
    if training:
        run(rig.op(L.BN_STATS, sums=sums))
        run(rig.op(L.BN_FINALIZE, **com, **r1), rig.op(L.BN_APPLY, **com, **r1))
        run(rig.op(L.BN_FIN_APPLY, **com, **r2))
    else:
        run(rig.op(L.BN_FINALIZE, **com, **r1), rig.op(L.BN_APPLY, **com, **r1))
    for k in ('mean', 'invstd', 'running_mean', 'running_var', 'sums'):
        assert guard_ok(r1[k] if k != 'sums' else sums), k + ' written past its end'

    # reference: F.batch_norm in float64, once per group in group order
    rm, rv = rm0.double().clone(), rv0.double().clone()
    yref = torch.cat([act64(F.batch_norm(xg, rm, rv, gm64, bt64, bool(training), MOM, EPS), act)
                      for xg in x64.chunk(groups)])
    if training:
        s = body(sums, 2 * GC).view(groups, 2, C_)
        for q_, sq in enumerate(st):
            assert_within(s[q_, 0], sq['s0'], 4e-6 * sq['sabs'], 'sum x')
            assert_within(s[q_, 1], sq['s1'], 4e-6 * sq['s1'], 'sum x^2')
        mref = torch.stack([sq['m'] for sq in st])
        iref = torch.stack([1 / (sq['var'] + EPS).sqrt() for sq in st])
        itol = torch.stack([inv_rel_tol(sq) for sq in st])
        mtol = torch.stack([4e-6 * sq['eabs'] for sq in st])
    else:
        mref = rm0.double().expand(groups, C_)
        iref = (1 / (rv0.double() + EPS).sqrt()).expand(groups, C_)
        itol = torch.full((groups, C_), 1e-6, dtype=torch.float64)
        mtol = torch.zeros(groups, C_, dtype=torch.float64)
    mean_k, inv_k = body(r1['mean'], GC).view(groups, C_), body(r1['invstd'], GC).view(groups, C_)
    assert_within(mean_k, mref, mtol + 2 ** -24 * mref.abs(), 'mean')
    assert_within(inv_k, iref, itol * iref, 'invstd')

    # y: per-element bound from the fp32 arithmetic of (x - mean) * invstd * gamma + beta and the statistics' error
    xs = lambda t: t.view(groups, B // groups, C_, H, W)  # noqa: E731
    mexp, iexp, texp = mref[:, None, :, None, None], iref[:, None, :, None, None], itol[:, None, :, None, None]
    xh = (xs(x64) - mexp) * iexp
    gm, bt = gm64[None, None, :, None, None], bt64[None, None, :, None, None]
    ytol = 4e-6 * (gm.abs() * (xs(x64).abs() + mexp.abs()) * iexp + bt.abs()) + (gm * xh).abs() * texp + \
        mtol[:, None, :, None, None] * iexp * gm.abs()
    ytol = ytol.reshape(B, C_, H, W)
    if prec == 'fp16':
        ytol = ytol + 2 ** -11 * yref.abs() + 2 ** -24
    y_k = download(r1['y'], C_)
    assert_within(y_k, yref, ytol, 'y')
    inner, rest = region(r1['y'])
    assert (inner[:, C_:] == 0).all(), 'padding lanes of y not zero'
    assert (rest == SENT).all(), 'APPLY wrote outside the image'

    nbt = int(r1['num_batches_tracked'].item())
    if training:
        rtol_m = 1e-6 * (rm.abs() + rm0.double().abs()) + MOM * mtol.sum(0)
        vtol_each = torch.stack([2 * sq['var'] * inv_rel_tol(sq) for sq in st])
        rtol_v = 1e-6 * (rv.abs() + rv0.double().abs()) + MOM * N / (N - 1) * vtol_each.sum(0)
        assert_within(body(r1['running_mean'], C_), rm, rtol_m, 'running_mean')
        assert_within(body(r1['running_var'], C_), rv, rtol_v, 'running_var')
        assert nbt == nbt0 + groups
        # route 2 (FIN_APPLY) equals route 1 bit for bit
        for k in ('mean', 'invstd', 'running_mean', 'running_var', 'num_batches_tracked'):
            assert torch.equal(r2[k], r1[k]), k
        assert torch.equal(r2['y'].t, r1['y'].t)
        # RESTAT: another forward over the same batch, groups in reverse order
        run(rig.op(L.BN_RESTAT, **com, **r1))
        for xg in reversed(x64.chunk(groups)):
            F.batch_norm(xg, rm, rv, gm64, bt64, True, MOM, EPS)
        assert_within(body(r1['running_mean'], C_), rm, 2 * rtol_m, 'running_mean after RESTAT')
        assert_within(body(r1['running_var'], C_), rv, 2 * rtol_v, 'running_var after RESTAT')
        assert int(r1['num_batches_tracked'].item()) == nbt0 + 2 * groups
        assert guard_ok(r1['running_mean']) and guard_ok(r1['running_var'])
    else:
        assert torch.equal(r1['running_mean'].cpu()[:C_], rm0) and torch.equal(r1['running_var'].cpu()[:C_], rv0)
        assert nbt == nbt0

    # ---- backward: BWD_REDUCE, then BWD_FINAL + BWD_APPLY (route 1) or BWD_APPLY with dgamma set (route 2)
    gbuf = g32(dev, prec, B, C_, H, W)
    upload(gbuf, g)
    sums_b = guarded(torch.zeros(2 * GC), torch.float64, dev)
    gx1, gx2 = g32(dev, prec, B, C_, H, W, SENT), g32(dev, prec, B, C_, H, W, SENT)
    dgb1 = [guarded(dg0, torch.float32, dev), guarded(db0, torch.float32, dev)]
    dgb2 = [t.clone() for t in dgb1]
    bcom = dict(y=r1['y'], g=gbuf, sums=sums_b, mean=r1['mean'], invstd=r1['invstd'], gamma=gam, beta=bet)
    run(rig.op(L.BN_BWD_REDUCE, **bcom))
    run(rig.op(L.BN_BWD_FINAL, dgamma=dgb1[0], dbeta=dgb1[1], **bcom), rig.op(L.BN_BWD_APPLY, gx=gx1, **bcom))
    run(rig.op(L.BN_BWD_APPLY, gx=gx2, dgamma=dgb2[0], dbeta=dgb2[1], **bcom))
    assert torch.equal(gx1.t, gx2.t) and torch.equal(dgb1[0], dgb2[0]) and torch.equal(dgb1[1], dgb2[1])
    assert guard_ok(sums_b) and guard_ok(dgb1[0]) and guard_ok(dgb1[1])

    # reference: float64 autograd of F.batch_norm; the activation's derivative from the stored output (as the kernel)
    gp = g.double() * act_grad_from_output(y_k, act)
    gw, gb_ = gm64.clone().requires_grad_(True), bt64.clone().requires_grad_(True)
    xr = x64.clone().requires_grad_(True)
    if training:
        out = torch.cat([F.batch_norm(xg, None, None, gw, gb_, True, MOM, EPS) for xg in xr.chunk(groups)])
    else:
        out = F.batch_norm(xr, rm0.double(), rv0.double(), gw, gb_, False, MOM, EPS)
    out.backward(gp)
    gxref, dgref, dbref = xr.grad, gw.grad + dg0.double(), gb_.grad + db0.double()
    gps = xs(gp)
    if training:
        A = gps.mean((1, 3, 4), keepdim=True)
        Bm = (gps * xh).mean((1, 3, 4), keepdim=True)
    else:
        A = Bm = torch.zeros(1, dtype=torch.float64)
    xsc = xh.abs() + (xs(x64).abs() + mexp.abs()) * iexp
    gxtol = (2e-5 * gm.abs() * iexp * (gps.abs() + A.abs() + Bm.abs() * xsc)).reshape(B, C_, H, W)
    if training:
        gxtol = gxtol + gxref.abs() * texp.expand(-1, B // groups, -1, H, W).reshape(B, C_, H, W) * 2
    if prec == 'fp16':
        gxtol = gxtol + 2 ** -11 * gxref.abs() + 2 ** -24
    assert_within(download(gx1, C_), gxref, gxtol, 'gx')
    inner, rest = region(gx1)
    assert (inner[:, C_:] == 0).all(), 'padding lanes of gx not zero'
    assert (rest == SENT).all(), 'BWD_APPLY wrote outside the image'
    dgtol = (4e-6 * gps.abs() * xsc + gps.abs() * xh.abs() * texp).sum((0, 1, 3, 4)) + 2 ** -22 * (dg0.double().abs() + dgref.abs())
    dbtol = 4e-6 * gps.abs().sum((0, 1, 3, 4)) + 2 ** -22 * (db0.double().abs() + dbref.abs())
    assert_within(body(dgb1[0], C_), dgref, dgtol, 'dgamma')
    assert_within(body(dgb1[1], C_), dbref, dbtol, 'dbeta')


OFFSET_SHAPES = [  # discriminator BatchNorm layers on the (fake, real) pair of 16 x 128^2 crops: ppt 1 / 4 / 8
    ('fp16', 32, 128, 32, 32, 1), ('fp16', 32, 128, 64, 64, 4), ('fp32', 32, 128, 64, 64, 8)]


@pytest.mark.parametrize('case', OFFSET_SHAPES)
def test_batchnorm_statistics_of_offset_inputs(dev, case):
    """|mean| / std up to 30: the kernel forms var = E[x^2] - mean^2 from fp32 partial sums.  A CPU emulation of its
    summation order predicts a relative invstd error <= 1.2e-5 at these shapes; the bound is 5e-5."""
    E, L = _mods()
    prec, B, C_, H, W, ppt = case
    assert bn_ppt(B, C_, H, W, E._dt(prec)[2])[1] == ppt
    rng = np.random.default_rng(77 + ppt)
    sd = rng.uniform(0.5, 2.0, C_)
    mu = 30.0 * sd * np.where(np.arange(C_) % 2, 1.0, -1.0) * np.linspace(0.1, 1.0, C_)
    x = q(torch.from_numpy(mu[None, :, None, None] + sd[None, :, None, None] * rng.standard_normal((B, C_, H, W))).float(), prec)
    rig = BNRig(dev, prec, B, C_, H, W, 2, 1, L.ACT_NONE, x)
    sums = torch.zeros(4 * C_, dtype=torch.float64, device=dev)
    mean, inv = torch.zeros(2 * C_, device=dev), torch.zeros(2 * C_, device=dev)
    run(rig.op(L.BN_STATS, sums=sums), rig.op(L.BN_FINALIZE, sums=sums, mean=mean, invstd=inv))
    st = bn_stats_ref(x.double(), 2)
    iref = torch.cat([1 / (s['var'] + EPS).sqrt() for s in st])
    mref = torch.cat([s['m'] for s in st])
    rel = ((inv.cpu().double() - iref).abs() / iref).max().item()
    print('offset x30 %s B=%d C=%d %dx%d ppt=%d: max rel invstd err %.3e' % (prec, B, C_, H, W, ppt, rel))
    assert rel <= 5e-5
    assert ((mean.cpu().double() - mref).abs() <= 4e-6 * torch.cat([s['eabs'] for s in st])).all()


# ----------------------------------------------------------------------------------------------------------------
# max-pool and pixel shuffle
# ----------------------------------------------------------------------------------------------------------------

def pool_op(prec, mode, B, C_, H, W, x=None, y=None, g=None, gx=None, relu_mask=0):
    E, L = _mods()
    p = L.esr_pool()
    p.dtype, p.mode, p.B, p.C, p.H, p.W, p.relu_mask = E._dt(prec)[0], mode, B, C_, H, W, relu_mask
    for k, v in (('x', x), ('y', y), ('g', g), ('gx', gx)):
        if v is not None:
            setattr(p, k, v.view(0, v.C))
    return p


def pool_case(dev, prec, B, C_, Hi, Wi, x, g, relu_mask):
    """runs forward and backward on NCHW x [B, C, Hi, Wi] and g [B, C, Hi // 2, Wi // 2]; returns (y, its region,
    gx's region over 2H x 2W, the rest of gx's buffer)"""
    _, L = _mods()
    H, W = Hi // 2, Wi // 2
    xb, gb = g32(dev, prec, B, C_, Hi, Wi), g32(dev, prec, B, C_, H, W)
    upload(xb, x)
    upload(gb, g)
    yb, gxb = g32(dev, prec, B, C_, H, W, SENT), g32(dev, prec, B, C_, Hi, Wi, SENT)
    run((L.OP_POOL, 'pool', pool_op(prec, L.POOL_FWD, B, C_, H, W, x=xb, y=yb)),
        (L.OP_POOL, 'pool', pool_op(prec, L.POOL_BWD, B, C_, H, W, x=xb, g=gb, gx=gxb, relu_mask=relu_mask)))
    y_in, y_rest = region(yb)
    gx_in, gx_rest = region(gxb, 2 * H, 2 * W)
    return y_in, y_rest, gx_in, gx_rest, yb, gxb


def pool_ref(x, g, relu_mask):
    xr = x.double().clone().requires_grad_(True)
    y = F.max_pool2d(xr, 2, 2)
    y.backward(g.double())
    gx = xr.grad
    if relu_mask:
        gx = gx * (x.double() > 0)
    return y.detach(), gx


@pytest.mark.parametrize('relu_mask', [0, 1])
@pytest.mark.parametrize('size', [(8, 8), (9, 7), (2, 3), (5, 34), (33, 16)])
@pytest.mark.parametrize('C_', [3, 24, 64])
@pytest.mark.parametrize('prec', ['fp32', 'fp16'])
def test_maxpool_against_fp64(dev, prec, C_, size, relu_mask):
    """Inputs are integers in [-2, 2], so most windows hold ties: the gradient goes to the first maximum in
    row-major window order.  The backward writes exactly the 2H x 2W region of a gradient buffer of the full (odd)
    input size — every element, zeros and padding lanes included — and leaves the dropped row / column and the
    halo alone (the plan relies on both: the conv in front reads them as zeros)."""
    Hi, Wi = size
    B = 3
    rng = np.random.default_rng(seed_of(prec, C_, size, relu_mask))
    x = torch.from_numpy(rng.integers(-2, 3, (B, C_, Hi, Wi))).float()
    g = q(torch.from_numpy(rng.standard_normal((B, C_, Hi // 2, Wi // 2))).float(), prec)
    y_in, y_rest, gx_in, gx_rest, _, _ = pool_case(dev, prec, B, C_, Hi, Wi, x, g, relu_mask)
    yref, gxref = pool_ref(x, g, relu_mask)
    H, W = Hi // 2, Wi // 2
    assert torch.equal(y_in[:, :C_].double(), yref)
    assert (y_in[:, C_:] == 0).all() and (y_rest == SENT).all()
    assert torch.equal(gx_in[:, :C_].double(), gxref[:, :, :2 * H, :2 * W])
    assert (gx_in[:, C_:] == 0).all(), 'padding lanes of gx not written as zeros'
    assert (gx_rest == SENT).all(), 'pool backward wrote outside its 2H x 2W region'


@pytest.mark.parametrize('prec', ['fp32', 'fp16'])
def test_maxpool_nan_and_inf_windows(dev, prec):
    """NaN at each of the four window positions (alone, two of them, with +-inf next to it), +inf / -inf windows:
    the output and the gradient routing follow torch (a NaN wins; of two NaNs the later one takes the gradient)."""
    nan, inf = float('nan'), float('inf')
    wins = []
    for qpos in range(4):
        for other in (1.0, 3.0, inf, -inf, -2.0):
            w = [other, 0.5, -1.0, 2.0]
            w[qpos] = nan
            wins.append(w)
    wins += [[nan, nan, 1.0, 2.0], [1.0, nan, 2.0, nan], [nan, 1.0, 1.0, nan], [nan, nan, nan, nan],
             [inf, 1.0, inf, 2.0], [-inf, -inf, -inf, -inf], [-inf, 1.0, inf, nan], [1.0, 2.0, inf, -inf],
             [2.0, 2.0, 2.0, 2.0], [-1.0, -1.0, -3.0, -1.0]]
    C_, B = 24, 2
    n = len(wins)
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.integers(-2, 3, (B, C_, 2, 2 * n + 1))).float()
    for i, w in enumerate(wins):                      # window i of channel c, image b: rotated through the channels
        for b in range(B):
            c = (i * 5 + b * 7) % C_
            x[b, c, :, 2 * i:2 * i + 2] = torch.tensor(w).view(2, 2)
    g = q(torch.from_numpy(rng.uniform(0.5, 2.0, (B, C_, 1, n))).float(), prec)
    y_in, y_rest, gx_in, gx_rest, _, _ = pool_case(dev, prec, B, C_, 2, 2 * n + 1, x, g, 0)
    yref, gxref = pool_ref(x, g, 0)
    torch.testing.assert_close(y_in[:, :C_].double(), yref, rtol=0, atol=0, equal_nan=True)
    torch.testing.assert_close(gx_in[:, :C_].double(), gxref[:, :, :, :2 * n], rtol=0, atol=0)
    assert (gx_rest == SENT).all() and (y_rest == SENT).all()


def test_maxpool_of_a_map_too_small_to_pool_is_refused(dev):
    E, L = _mods()
    xb = g32(dev, 'fp32', 1, 8, 1, 3)
    yb = g32(dev, 'fp32', 1, 8, 1, 1)
    p = pool_op('fp32', L.POOL_FWD, 1, 8, 0, 1, x=xb, y=yb)       # 1 x 3 pools to 0 x 1
    assert L.lib().esr_maxpool2(C.byref(p), C.c_void_p(E.current_stream())) == -1   # ESR_ERR_INVALID
    assert b'invalid' in L.lib().esr_last_error()
    with pytest.raises(L.HipExtensionError):
        run((L.OP_POOL, 'pool', p))


@pytest.mark.parametrize('relu_mask', [0, 1])
@pytest.mark.parametrize('lo', [(7, 5), (4, 4), (1, 3), (9, 33)])
@pytest.mark.parametrize('ngrp', [1, 3])
@pytest.mark.parametrize('prec', ['fp32', 'fp16'])
def test_pixel_shuffle_against_fp64(dev, prec, ngrp, lo, relu_mask):
    """mode 2 = F.pixel_shuffle(x, 2), mode 3 = its float64 autograd adjoint (times ReLU'(x) with relu_mask), on
    C = CPG and 3 CPG high-resolution channels and odd low-resolution sizes; exact, and inside the image only."""
    E, L = _mods()
    cpg = E._dt(prec)[2]
    C_, (h, w), B = ngrp * cpg, lo, 2
    rng = np.random.default_rng(seed_of(prec, ngrp, lo, relu_mask))
    x = q(torch.from_numpy(rng.standard_normal((B, 4 * C_, h, w))).float(), prec)
    g = q(torch.from_numpy(rng.standard_normal((B, C_, 2 * h, 2 * w))).float(), prec)
    xb, gb = g32(dev, prec, B, 4 * C_, h, w), g32(dev, prec, B, C_, 2 * h, 2 * w)
    upload(xb, x)
    upload(gb, g)
    yb, gxb = g32(dev, prec, B, C_, 2 * h, 2 * w, SENT), g32(dev, prec, B, 4 * C_, h, w, SENT)
    fwd = pool_op(prec, L.POOL_SHUFFLE, B, C_, h, w, x=xb, y=yb)
    bwd = pool_op(prec, L.POOL_UNSHUFFLE, B, C_, h, w, x=xb, g=gb, gx=gxb, relu_mask=relu_mask)
    run((L.OP_POOL, 'pool', fwd), (L.OP_POOL, 'pool', bwd))
    xr = x.double().requires_grad_(True)
    y = F.pixel_shuffle(xr, 2)
    y.backward(g.double())
    gxref = xr.grad * (x.double() > 0) if relu_mask else xr.grad
    y_in, y_rest = region(yb)
    gx_in, gx_rest = region(gxb)
    assert torch.equal(y_in.double(), y.detach()) and (y_rest == SENT).all()
    assert torch.equal(gx_in.double(), gxref) and (gx_rest == SENT).all()


# ----------------------------------------------------------------------------------------------------------------
# Linear
# ----------------------------------------------------------------------------------------------------------------

def linear_run(dev, mode, B, I, O, act=0, in_act=0, **t):
    _, L = _mods()
    p = L.esr_linear()
    p.mode, p.B, p.I, p.O, p.act, p.in_act = mode, B, I, O, act, in_act
    for k, v in t.items():
        if v is not None:
            setattr(p, k, v.data_ptr())
    run((L.OP_LINEAR, 'linear', p))


def linear_check(dev, B, I, O, act, use_ysaved, in_act, seed):
    """forward y, bwdx gx and bwdw dw / db (onto non-zero buffers) against float64.  Bound per fp32 result:
    4e-6 * sum |terms| of that element, asserted to lie well below the element's median |term| (a dropped, doubled
    or misindexed term must fail)."""
    _, L = _mods()
    rng = np.random.default_rng(seed)
    # magnitudes in [0.5, 1.5], random signs: no term is negligible, so every element's median |term| is meaningful
    T = lambda *s: torch.from_numpy(rng.uniform(0.5, 1.5, s) * rng.choice([-1.0, 1.0], s)).float()  # noqa: E731
    x, w, bias, g, ys = T(B, I), T(O, I), T(O), T(B, O), T(B, O)
    dw0, db0 = T(O, I), T(O)
    d = {k: v.to(dev) for k, v in dict(x=x, w=w, b=bias, g=g, ysaved=ys).items()}
    y = torch.full((B, O), SENT, device=dev)
    gx = torch.full((B, I), SENT, device=dev)
    dw, db = dw0.to(dev), db0.to(dev)
    ysv = d['ysaved'] if use_ysaved else None
    linear_run(dev, 0, B, I, O, act, x=d['x'], w=d['w'], b=d['b'], y=y)
    linear_run(dev, 1, B, I, O, act, in_act, x=d['x'], w=d['w'], g=d['g'], ysaved=ysv, gx=gx)
    linear_run(dev, 2, B, I, O, act, x=d['x'], w=d['w'], g=d['g'], ysaved=ysv, dw=dw, db=db)
    x64, w64 = x.double(), w.double()

    def check(got, terms, extra, factor, what, post=lambda v: v):
        """got = post(factor * (sum over the last axis of terms + extra)); post is 1-Lipschitz"""
        ref = post(factor * (terms.sum(-1) + extra))
        bound = 4e-6 * (terms.abs().sum(-1) + extra.abs())
        med = terms.abs().median(-1).values
        assert (bound <= 0.25 * med).all(), '%s: the bound would not see a dropped term' % what
        return assert_within(got, ref, bound * factor.abs(), what)

    one = torch.ones((), dtype=torch.float64)
    # forward: terms x[b][i] w[o][i]; LeakyReLU is 1-Lipschitz, so the bound carries over
    terms = x64[:, None, :] * w64[None, :, :]
    worst = [check(y.cpu(), terms, bias.double().expand(B, O), one, 'y', post=lambda v: act64(v, act))]
    gp = g.double() * (act_grad_from_output(ys, act) if use_ysaved else 1.0)
    # bwdx: terms g'[b][o] w[o][i], then * in_act'(x[b][i])
    fac = act_grad_from_output(x, in_act) if in_act else one
    worst.append(check(gx.cpu(), (gp[:, :, None] * w64[None, :, :]).transpose(1, 2), torch.zeros(B, I, dtype=torch.float64), fac, 'gx'))
    # bwdw: terms g'[b][o] x[b][i] over b, onto dw0 / db0
    worst.append(check(dw.cpu(), (gp.t()[:, None, :] * x64.t()[None, :, :]), dw0.double(), one, 'dw'))
    worst.append(check(db.cpu(), gp.t(), db0.double(), one, 'db'))
    return max(worst)


LIN_OS, LIN_BS = (1, 7, 10, 23, 100), (1, 7, 8, 9, 17, 32)
LIN_CASES = [(O, B, I) for O in LIN_OS for B in LIN_BS for I in (1, 300)] + \
    [(O, B, I) for O, B in ((23, 17), (100, 32), (10, 9), (1, 8), (7, 1), (23, 9)) for I in (100, 8192)]


@pytest.mark.parametrize('case', LIN_CASES)
def test_linear_against_fp64(dev, case):
    """O = 23: two 10-row rounds of linear_bwdx_kernel + a 3-row tail; B = 9 / 17: 8-row rounds of
    linear_bwdw_kernel + a tail; O = 10 / B = 8, 32: main loop only; O in {1, 7} / B < 8: tail only."""
    _, L = _mods()
    O, B, I = case
    k = LIN_CASES.index(case)
    act, use_ys, in_act = (L.ACT_NONE, L.ACT_LRELU)[k % 2], (k // 2) % 2 == 0, (L.ACT_NONE, L.ACT_LRELU, L.ACT_RELU)[k % 3]
    linear_check(dev, B, I, O, act, use_ys, in_act, seed=k)


@pytest.mark.parametrize('in_act', [0, 1, 2])
@pytest.mark.parametrize('use_ys', [True, False])
@pytest.mark.parametrize('act', [0, 1])
def test_linear_activation_variants(dev, act, use_ys, in_act):
    linear_check(dev, 17, 300, 23, act, use_ys, in_act, seed=100 + 6 * act + 3 * use_ys + in_act)


# ----------------------------------------------------------------------------------------------------------------
# determinism
# ----------------------------------------------------------------------------------------------------------------

def test_kernels_are_deterministic(dev):
    """One representative case per kernel, run twice: bit-identical.  Exception: the BatchNorm sums are fp64 atomics
    (order of arrival), so they are only required to agree closely; every pass downstream of a given sums buffer must
    be bit-identical."""
    E, L = _mods()
    # BatchNorm
    prec, B, C_, H, W, groups = 'fp16', 32, 24, 60, 60, 2
    x, gamma, beta, rm0, rv0, g, _, _ = bn_inputs(9, prec, B, C_, H, W)
    rig = BNRig(dev, prec, B, C_, H, W, groups, 1, L.ACT_LRELU, x)
    gbuf = g32(dev, prec, B, C_, H, W)
    upload(gbuf, g)
    gam, bet = gamma.to(dev), beta.to(dev)
    sums = [torch.zeros(2 * groups * C_, dtype=torch.float64, device=dev) for _ in range(2)]
    for s in sums:
        run(rig.op(L.BN_STATS, sums=s))
    torch.testing.assert_close(sums[1], sums[0], rtol=1e-12, atol=0)
    outs = []
    for _ in range(2):
        o = dict(mean=torch.zeros(groups * C_, device=dev), invstd=torch.zeros(groups * C_, device=dev),
                 running_mean=rm0.to(dev), running_var=rv0.to(dev), y=g32(dev, prec, B, C_, H, W),
                 gx=g32(dev, prec, B, C_, H, W), sums_b=torch.zeros(2 * groups * C_, dtype=torch.float64, device=dev),
                 dgamma=torch.zeros(C_, device=dev), dbeta=torch.zeros(C_, device=dev))
        run(rig.op(L.BN_FIN_APPLY, sums=sums[0], gamma=gam, beta=bet, mean=o['mean'], invstd=o['invstd'], y=o['y'],
                   running_mean=o['running_mean'], running_var=o['running_var']))
        bc = dict(y=o['y'], g=gbuf, mean=o['mean'], invstd=o['invstd'], gamma=gam, beta=bet)
        run(rig.op(L.BN_BWD_REDUCE, sums=o['sums_b'], **bc))
        outs.append(o)
    torch.testing.assert_close(outs[1]['sums_b'], outs[0]['sums_b'], rtol=1e-12, atol=1e-300)
    for o in outs:   # the apply pass from ONE backward sums buffer
        run(rig.op(L.BN_BWD_APPLY, sums=outs[0]['sums_b'], y=o['y'], g=gbuf, gx=o['gx'], mean=o['mean'],
                   invstd=o['invstd'], gamma=gam, beta=bet, dgamma=o['dgamma'], dbeta=o['dbeta']))
    for k in ('mean', 'invstd', 'running_mean', 'running_var', 'dgamma', 'dbeta'):
        assert torch.equal(outs[0][k], outs[1][k]), k
    assert torch.equal(outs[0]['y'].t, outs[1]['y'].t) and torch.equal(outs[0]['gx'].t, outs[1]['gx'].t)
    # max-pool / pixel shuffle
    x = torch.from_numpy(np.random.default_rng(3).integers(-2, 3, (4, 24, 9, 7))).float()
    g = torch.from_numpy(np.random.default_rng(4).standard_normal((4, 24, 4, 3))).float()
    a, b = pool_case(dev, 'fp16', 4, 24, 9, 7, x, g, 1), pool_case(dev, 'fp16', 4, 24, 9, 7, x, g, 1)
    assert torch.equal(a[4].t, b[4].t) and torch.equal(a[5].t, b[5].t)
    # linear
    rng = np.random.default_rng(6)
    B, I, O = 17, 300, 23
    tt = {k: torch.from_numpy(rng.standard_normal(s)).float().to(dev)
          for k, s in dict(x=(B, I), w=(O, I), b=(O,), g=(B, O), ysaved=(B, O)).items()}
    res = []
    for _ in range(2):
        y, gx = torch.zeros(B, O, device=dev), torch.zeros(B, I, device=dev)
        dw, db = torch.ones(O, I, device=dev), torch.ones(O, device=dev)
        linear_run(dev, 0, B, I, O, L.ACT_LRELU, x=tt['x'], w=tt['w'], b=tt['b'], y=y)
        linear_run(dev, 1, B, I, O, L.ACT_LRELU, L.ACT_LRELU, x=tt['x'], w=tt['w'], g=tt['g'], ysaved=tt['ysaved'], gx=gx)
        linear_run(dev, 2, B, I, O, L.ACT_LRELU, x=tt['x'], w=tt['w'], g=tt['g'], ysaved=tt['ysaved'], dw=dw, db=db)
        res.append((y, gx, dw, db))
    for u, v in zip(*res):
        assert torch.equal(u, v)
