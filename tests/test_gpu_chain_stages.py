"""Every stage the fused dense-block chains store (csrc/rdb_chain_kernel.h: esr_rdb_forward modes 0 and 1,
esr_rdb_backward) against a float64 reference of THAT stage alone, computed on the CPU from the values the kernel stored
for the stages before it (tests/chain_stage_refs.py): forward x1..x4 and the block output, backward g_a4, g_a3, the raw
g_x2, g_a2, g_a1, the next g_t / dL/dx and the skip gradient out_a — every pixel of every image of every block.  A mask
flip or a rounding in one stage therefore cannot reach the next stage's comparison, and each stage is held to the bound of
one stored conv result: error relative to the reference's largest magnitude <= 1.5e-3 in fp16 (two fp16 roundings,
2 x 2^-11, plus fp32 accumulation; TOL_DG of test_gpu_conv_backward.py), 4e-6 in fp32.

Weights: the master rounded once as the packed operands hold it (recomputed, not read back).  Masks: m_k = (a_k > 0) of
the float64 pre-activation from stored inputs; elements with |a_k| < 1e-4 max|a_k| are left out of g_ak (the kernel's
fp32 sum may land on the other side), asserted to be at most 0.5 % of a stage.  Noise: z from ops.philox_normal for the
step's seed.  The training plans are driven through engine.TrainBuilder with build_rrdbnet_train_plan's calls, so that
S, Qs, XF, GX, gA stay reachable; after every launch the chain workspaces' timeout word and the library's abort word
are zero, and afterwards the zero ring and the rows / columns past the image of every such buffer hold exactly 0.

Worst error / scale per stage measured on an MI355X (each test prints its own with -s); fp16 sits at one to two
roundings of the stored result (2^-12 = 2.4e-4), and the three tile heights of case b agree in every digit:
  case a  forward  x1 1.88e-4  x2 2.81e-4  x3 2.40e-4  x4 2.94e-4  y 2.53e-4
          backward g_a4 2.46e-4  g_a3 2.45e-4  g_x2 2.78e-4  g_a2 3.83e-4  g_a1 4.31e-4  x_out 2.52e-4
  case b  forward  x1 2.58e-4  x2 3.58e-4  x3 2.78e-4  x4 3.08e-4  y 3.43e-4
          backward g_a4 3.46e-4  g_a3 3.28e-4  g_x2 4.31e-4  g_a2 4.55e-4  g_a1 3.01e-4  x_out 3.72e-4
  case c  forward  x1 3.85e-4  x2 3.89e-4  x3 3.89e-4  x4 3.87e-4  y 3.88e-4
          backward g_a4 4.55e-4  g_a3 4.14e-4  g_x2 4.68e-4  g_a2 3.08e-4  g_a1 3.63e-4  x_out 3.53e-4  out_a 2.71e-4
  case d  forward  x1 2.75e-4  x2 3.90e-4  x3 2.76e-4  x4 3.49e-4  y 4.01e-4
          backward g_a4 3.66e-4  g_a3 3.63e-4  g_x2 3.63e-4  g_a2 2.74e-4  g_a1 3.12e-4  x_out 3.86e-4
  mode 0  fp16     x1 2.34e-4  x2 3.29e-4  x3 2.69e-4  x4 3.30e-4  y 3.90e-4
          fp32     x1 7.39e-7  x2 8.67e-7  x3 1.38e-6  x4 8.93e-7  y 2.62e-7"""
import pytest
import torch

from tests import chain_stage_refs as R
from tests.test_gpu_conv_backward import region

pytestmark = pytest.mark.gpu

TOL = {'fp16': 1.5e-3, 'fp32': 4e-6}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _mods():
    from esrganplus_amd import engine as E, _lib as L, functional as Fn, ops
    return E, L, Fn, ops


def inner(buf, c0=0, n=None):
    """channels [c0, c0 + n) of a G32 buffer's image pixels as float64 NCHW (the stored values, exactly)"""
    t = region(buf)[0]
    return t[:, c0:(c0 + n) if n else None].double()


def assert_ring_is_zero(bufs):
    for name, buf in bufs:
        rest = region(buf)[1]
        assert (rest == 0).all(), '%s: %d non-zero elements outside the image' % (name, int((rest != 0).sum()))


def assert_chains_clean(*ws):
    _, L, _, _ = _mods()
    torch.cuda.synchronize()
    for w in ws:
        assert int(w[1].item()) == 0, 'a bounded spin of the chain timed out'
    assert L.lib().esr_rdb_check_abort() == 0


class Worst:
    """worst err / scale per stage over the blocks of a case"""

    def __init__(self, what, tol):
        self.what, self.tol, self.e, self.bad = what, tol, {}, []

    def check(self, stage, where, got, ref, unsure=None):
        keep = None
        if unsure is not None:
            share = unsure.double().mean().item()
            assert share <= R.MASK_SHARE, '%s %s %s: %.2e of the elements left out' % (self.what, where, stage, share)
            keep = ~unsure
        e = R.rel_err(got, ref, keep)
        self.e[stage] = max(self.e.get(stage, 0.0), e)
        if not e <= self.tol:
            d = (got.double() - ref.double()).abs() * (keep if keep is not None else 1)
            at = tuple(int(v) for v in (d == d.max()).nonzero()[0])
            self.bad.append('%s %s: err/scale %.3e at (b, c, y, x) = %s' % (where, stage, e, at))

    def done(self):
        print('%s: worst err/scale  %s' % (self.what, '  '.join('%s %.2e' % kv for kv in self.e.items())))
        assert not self.bad, '\n'.join(self.bad)


_REFS = {}


def cached(key, inputs, fn):
    """fn() once per (key, stored inputs): runs whose stored inputs agree bit for bit share a reference"""
    for ins, out in _REFS.setdefault(key, []):
        if len(ins) == len(inputs) and all((a is None and b is None) or (a is not None and b is not None and torch.equal(a, b))
                                           for a, b in zip(ins, inputs)):
            return out
    out = fn()
    _REFS[key].append((inputs, out))
    return out


# ----------------------------------------------------------------------------------------------------------------
# training chains (modes 1 and 2)
# ----------------------------------------------------------------------------------------------------------------

def build(mod, kind, in_nc, out_nc, B, H, W, dev, noise):
    """engine.build_rrdbnet_train_plan's calls, in its order; the builder is kept"""
    E, _, _, _ = _mods()
    st = E.current_stream()
    wp = mod._weights(dev)
    dp = mod._dgrad_weights(dev)
    dp.ensure(st)
    nb = mod.nb if kind == 'net' else 1
    bld = E.TrainBuilder(wp, dp, nb, B, H, W, mod.precision, dev, noise, mod.variant, False, kind, False,
                         mod.upscale if kind == 'net' else 4)
    bld.forward_head(in_nc)
    assert bld.chained, 'the fused training chains were not chosen'
    bld.forward_blocks_chain()
    bld.forward_exit(out_nc)
    bld.grad_store(mod)
    bld.backward_buffers(out_nc)
    if bld.block:
        bld.backward_entry_block()
    else:
        bld.backward_tail(out_nc)
    bld.backward_blocks()
    bld.backward_exit(in_nc)
    bld.tp.packs = (wp, dp)
    assert bld.tp.fwd.chain_ops and bld.tp.bwd_chain_ops
    return bld


def step(bld, x, gy, noise):
    """one training forward + backward of the plan; returns the step's Philox seed"""
    E, _, Fn, _ = _mods()
    tp, st = bld.tp, E.current_stream()
    torch.manual_seed(R.TORCH_SEED)
    seed = Fn._draw_seed() if noise else 0
    Fn._train_forward(tp, x, st, seed, None)
    assert_chains_clean(tp.fwd.chain_ws)
    Fn._train_backward(tp, gy, st, noise, False, seed, bld.block)
    assert_chains_clean(tp.fwd.chain_ws, tp.bwd_chain_ws)
    return seed


def check_train_plan(what, bld, sd, prefix_of, noise, seed, dev):
    """every stored stage of every block of the plan against its stage-local reference"""
    _, _, _, ops = _mods()
    nb, nj, B, H, W = bld.nb, bld.nj, bld.B, bld.H, bld.W
    per = 4 if bld.variant == 'test_image' else 3
    shape = (B, 64, H, W)
    zc = {}

    def z(layer):
        if not noise or layer is None:
            return None
        if layer not in zc:
            zc[layer] = ops.philox_normal(shape, seed, layer, dev).cpu()
        return zc[layer]
    l_rdb = lambda i, j: per * i + j
    l_rrdb = lambda i: (per * i + 3) if (per == 4 and bld.kind != 'rdb') else None
    wf, wb = Worst(what + ' forward', TOL['fp16']), Worst(what + ' backward', TOL['fp16'])
    for i in range(nb):
        for j in range(nj):
            where, p = 'block (%d, %d)' % (i, j), prefix_of(i, j)
            S = inner(bld.S[i][j])
            x, x1, x2, x3, x4 = S[:, :64], S[:, 64:96], S[:, 96:128], S[:, 128:160], S[:, 160:192]
            y = inner(bld.x_out(i, j), 0, 64)
            tail = bld.rrdb_x(i, j) is not None
            assert tail == (j == 2 and bld.kind != 'rdb')
            res2 = inner(bld.S[i][0], 0, 64) if tail else None
            z1, z2 = z(l_rdb(i, j)), z(l_rrdb(i)) if tail else None
            fs = cached((what, 'f', i, j), (x, x1, x2, x3, x4, res2, z1, z2),
                        lambda: R.forward_stages(R.forward_weights(sd, p, 'fp16'), x, x1, x2, x3, x4, z1, res2, z2))
            for name, got in (('x1', x1), ('x2', x2), ('x3', x3), ('x4', x4), ('y', y)):
                wf.check(name, where, got, fs[name])
            m, unsure = R.masks_of(fs)
            # backward
            Q = inner(bld.Qs[bld.bwd_index(i, j)])
            g_t, g_a4, g_a3, g_a2, g_a1, g_x2 = Q[:, :64], Q[:, 64:96], Q[:, 96:128], Q[:, 128:160], Q[:, 160:192], Q[:, 192:224]
            ex = bld.block_exit(i, j)
            if j > 0:
                want = (False, False, l_rdb(i, j - 1), None)
            elif bld.kind == 'rdb':
                want = (False, False, None, None)
            elif bld.block or i == 0:
                want = (True, False, None, None)
            else:
                want = (True, True, l_rdb(i - 1, 2), l_rrdb(i - 1))
            assert (ex.skip_in is not None, ex.skip_out is not None) == want[:2], where
            skip = inner(ex.skip_in, 0, 64) if want[0] else None
            zb1, zb2 = z(want[2]), z(want[3])
            bs = cached((what, 'b', i, j), (g_t, g_a4, g_a3, g_x2, g_a2, g_a1, skip, zb1, zb2, x, x1, x2, x3),
                        lambda: R.backward_stages(R.backward_weights(sd, p), g_t, m, g_a4, g_a3, g_x2, g_a2, g_a1,
                                                  skip, zb1, zb2, want[1]))
            for name, got, k in (('g_a4', g_a4, 4), ('g_a3', g_a3, 3), ('g_x2', g_x2, None), ('g_a2', g_a2, 2), ('g_a1', g_a1, 1)):
                wb.check(name, where, got, bs[name], unsure[k] if k else None)
            wb.check('x_out', where, inner(ex.dst, 0, 64), bs['x_out'])
            if want[1]:
                wb.check('out_a', where, inner(ex.skip_out, 0, 64), bs['out_a'])
    bufs = [('S[%d][%d]' % (i, j), bld.S[i][j]) for i in range(nb) for j in range(nj)]
    bufs += [('Q[%d]' % n, q_) for n, q_ in enumerate(bld.Qs)] + [('XF', bld.XF), ('gA[0]', bld.gA[0]), ('gA[1]', bld.gA[1])]
    bufs += [('GX', bld.GX)] if bld.GX is not None else [('GF', bld.GF)]
    assert_ring_is_zero(bufs)
    wf.done()
    wb.done()


BLOCK_RUNS = [('a', None), ('b', None), ('b', '4'), ('b', '1'), ('d', None)]


@pytest.mark.parametrize('case,rows', BLOCK_RUNS, ids=['%s-rows%s' % (c, r or 'auto') for c, r in BLOCK_RUNS])
def test_block_training_chains_stage_by_stage(dev, monkeypatch, case, rows):
    """Stand-alone dense block / RRDB (both variants), fp16.  Case b: (2, 64, 33, 70) is 3 x 3 tiles of 16 x 32 with a
    one-row and a six-column ragged edge (ESR_RDB_ROWS = 4), 9 x 3 four-row tiles with ESR_RDB_ROWS = 1; the height the
    library picks by itself runs too."""
    monkeypatch.setenv('ESR_RDB_TRAIN_CHAIN', '1')
    if rows is None:
        monkeypatch.delenv('ESR_RDB_ROWS', raising=False)
    else:
        monkeypatch.setenv('ESR_RDB_ROWS', rows)
    kind, shape, train, _, xseed, gseed = R.BLOCK_CASES[case]
    mod = R.block_module(kind).to(dev).train(train).set_precision('fp16')
    sd = {k: v.detach().cpu() for k, v in mod.state_dict().items()}
    has_noise = mod.noise is not None if kind == 'rdb' else True
    noise = bool(train and has_noise)
    B, _, H, W = shape
    bld = build(mod, 'rdb' if kind == 'rdb' else 'rrdb', 64, 64, B, H, W, dev, noise)
    seed = step(bld, R.randn(shape, xseed).to(dev), R.randn(shape, gseed).to(dev), noise)
    pre = R.block_prefixes(kind)
    check_train_plan('case %s rows %s' % (case, rows or 'auto'), bld, sd, lambda i, j: pre[j], noise, seed, dev)


def test_trunk_training_chains_stage_by_stage(dev, monkeypatch):
    """RRDB_Net, nb = 2: the trunk's blocks — the only plans whose backward has a block with out_a (the RDB1 of RRDB 1
    leaves the skip gradient of RRDB 0 in gA and 0.2 x it, through both noise layers, as RDB3's g_t)."""
    from esrganplus_amd import architecture as arch, synth
    monkeypatch.setenv('ESR_RDB_TRAIN_CHAIN', '1')
    monkeypatch.delenv('ESR_RDB_ROWS', raising=False)
    c = R.NET_CASE
    sd = synth.rrdbnet_state_dict(nb=c['nb'], seed=c['wseed'], gain=c['gain'])
    net = getattr(arch, c['cls'])(3, 3, 64, c['nb']).to(dev).train().set_precision('fp16')
    net.load_state_dict(sd, strict=True)
    B, _, H, W = c['shape']
    bld = build(net, 'net', 3, 3, B, H, W, dev, True)
    assert any(bld.block_exit(i, 0).skip_out is not None for i in range(c['nb']))
    x = synth.image_batch(c['xseed'], *c['shape'], name='stages.x').to(dev)
    gy = R.randn((B, 3, 4 * H, 4 * W), c['gseed']).to(dev)
    seed = step(bld, x, gy, True)
    check_train_plan('case c', bld, sd, lambda i, j: 'model.1.sub.%d.RDB%d' % (i, j + 1), True, seed, dev)


# ----------------------------------------------------------------------------------------------------------------
# inference chain (mode 0), one block with its dense slices saved
# ----------------------------------------------------------------------------------------------------------------

INFER_RUNS = [('fp16', None), ('fp16', '4'), ('fp32', None)]


@pytest.mark.parametrize('prec,rows', INFER_RUNS, ids=['%s-rows%s' % (p, r or 'auto') for p, r in INFER_RUNS])
def test_inference_chain_stage_by_stage(dev, monkeypatch, prec, rows):
    """Builder.rdb_chain over ONE block with ESR_RDB_FULL_OUT and save_dense = 1 at (2, 64, 33, 70): x1..x4 and y.
    (Chains of several mode-0 blocks keep their intermediates in the LDS: they stay with the end-to-end tests.)"""
    E, L, _, _ = _mods()
    if rows is None:
        monkeypatch.delenv('ESR_RDB_ROWS', raising=False)
    else:
        monkeypatch.setenv('ESR_RDB_ROWS', rows)
    c = R.INFER_CASE
    B, _, H, W = c['shape']
    mod = R.block_module('rdb').to(dev).eval().set_precision(prec)
    sd = {k: v.detach().cpu() for k, v in mod.state_dict().items()}
    st = E.current_stream()
    wp = mod._weights(dev)
    bld = E.Builder(wp, B, H, W, prec, dev, False, mod.variant, 'rdb', 1)
    assert E.rdb_chain_ok(B, H, W, False, False)
    P = bld.plan
    xa, xb = bld.buf(64), bld.buf(64)
    P.in_op = bld.import_nchw(xa, 64)
    k = bld.rdb_chain([('rdb', xa, xb, None, None, None)])
    dense = [b for b in bld.bufs if isinstance(b, E.G32) and b.C == 128]
    assert len(dense) == 1
    ch = P.ops.ops[k].u.rdb_chain
    ch.save_dense = 1
    P.ops._arr = None
    assert ch.n_blocks == 1 and ch.mode == 0
    P.out_op = bld.export_nchw(xb, 64)
    P.out_shape = (B, 64, H, W)
    out = torch.empty(P.out_shape, dtype=torch.float32, device=dev)
    P.run(R.randn(c['shape'], c['xseed']).to(dev), out, st)
    assert_chains_clean(P.chain_ws)
    x, D, y = inner(xa, 0, 64), inner(dense[0]), inner(xb, 0, 64)
    got = {'x1': D[:, :32], 'x2': D[:, 32:64], 'x3': D[:, 64:96], 'x4': D[:, 96:128], 'y': y}
    assert torch.equal(y.float(), out.cpu())
    fs = cached(('infer', prec), (x, got['x1'], got['x2'], got['x3'], got['x4']),
                lambda: R.forward_stages(R.forward_weights(sd, '', prec), x, got['x1'], got['x2'], got['x3'], got['x4']))
    _, unsure = R.masks_of(fs)
    assert max(u.double().mean().item() for u in unsure.values()) <= R.MASK_SHARE
    w = Worst('mode 0 %s rows %s' % (prec, rows or 'auto'), TOL[prec])
    for name in ('x1', 'x2', 'x3', 'x4', 'y'):
        w.check(name, 'block 0', got[name], fs[name])
    assert_ring_is_zero([('x_in', xa), ('dense', dense[0]), ('x_out', xb)])
    w.done()
