"""Kernels that take an esr_g32, launched on views whose bytes lie beyond 2^31 and 2^32 from the view's pointer
(tests/far_views.py: the arena, the three families, relocate / gather / scan), and the refusals of the views DESIGN.md
"Address widths" puts beyond a kernel's limit.

A launched case builds its op on compact engine.G32 buffers exactly as the op's own test file does, runs it, checks it
against float64 with that file's reference and tolerance, then runs the SAME op struct rewritten to far views of every
family the case fits and requires: every relocated buffer — inputs, outputs, sentinels — bit-identical to the compact
buffer after the compact run; the compact buffers untouched by the far run; every arena byte outside the windows still
0x3C.  Dispatch depends on B, H, W and channels, never on strides, so both runs take the branch the case pins
(test_far_views_host.py pins them without a GPU and proves the arena property of every case).  Sums formed with
floating-point atomics (the BatchNorm statistics) are compared within their own test's tolerance instead.

Launched: the forward conv on every dispatch branch and operand (a), the chains in modes 0, 1 and 2 (b), the dense-block
weight gradients (c), the per-conv weight gradients fp32 / fp16 / multi (d), BatchNorm, pooling and the shuffles (e), the
layout kernels (f) and the six image ends (g) — each on every family its audit row allows.  The band form of mode 0 runs with
its band-local buffers (the block outputs in between and the dense scratch, one entry per band) on the far batch; the
band views of the tall image buffers carry strides of their own (batch_stride = band_rows rows) and stay compact, and
four tall planes past 2^31 are the chain's limit — a refusal.

A refusal launches nothing: the call returns ESR_ERR_INVALID / ESR_ERR_UNSUPPORTED, esr_last_error() names the limit and
the arena is untouched."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import far_views as FV
from tests.test_gpu_conv_backward import (SENT, SLOPE, TOL_DG, WgradRig, _mods, cdiv, dev, dgrad_ref, g32, q,  # noqa: F401
                                          region, rel_err, rnd, run, ts2_branch, upload, wgrad16_grid)
from tests.test_gpu_conv_forward import Fwd, TOL, fwd_branch, in_map

ARENA_BYTES = FV.PTR_OFF + 3 * FV.FAR + FV.SPAN + FV.TAIL          # 8.63 GiB: four far groups and their windows
ALL, BG, GP, B_, G_ = ('batch', 'group', 'plane'), ('batch', 'group'), ('group', 'plane'), ('batch',), ('group',)
CPG = {'fp16': 16, 'fp32': 8}


@pytest.fixture(scope='module')
def arena(dev):
    assert ARENA_BYTES <= FV.ARENA_MAX
    a = FV.Arena(dev, ARENA_BYTES)
    yield a
    del a.t
    del a
    torch.cuda.empty_cache()


def far_runs(arena, op, bufs, pre, families, launch, table=None, expect=None, keep=()):
    """for every family: relocate (windows = the buffers' contents BEFORE the compact run), launch(relocated), and hand
    (family, Relocated) to the caller's checks; afterwards the arena scan, and the windows are blanked again"""
    for fam in families:
        rel = FV.relocate(op, bufs, fam, arena, contents=pre, table=table, keep=keep)
        if expect is not None:
            got = [(fb.B, fb.ng, fb.Hp, fb.Wp) for fb in rel.used]
            assert got == expect, (fam, got, expect)
        try:
            launch(rel)
            yield fam, rel
            assert arena.scan(rel.used), '%s family: a byte outside the windows changed' % fam
            arena.clear(rel.used)
        except BaseException:
            arena.t.fill_(FV.FILL)
            raise


def same_as_compact(arena, rel, post, what):
    for i, fb in enumerate(rel.fbs):
        if fb is not None:
            assert torch.equal(arena.gather(fb), FV.Arena._bytes(post[i], fb.ng)), '%s: buffer %d differs' % (what, i)


# ----------------------------------------------------------------------------------------------------------------
# a. esr_conv_forward
# ----------------------------------------------------------------------------------------------------------------

def lre(**kw):
    return dict(act='lrelu', **kw)


# name, prec, B, cin, cout, kind, H, W (the OUTPUT map), debug_flags, spec, branch, families, extra
# Channel counts keep every view within what a family can hold: 4 groups (group), 2 groups (plane).  The batch family
# needs B <= 3, so the 8-row tiles (a grid of more than 128 workgroups) run on the group and plane families only.
CONV_CASES = [
    ('f16_r1_pipe', 'fp16', 3, 32, 24, '3x3', 13, 40, 0, lre(), (1, 'pipe', 1), ALL, None),
    ('f16_r1_plain', 'fp16', 3, 64, 64, '3x3', 13, 40, 0, dict(act='relu'), (1, 'plain', 1), BG, None),
    ('f16_r2_pipe', 'fp16', 40, 32, 16, '3x3', 20, 40, 0, lre(), (2, 'pipe', 1), GP, None),
    ('f16_r2_plain', 'fp16', 20, 48, 64, '3x3', 20, 40, 0, dict(act='relu'), (2, 'plain', 1), G_, None),
    ('f16_r4_pipe', 'fp16', 3, 24, 32, '3x3', 20, 40, 256, lre(), (4, 'pipe', 1), ALL, None),
    ('f16_r4_plain', 'fp16', 3, 24, 32, '3x3', 20, 40, 256 | 64, dict(act='none'), (4, 'plain', 1), ALL, None),
    ('f16_r4_two', 'fp16', 3, 64, 64, '3x3', 18, 33, 256, lre(), (4, 'plain', 1), BG, None),
    ('f16_f1x1_r1', 'fp16', 3, 64, 32, '3x3', 13, 40, 0, lre(w1x1=64, aux=32), (1, '1x1', 1), BG, None),
    ('f16_f1x1_r2', 'fp16', 40, 32, 32, '3x3', 20, 40, 0, lre(w1x1=32), (2, '1x1', 1), GP, None),
    ('f16_f1x1_r4', 'fp16', 3, 32, 32, '3x3', 13, 40, 256, lre(w1x1=32), (4, '1x1', 1), ALL, None),
    ('f16_1x1_one', 'fp16', 3, 24, 32, '1x1', 11, 40, 0, lre(), 'one', ALL, None),
    ('f16_1x1_two', 'fp16', 3, 48, 64, '1x1', 11, 40, 0, dict(act='none'), 'two', BG, None),
    ('f16_ups_one', 'fp16', 3, 24, 32, 'ups', 26, 40, 0, lre(), 'one', ALL, None),
    ('f16_ups_two', 'fp16', 3, 32, 64, 'ups', 18, 70, 0, lre(), 'two', BG, None),
    ('f16_sub_one', 'fp16', 3, 24, 32, 'sub', 26, 70, 0, lre(), 'one', ALL, None),
    ('f16_sub_two', 'fp16', 3, 32, 64, 'sub', 18, 40, 0, lre(), 'two', BG, None),
    ('f16_s2_wide', 'fp16', 3, 24, 32, 's2', 9, 34, 0, lre(), 'wide', ALL, None),
    ('f16_s2_plain', 'fp16', 3, 32, 64, 's2', 9, 20, 0, lre(), 'plain', BG, None),
    ('f32_pipe', 'fp32', 3, 16, 16, '3x3', 13, 40, 0, lre(), (4, 'pipe', 1), ALL, None),
    ('f32_plain', 'fp32', 3, 16, 16, '3x3', 13, 40, 64, dict(act='none'), (4, 'plain', 1), ALL, None),
    ('f32_two', 'fp32', 3, 24, 64, '3x3', 18, 33, 0, lre(), (4, 'plain', 1), B_, None),
    ('f32_f1x1', 'fp32', 3, 32, 32, '3x3', 13, 40, 0, lre(w1x1=32), (4, '1x1', 1), BG, None),
    ('f32_1x1_one', 'fp32', 3, 16, 16, '1x1', 11, 40, 0, dict(act='relu'), 'one', ALL, None),
    ('f32_1x1_two', 'fp32', 3, 24, 64, '1x1', 11, 40, 0, lre(), 'two', B_, None),
    ('f32_ups_one', 'fp32', 3, 16, 16, 'ups', 26, 40, 0, dict(act='relu'), 'one', ALL, None),
    ('f32_ups_two', 'fp32', 3, 24, 64, 'ups', 18, 70, 0, lre(), 'two', B_, None),
    ('f32_sub_one', 'fp32', 3, 16, 16, 'sub', 26, 70, 0, lre(), 'one', ALL, None),
    ('f32_sub_two', 'fp32', 3, 24, 64, 'sub', 18, 40, 0, dict(act='relu'), 'two', B_, None),
    ('f32_s2_wide', 'fp32', 3, 16, 16, 's2', 9, 34, 0, dict(act='relu'), 'wide', ALL, None),
    ('f32_s2_plain', 'fp32', 3, 24, 64, 's2', 9, 20, 0, lre(), 'plain', B_, None),
    # operands: res1 + res2, aux_out + z1, and mask + out2 + out3 (the BWD instantiation of the epilogue)
    ('f16_res12', 'fp16', 3, 32, 32, '3x3', 13, 40, 0, lre(res1=(0.2, None), res2=(0.7, None)), (1, 'pipe', 1), ALL, None),
    ('f16_aux_z1', 'fp16', 3, 32, 32, '3x3', 13, 40, 0, lre(aux=0, z1=None), (1, 'pipe', 1), ALL, None),
    ('f16_bwd3', 'fp16', 3, 32, 32, '3x3', 13, 40, 0, lre(res1=(0.2, None)), (1, 'pipe', 1), ALL, 'bwd3'),
    ('f32_res12_aux_z1', 'fp32', 3, 16, 16, '3x3', 13, 40, 0, lre(res1=(0.2, None), res2=(0.7, None), aux=0, z1=None),
     (4, 'pipe', 1), ALL, None),
    ('f32_bwd3', 'fp32', 3, 16, 16, '3x3', 13, 40, 0, lre(res1=(0.2, None)), (4, 'pipe', 1), ALL, 'bwd3'),
    # the PACK branch: several small images per tile, K split over workgroups, BatchNorm statistics in the finishing
    # pass.  Its staging map spans the images of a tile AND the plane in 32 bits: the far batch and the near-limit plane
    # (two more images on top of a plane 896 bytes below 2^31) are refusals (below)
    ('f16_pack', 'fp16', 3, 64, 64, 's2', 8, 8, 0, lre(), 'plain', G_, 'ksplit'),
    ('f16_pack_c32', 'fp16', 3, 32, 32, 's2', 8, 8, 0, lre(), 'plain', G_, 'ksplit'),
]


def conv_branch(c):
    name, prec, B, cin, cout, kind, H, W, flags, spec = c[:10]
    return fwd_branch(prec, B, H, W, cout, kind, flags, spec.get('w1x1', 0))


def conv_shapes(c):
    """(B, groups a view reaches, Hp, Wp) of every buffer of a conv case, in fwd_bufs' order — without a GPU"""
    name, prec, B, cin, cout, kind, H, W, flags, spec, _, _, extra = c
    cpg = CPG[prec]
    Hi, Wi = in_map(kind, H, W)
    out = [(B, cdiv(cin, cpg)) + FV.g32_dims(Hi, Wi)]
    co = (B, cdiv(cout, cpg)) + FV.g32_dims(H, W)
    out += [co for k in ('res1', 'z1', 'z2', 'res2') if k in spec]
    if spec.get('aux') is not None:
        out.append((B, (spec['aux'] + cout + cpg - 1) // cpg) + FV.g32_dims(H, W))
    out.append(co)
    if extra == 'bwd3':
        out += [co, co, co]
    return out


def fwd_bufs(f):
    bufs = [f.xin] + list(f.bufs.values())
    for _, b, *_ in f.checks:
        if all(b is not o for o in bufs):
            bufs.append(b)
    return bufs


def add_bwd3(f, dev):
    """mask + out2 + out3 on a forward rig: out2 = v * act'(mask) from cout block 0, out3 = v * gamma (no noise)"""
    _, L = _mods()
    B, cout, H, W, prec = f.B, f.cout, f.H, f.W, f.prec
    m = rnd((B, cout, H, W), 'far.mask', f.name)
    m = torch.where(m.abs() < 0.3, torch.zeros_like(m), m)               # exact zeros: act' of the negative side
    mk = g32(dev, prec, B, cout, H, W)
    upload(mk, m)
    f.bufs['mask'] = mk
    out2, out3 = g32(dev, prec, B, cout, H, W, SENT), g32(dev, prec, B, cout, H, W, SENT)
    gamma = 0.5
    f.c.mask, f.c.out2, f.c.mask_cb_begin, f.c.mask_act = mk.view(0, cout), out2.view(0, cout), 0, L.ACT_LRELU
    f.c.out3, f.c.gamma, f.c.layer3 = out3.view(0, cout), gamma, L.NO_LAYER
    mq = q(m, prec)[f.idx].double()
    f.checks.append(('out2', out2, 0, cout, f.ref_out * torch.where(mq > 0, 1.0, SLOPE)))
    f.checks.append(('out3', out3, 0, cout, f.ref_out * gamma))


def add_ksplit(f, dev):
    """esr_conv.ksplit = 2 with the BatchNorm statistics of the stored output (ops.conv2d's arguments)"""
    f.ws = torch.zeros(2 * f.B * f.H * f.W * cdiv(f.cout, 32) * 32, device=dev)
    f.stats = torch.zeros(1, 2 * f.cout, dtype=torch.float64, device=dev)
    f.c.ksplit, f.c.split_ws = 2, f.ws.data_ptr()
    f.c.stat_sums, f.c.stat_groups, f.c.stat_C = f.stats.data_ptr(), 1, f.cout


def stats_ok(f, res):
    """test_gpu_forward.test_stride2_conv_packed_split_k's check of stat_sums: the sums over the stored values"""
    H, W, co = f.H, f.W, f.cout
    t = res['out']
    ng = cdiv(co, f.cpg)
    y = t[:, :ng, 1:H + 1, 1:W + 1, :].permute(0, 1, 4, 2, 3).reshape(f.B, ng * f.cpg, H, W)[:, :co].double()
    st = f.stats.cpu()
    yg = y.reshape(1, f.B, co, -1)
    return (torch.allclose(st[:, :co], yg.sum(dim=(1, 3)), rtol=1e-6, atol=1e-6) and
            torch.allclose(st[:, co:], (yg * yg).sum(dim=(1, 3)), rtol=1e-6, atol=1e-6))


@pytest.mark.gpu
@pytest.mark.parametrize('case', CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_forward_on_far_views(dev, arena, case):
    name, prec, B, cin, cout, kind, H, W, flags, spec, branch, fams, extra = case
    assert conv_branch(case) == branch
    f = Fwd(dev, 'far_' + name, prec, B, cin, cout, kind, H, W, flags, spec)
    if extra == 'bwd3':
        add_bwd3(f, dev)
    if extra == 'ksplit':
        add_ksplit(f, dev)
    bufs = fwd_bufs(f)
    pre = [b.t.clone() for b in bufs]
    res = f.run()
    e = f.check(res)
    print('far conv %s: compact err/scale %.2e' % (name, e))
    if extra == 'ksplit':
        assert stats_ok(f, res), name
    post = [b.t.clone() for b in bufs]
    compact = f.c

    def launch(rel):
        f.c = rel.op
        if f.nchw is not None:
            f.nchw.fill_(SENT)
        if extra == 'ksplit':
            f.stats.zero_()
        launch.res = f.run()
        f.c = compact

    for fam, rel in far_runs(arena, f.c, bufs, pre, fams, launch, expect=conv_shapes(case)):
        for k in res:                      # the compact buffers as the compact run left them
            assert torch.equal(res[k], launch.res[k]), (name, fam, k)
        same_as_compact(arena, rel, post, '%s %s' % (name, fam))
        if extra == 'ksplit':              # fp64 atomics: the statistics within their own tolerance, not bit for bit
            assert stats_ok(f, res), (name, fam)


TS2_CASES = [   # name, prec, B, cin, cout (of the FORWARD conv), H, W (this op's output), branch, families
    ('f16_ts2_one', 'fp16', 3, 32, 32, 18, 40, 'one', ALL),
    ('f16_ts2_two', 'fp16', 3, 64, 48, 18, 40, 'ts2_one', BG),
    ('f32_ts2_one', 'fp32', 3, 16, 16, 18, 40, 'one', ALL),
]


def ts2_shapes(c):
    name, prec, B, cin, cout, H, W, _, _ = c
    return [(B, cdiv(cout, CPG[prec])) + FV.g32_dims(H // 2, W // 2), (B, cdiv(cin, CPG[prec])) + FV.g32_dims(H, W)]


@pytest.mark.gpu
@pytest.mark.parametrize('case', TS2_CASES, ids=[c[0] for c in TS2_CASES])
def test_transposed_stride2_on_far_views(dev, arena, case):
    """upsample == 2, the adjoint of the 4x4/s2 conv, as test_gpu_conv_backward builds it (its reference and gate)"""
    E, L = _mods()
    name, prec, B, cin, cout, H, W, branch, fams = case
    assert ts2_branch(B, H, W, cdiv(cin, 32)) == branch
    w = q(rnd((cout, cin, 4, 4), 'far.ts2.w', name, scale=1.0 / np.sqrt(cout * 16)), prec)
    gy = q(rnd((B, cout, H // 2, W // 2), 'far.ts2.gy', name), prec)
    idx = [0, B - 1]
    ref = dgrad_ref((name, prec, B, cin, cout, 'ts2', H, W, 0, 'plain', None, None), w, gy, idx)
    dp = E.DgradPack([('c', w.to(dev))], prec, dev, {'c': {'ts2': True}})
    dp.ensure(E.current_stream())
    gin = g32(dev, prec, B, cout, H // 2, W // 2)
    upload(gin, gy)
    out = g32(dev, prec, B, cin, H, W, SENT)
    c = E._conv(E._dt(prec)[0], B, H, W, gin.view(0), cout, out.view(0, cin), dp.entries['c'], L.ACT_NONE,
                ks=4, stride=1, upsample=2)
    c.bias = None
    bufs = [gin, out]
    pre = [b.t.clone() for b in bufs]

    def launch_op(op):
        ops = L.OpList()
        ops.add_conv(op)
        run(ops)
    launch_op(c)
    e = rel_err(region(out)[0][idx, :cin], ref)
    print('far ts2 %s: compact err/scale %.2e' % (name, e))
    assert e <= TOL_DG[prec], e
    assert (region(out)[1] == SENT).all()
    post = [b.t.clone() for b in bufs]
    for fam, rel in far_runs(arena, c, bufs, pre, fams, lambda rel: launch_op(rel.op), expect=ts2_shapes(case)):
        assert all(torch.equal(b.t, p) for b, p in zip(bufs, post))
        same_as_compact(arena, rel, post, '%s %s' % (name, fam))


# ----------------------------------------------------------------------------------------------------------------
# b. the fused dense-block chain, mode 0 (the only family whose offsets its one-descriptor-per-image addressing can
#    hold is the far batch; the others are refusals)
# ----------------------------------------------------------------------------------------------------------------

CHAIN_CASES = [   # name, prec, kind, B, H, W, ESR_RDB_ROWS, force the general kernel
    ('f16_rdb_general', 'fp16', 'rdb', 3, 20, 40, None, False),
    ('f16_rrdb_regular', 'fp16', 'rrdb', 3, 16, 64, '4', False),
    ('f16_rrdb_general', 'fp16', 'rrdb', 3, 16, 64, '4', True),
    ('f32_rrdb', 'fp32', 'rrdb', 3, 20, 40, None, False),
]


def chain_shapes(c):
    name, prec, kind, B, H, W, _, _ = c
    d = FV.g32_dims(H, W)
    return [(B, 64 // CPG[prec]) + d, (B, 64 // CPG[prec]) + d, (B, 128 // CPG[prec]) + d]


@pytest.mark.gpu
@pytest.mark.parametrize('case', CHAIN_CASES, ids=[c[0] for c in CHAIN_CASES])
def test_inference_chain_on_far_batch(dev, arena, monkeypatch, case):
    """esr_rdb_forward mode 0 through Builder.rdb_chain — one block with its dense slices saved (checked against
    float64 stage by stage, test_gpu_chain_stages' reference and gate) and the three blocks of an RRDB with its tail
    (x_in, x_out, res2, dense) in the regular and the general kernel — with x_in, x_out, res2 and dense far"""
    from tests import chain_stage_refs as R
    from tests.test_gpu_chain_stages import TOL as CTOL, Worst, assert_chains_clean, inner
    E, L = _mods()
    name, prec, kind, B, H, W, rows, general = case
    if rows is None:
        monkeypatch.delenv('ESR_RDB_ROWS', raising=False)
    else:
        monkeypatch.setenv('ESR_RDB_ROWS', rows)
    mod = R.block_module(kind).to(dev).eval().set_precision(prec)
    sd = {k: v.detach().cpu() for k, v in mod.state_dict().items()}
    st = E.current_stream()
    bld = E.Builder(mod._weights(dev), B, H, W, prec, dev, False, mod.variant, kind, 1)
    assert E.rdb_chain_ok(B, H, W, False, False)
    P = bld.plan
    xa, xb = bld.buf(64), bld.buf(64)
    P.in_op = bld.import_nchw(xa, 64)
    if kind == 'rdb':
        k = bld.rdb_chain([('rdb', xa, xb, None, None, None)])
    else:
        k = bld.rdb_chain(bld.rrdb_chain_specs('rrdb', 0, xa, xb))
    dense = [b for b in bld.bufs if isinstance(b, E.G32) and b.C == 128][0]
    table = [t for t in bld.bufs if hasattr(t, 'host_table')][0]
    ch = P.ops.ops[k].u.rdb_chain
    ch.save_dense = 1
    P.ops._arr = None
    res_buf = xb if kind == 'rdb' else xa
    P.out_op = bld.export_nchw(res_buf, 64)
    P.out_shape = (B, 64, H, W)
    out = torch.empty(P.out_shape, dtype=torch.float32, device=dev)
    x = R.randn((B, 64, H, W), 145)
    old = L.lib().esr_debug_chain_force_general(1 if general else 0)
    try:
        P.run(x.to(dev), out, st)
        torch.cuda.synchronize()
        assert_chains_clean(P.chain_ws)
        variant = L.lib().esr_debug_chain_last_variant()
        assert bool(variant & 1) == (prec == 'fp16' and rows == '4' and not general), variant
        if kind == 'rdb':
            xs, D, y = inner(xa, 0, 64), inner(dense), inner(xb, 0, 64)
            got = {'x1': D[:, :32], 'x2': D[:, 32:64], 'x3': D[:, 64:96], 'x4': D[:, 96:128], 'y': y}
            fs = R.forward_stages(R.forward_weights(sd, '', prec), xs, got['x1'], got['x2'], got['x3'], got['x4'])
            wst = Worst('far chain %s' % name, CTOL[prec])
            for s in ('x1', 'x2', 'x3', 'x4', 'y'):
                wst.check(s, 'block 0', got[s], fs[s])
            wst.done()
        bufs = [xa, xb, dense]
        post = [b.t.clone() for b in bufs]
        # the far run starts from what the compact chain started from: x in xa (the RRDB's last block wrote xa, so it is
        # imported again), everything else zero as the plan allocated it
        pre = [torch.zeros_like(b.t) for b in bufs]
        tmp = g32(dev, prec, B, 64, H, W)
        upload(tmp, x)
        pre[0] = tmp.t.clone()

        def launch(rel):
            blk = E.upload_table(rel.table, dev)
            launch.keep = blk
            op = rel.op
            op.blocks = blk.data_ptr()
            assert L.lib().esr_rdb_chain_check(op, C.addressof(rel.table)) == 0, L.lib().esr_last_error()
            lst = L.OpList()
            lst.add(L.OP_RDB_CHAIN, 'rdb_chain', op)
            lst.run(st)
            torch.cuda.synchronize()
            assert_chains_clean(P.chain_ws)

        for fam, rel in far_runs(arena, ch, bufs, pre, B_, launch, table=table.host_table, expect=chain_shapes(case)):
            assert all(torch.equal(b.t, p) for b, p in zip(bufs, post))
            same_as_compact(arena, rel, post, '%s %s' % (name, fam))
    finally:
        L.lib().esr_debug_chain_force_general(old)


TRAIN_CHAIN_SHAPE = (3, 64, 24, 40)


def train_chain_bufs(bld):
    """every G32 buffer of a training plan, once"""
    E, _ = _mods()
    out = []
    for b in bld.tp.bufs:
        if isinstance(b, E.G32) and all(b is not o for o in out):
            out.append(b)
    return out


@pytest.mark.gpu
def test_training_chains_on_far_batch(dev, arena, monkeypatch):
    """esr_rdb_forward mode 1 and esr_rdb_backward over the three blocks of an RRDB (res2 and the RRDB tail included), as
    test_gpu_chain_stages builds, steps and checks them against float64 stage by stage.  Then each chain launch alone,
    from the buffers as the step left them: on the compact views and, from the same state, with x_in, x_out, res2,
    dense, aux and out_a on the far batch — every buffer of the plan bit-identical afterwards."""
    from tests import chain_stage_refs as R
    from tests import test_gpu_chain_stages as CS
    E, L = _mods()
    monkeypatch.setenv('ESR_RDB_TRAIN_CHAIN', '1')
    monkeypatch.delenv('ESR_RDB_ROWS', raising=False)
    shape = TRAIN_CHAIN_SHAPE
    B, _, H, W = shape
    mod = R.block_module('rrdb').to(dev).train(False).set_precision('fp16')
    sd = {k: v.detach().cpu() for k, v in mod.state_dict().items()}
    bld = CS.build(mod, 'rrdb', 64, 64, B, H, W, dev, False)
    seed = CS.step(bld, R.randn(shape, 125).to(dev), R.randn(shape, 126).to(dev), False)
    prefixes = R.block_prefixes('rrdb')
    CS.check_train_plan('far batch', bld, sd, lambda i, j: prefixes[j], False, seed, dev)
    tp, st = bld.tp, E.current_stream()
    bufs = train_chain_bufs(bld)
    tables = [t for t in tp.bufs if hasattr(t, 'host_table') and isinstance(t.host_table[0], L.esr_rdb_block)]
    size = C.sizeof(L.esr_rdb_block)
    launches = [(L.OP_RDB_CHAIN, tp.fwd.ops.array()[i].u.rdb_chain, 1) for i in tp.fwd.chain_ops] + \
               [(L.OP_RDB_CHAIN_BWD, tp.bwd.array()[i].u.rdb_chain, 2) for i in tp.bwd_chain_ops]
    assert {m for _, _, m in launches} == {1, 2}
    keep = []
    for kind, ch, mode in launches:
        ch = type(ch).from_buffer_copy(ch)
        assert ch.mode == mode and ch.noise_mode == L.NOISE_OFF
        blk_t = [t for t in tables if 0 <= ch.blocks - t.data_ptr() < t.numel()][0]
        k0 = (ch.blocks - blk_t.data_ptr()) // size
        host = (L.esr_rdb_block * ch.n_blocks)(*blk_t.host_table[k0:k0 + ch.n_blocks])

        def launch(op, table):
            keep.append(E.upload_table(table, dev))
            op.blocks = keep[-1].data_ptr()
            assert L.lib().esr_rdb_chain_check(C.byref(op), C.addressof(table)) == 0, L.lib().esr_last_error()
            lst = L.OpList()
            lst.add(kind, 'rdb_chain', op)
            lst.run(st)
            CS.assert_chains_clean(tp.fwd.chain_ws, tp.bwd_chain_ws)
        pre = [b.t.clone() for b in bufs]
        launch(ch, host)
        post = [b.t.clone() for b in bufs]
        for fam, rel in far_runs(arena, ch, bufs, pre, B_, lambda rel: launch(rel.op, rel.table), table=host):
            assert all(torch.equal(b.t, p) for b, p in zip(bufs, post)), mode
            same_as_compact(arena, rel, post, 'chain mode %d' % mode)


BAND_IMAGE = (8129, 1)        # 509 tiles of 16 x 32 for 256 CUs: three row bands (engine.rdb_band_geometry)


def band_shapes():
    """[mid, dense] of the banded trunk at BAND_IMAGE: three bands of 2720 + 2 x 16 rows"""
    d = FV.g32_dims(2720 + 32, BAND_IMAGE[1])
    return [(3, 4) + d, (3, 8) + d]


@pytest.mark.gpu
def test_banded_chain_with_its_band_local_buffers_far(dev, arena, monkeypatch):
    """The band form of mode 0 (rdb_fused_band), driven through Builder.rdb_chain_banded as test_gpu_chain_valu's
    smallest banded launch is, on an image of three bands; checked against that file's float64 reference and bound.
    The band views of the two tall buffers carry strides of their own (batch_stride = band_rows rows) and stay where
    they are; the band-LOCAL buffers — mid (x_out of blocks 0 and 1, x_in of blocks 1 and 2) and the dense scratch,
    one entry per band — have a free batch stride, which an image of many bands takes past 2^31 and 2^32 in ordinary
    use.  Here they go to the far batch: band 1 past 2^31, band 2 past 2^32; the result, mid and dense bit-identical."""
    from esrganplus_amd import architecture as arch, synth
    from tests import chain_stage_refs as R
    from tests.test_gpu_chain_valu import rrdb_reference
    from tests.test_gpu_chain_variants import TOL as BTOL
    E, L = _mods()
    monkeypatch.delenv('ESR_RDB_ROWS', raising=False)
    H, W = BAND_IMAGE
    geom = E.rdb_band_geometry(H, W)
    assert geom == (2720, 16, 3), geom
    sd = synth.rrdbnet_state_dict(nb=1, seed=21)
    net = arch.RRDBNet(3, 3, 64, 1).to(dev).eval().set_precision('fp16')
    net.load_state_dict(sd, strict=True)
    bld = E.Builder(net._weights(dev), 1, H, W, 'fp16', dev, False, net.variant, 'net', 1)
    P, st = bld.plan, E.current_stream()

    def layout(view, to_g32):
        lo = L.esr_layout()
        lo.dtype, lo.to_g32, lo.B, lo.C, lo.H, lo.W, lo.g32 = bld.dt_e, to_g32, 1, 64, H, W, view
        return P.ops.add(L.OP_LAYOUT, 'layout', lo)

    def head(dst):
        P.in_op = layout(dst, 1)
    P.out_op = layout(bld.rdb_chain_banded(geom, head), 0)
    P.out_shape = (1, 64, H, W)
    x = R.randn((1, 64, H, W), 171)
    out = torch.empty(P.out_shape, dtype=torch.float32, device=dev)
    P.run(x.to(dev), out, st)
    torch.cuda.synchronize()
    assert int(P.chain_ws[1].item()) == 0 and L.lib().esr_rdb_check_abort() == 0
    e = R.rel_err(out.cpu(), rrdb_reference({k: v.detach().cpu() for k, v in sd.items()}, x,
                                            ['model.1.sub.0.RDB%d' % j for j in (1, 2, 3)]))
    print('far band: compact err / scale %.3e (bound %.1e)' % (e, BTOL))
    assert e <= BTOL
    tall0, tall1, mid, dense = [b for b in bld.bufs if isinstance(b, E.G32)]
    assert (mid.B, dense.B, dense.C) == (3, 3, 128) and tall0.B == 1
    ch = P.ops.ops[P.chain_ops[0]].u.rdb_chain
    ch = type(ch).from_buffer_copy(ch)
    assert ch.band_rows == geom[0] and ch.B == 3 and ch.n_blocks == 3
    table = [t for t in bld.bufs if hasattr(t, 'host_table')][0].host_table
    keep_t = []

    def launch(op, tbl):
        tall1.t.zero_()                         # the launch's result (nothing reads it): written again by every run
        keep_t.append(E.upload_table(tbl, dev))
        op.blocks = keep_t[-1].data_ptr()
        assert L.lib().esr_rdb_chain_check(C.byref(op), C.addressof(tbl)) == 0, L.lib().esr_last_error()
        lst = L.OpList()
        lst.add(L.OP_RDB_CHAIN, 'rdb_chain', op)
        lst.run(st)
        torch.cuda.synchronize()
        assert int(P.chain_ws[1].item()) == 0 and L.lib().esr_rdb_check_abort() == 0
    bufs = [tall0, tall1, mid, dense]
    pre = [b.t.clone() for b in bufs]
    launch(ch, table)                           # the chain launch alone, from the state the plan's run left
    post = [b.t.clone() for b in bufs]
    assert torch.equal(post[1], pre[1])         # ... which reproduces the plan's result
    for fam, rel in far_runs(arena, ch, bufs, pre, B_, lambda rel: launch(rel.op, rel.table), table=table,
                             expect=band_shapes(), keep=(tall0, tall1)):
        assert torch.equal(tall1.t, post[1]) and torch.equal(tall0.t, post[0])
        assert torch.equal(mid.t, post[2]) and torch.equal(dense.t, post[3])     # the compact ones: untouched
        same_as_compact(arena, rel, post, 'band form')


# ----------------------------------------------------------------------------------------------------------------
# e. pooling and pixel shuffle (esr_maxpool2 modes 0 to 5), f. esr_convert_layout
# ----------------------------------------------------------------------------------------------------------------

# (family, channel groups of the wider tensor): nine on the far batch, which has no group limit — the only family that
# holds the nine-fold channels of the 3x shuffle (modes 4 / 5)
POOL_CASES = [(p, fam_c) for p in ('fp16', 'fp32') for fam_c in (('batch', 9), ('group', 4), ('plane', 2))]


def nn_shapes(famc):
    """(B, groups, Hp, Wp) of the buffers of every relocation the pool / shuffle / layout / BatchNorm tests launch, by
    name — what the host test proves the arena property for, and what the GPU tests pass as `expect`"""
    fam, ngrp = famc
    B = 3
    px, py = (B, ngrp) + FV.g32_dims(9, 35), (B, ngrp) + FV.g32_dims(4, 17)
    out = {'pool fwd': [px, py], 'pool bwd': [px, py, px], 'layout': [(B, ngrp) + FV.g32_dims(13, 40)]}
    for r in (2, 3):
        if ngrp >= r * r:
            n = ngrp // (r * r)
            wide, narrow = (B, r * r * n) + FV.g32_dims(7, 5), (B, n) + FV.g32_dims(7 * r, 5 * r)
            out['shuffle %d' % r], out['unshuffle %d' % r] = [wide, narrow], [wide, narrow, wide]
    bn = (B, min(ngrp, 4)) + FV.g32_dims(7, 9)
    out.update({'bn stats': [bn], 'bn fin_apply': [bn] * 2, 'bn bwd_reduce': [bn] * 3, 'bn bwd_apply': [bn] * 4})
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('prec,famc', POOL_CASES, ids=['%s-%s' % (p, f[0]) for p, f in POOL_CASES])
def test_pool_and_shuffle_on_far_views(dev, arena, prec, famc):
    """max-pool forward / backward (exact against float64 autograd, test_gpu_nn_kernels' references), pixel shuffle 2
    and 3 and their adjoints (exact), on as many channel groups as the family holds: x, y, g and gx far"""
    from tests.test_gpu_nn_kernels import pool_op, pool_ref
    E, L = _mods()
    fam, ngrp = famc
    cpg, B = CPG[prec], 3
    rng = np.random.default_rng(zlib.crc32(repr((prec, fam)).encode()))

    def both(op, bufs, outs, what):
        """compact run, then the far run; returns the compact output regions"""
        pre = [b.t.clone() for b in bufs]
        run_ops = lambda o: run(_one(L, L.OP_POOL, 'pool', o))
        run_ops(op)
        post = [b.t.clone() for b in bufs]
        for f_, rel in far_runs(arena, op, bufs, pre, (fam,), lambda rel: run_ops(rel.op), expect=nn_shapes(famc)[what]):
            assert all(torch.equal(b.t, p) for b, p in zip(bufs, post))
            same_as_compact(arena, rel, post, '%s %s %s' % (what, prec, fam))
        return [region(o) for o in outs]

    # modes 0 / 1 on an odd input size
    C_, Hi, Wi = ngrp * cpg - 3, 9, 35
    H, W = Hi // 2, Wi // 2
    x = torch.from_numpy(rng.integers(-2, 3, (B, C_, Hi, Wi))).float()
    g = q(torch.from_numpy(rng.standard_normal((B, C_, H, W))).float(), prec)
    xb, gb = g32(dev, prec, B, C_, Hi, Wi), g32(dev, prec, B, C_, H, W)
    upload(xb, x)
    upload(gb, g)
    yb, gxb = g32(dev, prec, B, C_, H, W, SENT), g32(dev, prec, B, C_, Hi, Wi, SENT)
    yref, gxref = pool_ref(x, g, 1)
    (y_in, y_rest), = both(pool_op(prec, L.POOL_FWD, B, C_, H, W, x=xb, y=yb), [xb, yb], [yb], 'pool fwd')
    assert torch.equal(y_in[:, :C_].double(), yref) and (y_in[:, C_:] == 0).all() and (y_rest == SENT).all()
    both(pool_op(prec, L.POOL_BWD, B, C_, H, W, x=xb, g=gb, gx=gxb, relu_mask=1), [xb, gb, gxb], [gxb], 'pool bwd')
    t = gxb.t.float().cpu()
    gx_in = t[:, :, 1:2 * H + 1, 1:2 * W + 1, :].permute(0, 1, 4, 2, 3).reshape(B, gxb.ng * cpg, 2 * H, 2 * W)
    assert torch.equal(gx_in[:, :C_].double(), gxref[:, :, :2 * H, :2 * W]) and (gx_in[:, C_:] == 0).all()
    # modes 2 / 3 (pixel shuffle 2) and 4 / 5 (the phase-major shuffle 3): the wide side has r^2 times the groups, so
    # the narrow side takes a share of what the family holds
    for r, fwd_m, bwd_m in ((2, L.POOL_SHUFFLE, L.POOL_UNSHUFFLE), (3, L.POOL_SHUFFLE3, L.POOL_UNSHUFFLE3)):
        if ngrp < r * r:
            continue
        Cy, h, w = (ngrp // (r * r)) * cpg, 7, 5
        xs = q(torch.from_numpy(rng.standard_normal((B, r * r * Cy, h, w))).float(), prec)
        gs = q(torch.from_numpy(rng.standard_normal((B, Cy, r * h, r * w))).float(), prec)
        xb, gb = g32(dev, prec, B, r * r * Cy, h, w), g32(dev, prec, B, Cy, r * h, r * w)
        upload(xb, xs)
        upload(gb, gs)
        yb, gxb = g32(dev, prec, B, Cy, r * h, r * w, SENT), g32(dev, prec, B, r * r * Cy, h, w, SENT)
        xr = xs.double().requires_grad_(True)
        if r == 2:
            y = F.pixel_shuffle(xr, 2)
        else:    # y[b][c][3h+i][3w+j] = x[b][(3i + j) C + c][h][w]
            y = xr.reshape(B, 3, 3, Cy, h, w).permute(0, 3, 4, 1, 5, 2).reshape(B, Cy, 3 * h, 3 * w)
        y.backward(gs.double())
        (y_in, y_rest), = both(pool_op(prec, fwd_m, B, Cy, h, w, x=xb, y=yb), [xb, yb], [yb], 'shuffle %d' % r)
        assert torch.equal(y_in.double(), y.detach()) and (y_rest == SENT).all()
        (gx_in, gx_rest), = both(pool_op(prec, bwd_m, B, Cy, h, w, x=xb, g=gb, gx=gxb), [xb, gb, gxb], [gxb],
                                 'unshuffle %d' % r)
        assert torch.equal(gx_in.double(), xr.grad) and (gx_rest == SENT).all()


def _one(L, kind, field, st):
    lst = L.OpList()
    lst.add(kind, field, st)
    return lst


@pytest.mark.gpu
@pytest.mark.parametrize('prec,famc', POOL_CASES, ids=['%s-%s' % (p, f[0]) for p, f in POOL_CASES])
def test_batchnorm_on_far_views(dev, arena, prec, famc):
    """esr_batchnorm's four passes over a G32 — STATS (x), FIN_APPLY (x, y), BWD_REDUCE (y, g), BWD_APPLY (y, g, gx) —
    in training mode with LeakyReLU.  The compact run is held to test_gpu_nn_kernels' float64 bounds (its reference
    functions and tolerance formulas).  The statistics are sums of fp64 atomics whose order changes from run to run:
    the far STATS / BWD_REDUCE sums are compared with the compact ones within those bounds, and the far FIN_APPLY /
    BWD_APPLY start from the compact sums, so that y and gx must be bit-identical."""
    from tests import test_gpu_nn_kernels as NK
    E, L = _mods()
    fam, ngrp = famc
    ngrp = min(ngrp, 4)
    cpg, B, H, W, act = CPG[prec], 3, 7, 9, L.ACT_LRELU
    C_ = ngrp * cpg - 3
    x, gamma, beta, rm0, rv0, g, dg0, db0 = NK.bn_inputs(zlib.crc32(repr((prec, fam)).encode()), prec, B, C_, H, W)
    x64, gm64, bt64 = x.double(), gamma.double(), beta.double()
    rig = NK.BNRig(dev, prec, B, C_, H, W, 1, 1, act, x)
    gam, bet = gamma.to(dev), beta.to(dev)
    gbuf = g32(dev, prec, B, C_, H, W)
    upload(gbuf, g)
    ybuf, gxbuf = g32(dev, prec, B, C_, H, W, SENT), g32(dev, prec, B, C_, H, W, SENT)
    mk = lambda v: v.to(dev).clone()
    st_ = dict(mean=mk(torch.zeros(C_)), invstd=mk(torch.zeros(C_)), running_mean=mk(rm0), running_var=mk(rv0))
    sums, sums_b = torch.zeros(2 * C_, dtype=torch.float64, device=dev), torch.zeros(2 * C_, dtype=torch.float64, device=dev)
    fcom = dict(sums=sums, gamma=gam, beta=bet, y=ybuf, **st_)
    bcom = dict(y=ybuf, g=gbuf, sums=sums_b, mean=st_['mean'], invstd=st_['invstd'], gamma=gam, beta=bet)
    passes = [('stats', rig.op(L.BN_STATS, sums=sums)[2], [rig.xbuf]),
              ('fin_apply', rig.op(L.BN_FIN_APPLY, **fcom)[2], [rig.xbuf, ybuf]),
              ('bwd_reduce', rig.op(L.BN_BWD_REDUCE, **bcom)[2], [rig.xbuf, ybuf, gbuf]),
              ('bwd_apply', rig.op(L.BN_BWD_APPLY, gx=gxbuf, **bcom)[2], [rig.xbuf, ybuf, gbuf, gxbuf])]
    go = lambda o: run(_one(L, L.OP_BN, 'bn', o))
    # float64 references of the compact run
    sq = NK.bn_stats_ref(x64, 1)[0]
    yref = NK.act64(F.batch_norm(x64, None, None, gm64, bt64, True, NK.MOM, NK.EPS), act)
    iref, itol, mtol = 1 / (sq['var'] + NK.EPS).sqrt(), NK.inv_rel_tol(sq), 4e-6 * sq['eabs']
    ex = lambda t: t[None, :, None, None]
    xh = (x64 - ex(sq['m'])) * ex(iref)
    for what, op, bufs in passes:
        pre = [b.t.clone() for b in bufs]
        state = {k: v.clone() for k, v in st_.items()}
        go(op)
        post = [b.t.clone() for b in bufs]
        after = {k: v.clone() for k, v in st_.items()}
        if what == 'stats':
            s = sums.cpu().view(2, C_)
            NK.assert_within(s[0], sq['s0'], 4e-6 * sq['sabs'], 'sum x')
            NK.assert_within(s[1], sq['s1'], 4e-6 * sq['s1'], 'sum x^2')
        if what == 'fin_apply':
            ytol = 4e-6 * (ex(gm64).abs() * (x64.abs() + ex(sq['m']).abs()) * ex(iref) + ex(bt64).abs()) + \
                (ex(gm64) * xh).abs() * ex(itol) + ex(mtol * iref * gm64.abs())
            if prec == 'fp16':
                ytol = ytol + 2 ** -11 * yref.abs() + 2 ** -24
            y_k = NK.download(ybuf, C_)
            NK.assert_within(y_k, yref, ytol, 'y')
            assert (region(ybuf)[1] == SENT).all()
            gp = g.double() * NK.act_grad_from_output(y_k, act)
        if what == 'bwd_reduce':
            sb = sums_b.cpu().view(2, C_)
            tol_b = [4e-6 * gp.abs().sum((0, 2, 3)), (4e-6 * gp.abs() * (xh.abs() + (x64.abs() + ex(sq['m']).abs()) * ex(iref)) +
                                                      gp.abs() * xh.abs() * ex(itol)).sum((0, 2, 3))]
            NK.assert_within(sb[0], gp.sum((0, 2, 3)), tol_b[0], 'sum g')
            NK.assert_within(sb[1], (gp * xh).sum((0, 2, 3)), tol_b[1], 'sum g xhat')
        if what == 'bwd_apply':
            xr = x64.clone().requires_grad_(True)
            F.batch_norm(xr, None, None, gm64, bt64, True, NK.MOM, NK.EPS).backward(gp)
            A, Bm = gp.mean((0, 2, 3), keepdim=True), (gp * xh).mean((0, 2, 3), keepdim=True)
            xsc = xh.abs() + (x64.abs() + ex(sq['m']).abs()) * ex(iref)
            gxtol = 2e-5 * ex(gm64).abs() * ex(iref) * (gp.abs() + A.abs() + Bm.abs() * xsc) + xr.grad.abs() * ex(itol) * 2
            if prec == 'fp16':
                gxtol = gxtol + 2 ** -11 * xr.grad.abs() + 2 ** -24
            NK.assert_within(NK.download(gxbuf, C_), xr.grad, gxtol, 'gx')
            assert (region(gxbuf)[1] == SENT).all()
        kept = {'stats': sums, 'bwd_reduce': sums_b}.get(what)
        kept_c = kept.clone() if kept is not None else None

        def launch(rel):
            for k, v in state.items():                 # the per-channel state as it was before the compact pass
                st_[k].copy_(v)
            if kept is not None:
                kept.zero_()
            go(rel.op)

        for f_, rel in far_runs(arena, op, bufs, pre, (fam,), launch, expect=nn_shapes(famc)['bn ' + what]):
            assert all(torch.equal(b.t, p) for b, p in zip(bufs, post))
            same_as_compact(arena, rel, post, 'bn %s %s %s' % (what, prec, fam))
            assert all(torch.equal(st_[k], after[k]) for k in st_), what
            if kept is not None:                       # fp64 atomics: within the sums' own bound, then the compact sums again
                tols = [4e-6 * sq['sabs'], 4e-6 * sq['s1']] if what == 'stats' else tol_b
                for k in range(2):
                    NK.assert_within(kept.cpu().view(2, C_)[k], kept_c.cpu().view(2, C_)[k], tols[k], what + ' sums')
                kept.copy_(kept_c)


@pytest.mark.gpu
@pytest.mark.parametrize('prec,famc', POOL_CASES, ids=['%s-%s' % (p, f[0]) for p, f in POOL_CASES])
def test_layout_on_far_views(dev, arena, prec, famc):
    """esr_convert_layout: NCHW -> G32 (exact for fp32, the fp16 rounding for fp16), G32 -> NCHW, and G32 -> NCHW with
    accumulate, on a ragged channel count: bit-identical to the compact run, which is exact against the host values"""
    E, L = _mods()
    fam, ngrp = famc
    cpg, B, H, W = CPG[prec], 3, 13, 40
    C_ = ngrp * cpg - 3
    x = rnd((B, C_, H, W), 'far.layout', prec, fam)
    xd = x.to(dev)
    buf = g32(dev, prec, B, C_, H, W, SENT)

    def op(to_g32, nchw, acc=0):
        lo = L.esr_layout()
        lo.dtype, lo.to_g32, lo.B, lo.C, lo.H, lo.W = buf.esr_dtype, to_g32, B, C_, H, W
        lo.nchw, lo.g32, lo.accumulate = nchw.data_ptr(), buf.view(0, C_), acc
        return lo
    go = lambda o: run(_one(L, L.OP_LAYOUT, 'layout', o))
    pre = [buf.t.clone()]
    imp = op(1, xd)
    go(imp)
    post = [buf.t.clone()]
    inner = region(buf)[0]
    assert torch.equal(inner[:, :C_], q(x, prec)) and (inner[:, C_:] == 0).all()
    for f_, rel in far_runs(arena, imp, [buf], pre, (fam,), lambda rel: go(rel.op), expect=nn_shapes(famc)['layout']):
        same_as_compact(arena, rel, post, 'layout import %s %s' % (prec, fam))
    base = rnd((B, C_, H, W), 'far.layout.base', prec, fam)
    for acc in (0, 1):
        out = base.to(dev).clone()
        exp = op(0, out, acc)
        go(exp)
        want = q(x, prec) + base if acc else q(x, prec)
        assert torch.equal(out.cpu(), want)
        far_out = base.to(dev).clone()

        def launch(rel):
            rel.op.nchw = far_out.data_ptr()
            go(rel.op)
        for f_, rel in far_runs(arena, exp, [buf], post, (fam,), launch, expect=nn_shapes(famc)['layout']):
            assert torch.equal(far_out, out)
            same_as_compact(arena, rel, post, 'layout export %s %s' % (prec, fam))


# ----------------------------------------------------------------------------------------------------------------
# d. weight gradients of one conv: the fp32 kernel (no limit: every family), the fp16 kernels on the far batch (their
#    32-bit offsets span the groups of ONE image; the packed <= 16-column form spans the images of a tile too and has
#    no far family it can address: it is a refusal below), and a run of ops through esr_conv_wgrad_multi
# ----------------------------------------------------------------------------------------------------------------

WG_FAR = [   # WgradRig case (prec, B, cin, cout, ks, stride, upsample, H, W), families
    (('fp32', 3, 16, 16, 3, 1, 0, 13, 40), ALL),
    (('fp32', 3, 32, 24, 3, 1, 1, 12, 36), BG),
    (('fp32', 3, 16, 16, 1, 1, 0, 9, 33), ALL),
    (('fp32', 3, 16, 16, 4, 2, 0, 9, 20), ALL),
    (('fp16', 3, 48, 32, 3, 1, 0, 37, 33), B_),
    (('fp16', 3, 64, 64, 3, 1, 1, 20, 66), B_),
    (('fp16', 3, 64, 96, 1, 1, 0, 9, 33), B_),
    (('fp16', 3, 48, 64, 4, 2, 0, 9, 20), B_),
]
WG_MULTI = [('fp16', 3, 64, 32, 3, 1, 0, 12, 40), ('fp16', 3, 48, 64, 3, 1, 0, 9, 33), ('fp16', 3, 64, 32, 1, 1, 0, 12, 40),
            ('fp16', 3, 48, 72, 1, 1, 0, 9, 33)]            # the four batch kinds of test_gpu_conv_backward's multi run


def wg_shapes(case):
    """[g, in] as WgradRig allocates them"""
    prec, B, cin, cout, ks, st, ups, H, W = case
    Hi, Wi = (H // 2, W // 2) if ups else (H * st, W * st)
    return [(B, cdiv(cout, CPG[prec])) + FV.g32_dims(H, W), (B, cdiv(cin, CPG[prec])) + FV.g32_dims(Hi, Wi)]


def wg_run(dev, wgs, outs):
    """the esr_wgrad structs as ONE op list (consecutive ops go through esr_conv_wgrad_multi) with the deterministic
    arena, into zeroed dw / db; returns their copies"""
    E, L = _mods()
    for dw, db in outs:
        dw.zero_()
        db.zero_()
    ops = L.OpList()
    for wg in wgs:
        ops.add(L.OP_WGRAD, 'wgrad', wg)
    arena_ = E.attach_wgrad_arena(ops, dev)
    assert arena_ is not None
    run(ops)
    return [(dw.clone(), db.clone()) for dw, db in outs]


@pytest.mark.gpu
@pytest.mark.parametrize('case,fams', WG_FAR, ids=['-'.join(str(v) for v in c) for c, _ in WG_FAR])
def test_conv_wgrad_on_far_views(dev, arena, case, fams):
    """dW and db against float64 autograd (test_gpu_conv_backward's rig, reference and gate), then the same op with g
    and in far: the two-stage reduction is deterministic, so the gradients are bit-identical"""
    from tests.test_gpu_conv_backward import TOL_WG
    assert not wgrad16_grid(case[1], case[7], case[8], case[3], case[2], case[4], case[5], case[6])['packed']
    rig = WgradRig(dev, case)
    n = rig.cout * rig.cin * rig.ks * rig.ks
    outs = [(torch.zeros(n, device=dev), torch.zeros(rig.cout, device=dev))]
    wg = rig.op(*outs[0])
    bufs = [rig.gin, rig.xin]
    pre = [b.t.clone() for b in bufs]
    (dw, db), = wg_run(dev, [wg], outs)
    ew = rel_err(dw.cpu().reshape(rig.ref_w.shape), rig.ref_w)
    eb = rel_err(db.cpu(), rig.ref_b)
    print('far wgrad %s: dW err/scale %.2e, db %.2e' % (case, ew, eb))
    assert ew <= TOL_WG and eb <= TOL_WG, (ew, eb)
    got = {}
    for fam, rel in far_runs(arena, wg, bufs, pre, fams, lambda rel: got.update(r=wg_run(dev, [rel.op], outs)),
                             expect=wg_shapes(case)):
        assert torch.equal(got['r'][0][0], dw) and torch.equal(got['r'][0][1], db), (case, fam)
        same_as_compact(arena, rel, pre, 'wgrad %s %s' % (case, fam))


@pytest.mark.gpu
def test_conv_wgrad_multi_on_far_batch(dev, arena):
    """four batchable fp16 ops in one list (one batched launch of esr_conv_wgrad_multi, all four kinds): each against
    float64, then all eight views on the far batch, bit-identical"""
    from tests.test_gpu_conv_backward import TOL_WG, batch_grid
    assert {batch_grid(c[1], c[7], c[8], c[3], c[2], c[4])[1] for c in WG_MULTI} == {0, 1, 2, 3}
    rigs = [WgradRig(dev, c) for c in WG_MULTI]
    outs = [(torch.zeros(r.cout * r.cin * r.ks * r.ks, device=dev), torch.zeros(r.cout, device=dev)) for r in rigs]
    wgs = [r.op(*o) for r, o in zip(rigs, outs)]
    bufs = [b for r in rigs for b in (r.gin, r.xin)]
    pre = [b.t.clone() for b in bufs]
    first = wg_run(dev, wgs, outs)
    for r, (dw, db) in zip(rigs, first):
        assert rel_err(dw.cpu().reshape(r.ref_w.shape), r.ref_w) <= TOL_WG and rel_err(db.cpu(), r.ref_b) <= TOL_WG, r.case
    got = {}
    expect = [s for c in WG_MULTI for s in wg_shapes(c)]
    for fam, rel in far_runs(arena, wgs[0], bufs, pre, B_, lambda rel: got.update(r=wg_run(dev, [rel.op] + list(rel.table), outs)),
                             table=wgs[1:], expect=expect):
        for (dw, db), (dw2, db2) in zip(first, got['r']):
            assert torch.equal(dw, dw2) and torch.equal(db, db2)
        same_as_compact(arena, rel, pre, 'wgrad multi')


# ----------------------------------------------------------------------------------------------------------------
# c. esr_rdb_wgrad_run, one and three blocks, `in` and `q` on the far batch (one image must end below 2^31 bytes of its
#    base, and batch_stride is the descriptor's size: FAR fits; far groups and near-limit planes are refusals)
# ----------------------------------------------------------------------------------------------------------------

def rdb_wgrad_shapes(n_blocks, B=3, H=5, W=40):
    return [s for _ in range(min(n_blocks, 3)) for s in ((B, 12) + FV.g32_dims(H, W), (B, 14) + FV.g32_dims(H, W))]


@pytest.mark.gpu
@pytest.mark.parametrize('n_blocks', [1, 3])
def test_rdb_wgrad_on_far_batch(dev, arena, n_blocks):
    """test_gpu_rdb_wgrad's inputs, float64 correlation and bound; the pass is deterministic (its own test), so the far
    run's gradients are bit-identical"""
    from tests import test_gpu_rdb_wgrad as RW
    E, L = _mods()
    B, H, W = 3, 5, 40
    pairs = [RW._upload(dev, B, H, W, 70 + j) for j in range(n_blocks)]
    outs = [RW._outputs(dev) for _ in range(n_blocks)]
    wbs = (L.esr_rdb_wgrad_block * n_blocks)()
    for i in range(n_blocks):
        wbs[i].in_, wbs[i].q = pairs[i][2].view(0, 192), pairs[i][3].view(0, 224)
        for k in range(6):
            wbs[i].dw[k] = outs[i][0][k].data_ptr()
        for k in range(5):
            wbs[i].db[k] = outs[i][1][k].data_ptr()
    need = int(L.lib().esr_rdb_wgrad_workspace_elems(B, H, W, n_blocks))
    part = torch.empty(need, dtype=torch.float32, device=dev)
    rw = L.esr_rdb_wgrad()
    rw.dtype, rw.B, rw.H, rw.W, rw.n_blocks, rw.tap_major = L.ESR_F16, B, H, W, n_blocks, 0
    rw.scale5, rw.scale, rw.partial, rw.partial_elems = 0.2, 1.0, part.data_ptr(), need

    def launch(table):
        for dws, dbs in outs:
            for t in dws + dbs:
                t.zero_()
        assert L.lib().esr_rdb_wgrad_check(C.byref(rw), C.addressof(table)) == 0, L.lib().esr_last_error()
        blk = E.upload_table(table, dev)
        rw.blocks = blk.data_ptr()
        L.check(L.lib().esr_rdb_wgrad_run(C.byref(rw), C.c_void_p(E.current_stream())), 'esr_rdb_wgrad_run')
        torch.cuda.synchronize()
        return [[t.clone() for t in dws + dbs] for dws, dbs in outs]
    first = launch(wbs)
    for i in range(n_blocks):
        rdw, rdb = RW._reference(*pairs[i][:2])
        RW._check_block(outs[i][0], outs[i][1], rdw, rdb, 1.0, 'block %d' % i)
    bufs = [b for p in pairs for b in p[2:]]
    pre = [b.t.clone() for b in bufs]
    got = {}
    for fam, rel in far_runs(arena, rw, bufs, pre, B_, lambda rel: got.update(r=launch(rel.table)), table=wbs,
                             expect=rdb_wgrad_shapes(n_blocks)):
        assert all(torch.equal(a, b) for x, y in zip(first, got['r']) for a, b in zip(x, y))
        same_as_compact(arena, rel, pre, 'rdb_wgrad %d' % n_blocks)


# ----------------------------------------------------------------------------------------------------------------
# g. the image ends: three slots (batch entries) of one channel group.  The far batch puts slot 1 past 2^31 and slot 2
#    past 2^32, the near-limit plane stretches the rows; a far GROUP does not exist for a one-group view.
# ----------------------------------------------------------------------------------------------------------------

ENDS = ['dihedral', 'dihedral_reduce', 'tile', 'tile_x8', 'tile_many', 'tile_img', 'tile_set_x8']
END_FAMS = ('batch', 'plane')
END_IMG, END_TILE, END_PAD = (20, 26), 8, 2                      # windows of 12 x 12, a 3 x 4 tile grid


def ends_shapes(what):
    h, w = END_IMG if what.startswith('dihedral') else (END_TILE + 2 * END_PAD,) * 2
    return [(3, 1) + FV.g32_dims(h, w)]


@pytest.mark.gpu
@pytest.mark.parametrize('prec', ['fp16', 'fp32'])
@pytest.mark.parametrize('what', ENDS)
def test_image_ends_on_far_slots(dev, arena, what, prec):
    """Every end that writes G32 slots (and the dihedral reduce, which reads them), as its own test file checks it: the
    whole slot buffer, byte for byte, against the layout kernel on torch's slicing / transforms of the image — then the
    same op with the slot view far, bit-identical."""
    from esrganplus_amd import functional as Fn
    E, L = _mods()
    C_, (H, W), tile, pad = 3, END_IMG, END_TILE, END_PAD
    x = rnd((1, C_, H, W), 'far.ends', what).to(dev)
    x2 = rnd((1, C_, H, W), 'far.ends2', what).to(dev)
    th, tw, ny, nx, tiles = Fn.tiled_geometry(H, W, tile, pad)
    win = lambda img, t: img[:, :, tiles[t][4]:tiles[t][4] + th, tiles[t][5]:tiles[t][5] + tw]
    h, w = (H, W) if what.startswith('dihedral') else (th, tw)
    got, ref = g32(dev, prec, 3, C_, h, w, SENT), g32(dev, prec, 3, C_, h, w, SENT)
    keep = []

    def table(entries):
        rec = np.zeros(len(entries), dtype=Fn._tile_item_dtype())
        for k, (img, t, live) in enumerate(entries):
            rec[k] = (img.data_ptr(), H, W, t, live)
        keep.append(torch.from_numpy(rec.view(np.uint8).copy()).to(dev))
        return keep[-1].data_ptr()

    dt = got.esr_dtype
    if what in ('dihedral', 'dihedral_reduce'):
        d, fn = L.esr_dihedral(), 'esr_dihedral_op'
        d.dtype, d.to_g32, d.B, d.C, d.H, d.W, d.nchw = dt, 1, 1, C_, H, W, x.data_ptr()
        d.k_begin, d.k_count, d.scale = 0, 3, 1.0
        want = torch.cat([Fn.x8_transform(x, k) for k in range(3)], 0)
    elif what == 'tile':
        d, fn = L.esr_tile(), 'esr_tile_op'
        d.dtype, d.to_g32, d.B, d.C, d.H, d.W, d.nchw = dt, 1, 1, C_, H, W, x.data_ptr()
        d.tile, d.pad, d.scale, d.t_begin, d.t_count = tile, pad, 1, 5, 3
        want = torch.cat([win(x, t) for t in (5, 6, 7)], 0)
    elif what == 'tile_x8':
        d, fn = L.esr_tile_x8(), 'esr_tile_x8_op'
        d.dtype, d.to_g32, d.B, d.C, d.H, d.W, d.nchw = dt, 1, 1, C_, H, W, x.data_ptr()
        d.tile, d.pad, d.scale, d.t_begin, d.t_count = tile, pad, 1, 6, 1
        d.k_begin, d.k_count, d.mean_scale = 1, 3, 1.0
        want = torch.cat([Fn.x8_transform(win(x, 6), k) for k in (1, 2, 3)], 0)
    elif what in ('tile_many', 'tile_img'):
        d, fn = (L.esr_tile_many(), 'esr_tile_many_op') if what == 'tile_many' else (L.esr_tile_img(), 'esr_tile_img_op')
        if what == 'tile_img':
            u8 = [torch.randint(0, 256, (H, W, C_), generator=torch.Generator().manual_seed(5 + i), dtype=torch.uint8).to(dev)
                  for i in range(2)]
            lut = (torch.arange(256, dtype=torch.float32) / 255.0).to(dev)
            src = u8
            x, x2 = (lut[u.permute(2, 0, 1).long()].unsqueeze(0).contiguous() for u in u8)
        else:
            src = [x, x2]
        d.dtype, d.to_g32, d.C, d.tile, d.pad, d.scale, d.th, d.tw, d.n_slots = dt, 1, C_, tile, pad, 1, th, tw, 3
        d.items = table([(src[0], 0, 1), (src[1], 11, 1), (src[0], 6, 0)])        # the last one a filler: gathered too
        want = torch.cat([win(x, 0), win(x2, 11), win(x, 6)], 0)
    else:
        d, fn = L.esr_tile_set_x8(), 'esr_tile_set_x8_op'
        d.dtype, d.to_g32, d.C, d.tile, d.pad, d.scale, d.th, d.tw, d.n_windows = dt, 1, C_, tile, pad, 1, th, tw, 1
        d.items = table([(x, 7, 1)])
        d.k_begin, d.k_count, d.mean_scale = 0, 3, 1.0
        want = torch.cat([Fn.x8_transform(win(x, 7), k) for k in range(3)], 0)
    d.g32 = got.view(0, C_)
    upload(ref, want.contiguous())
    call = lambda op: (L.check(getattr(L.lib(), fn)(C.byref(op), C.c_void_p(E.current_stream())), fn), torch.cuda.synchronize())
    if what == 'dihedral_reduce':
        # the reduce reads the slots: y = (R_0(o_0) + R_1(o_1) + R_2(o_2)) * scale, sequential fp32 adds (test_gpu_x8)
        got.t.copy_(ref.t)
        outs = [q(want[k:k + 1], prec).to(dev) for k in range(3)]
        acc = Fn.x8_inverse(outs[0], 0)
        for k in (1, 2):
            acc = acc + Fn.x8_inverse(outs[k], k)
        y = torch.full((1, C_, H, W), SENT, device=dev)
        d.to_g32, d.nchw, d.scale = 0, y.data_ptr(), 0.5
        pre = [got.t.clone()]
        call(d)
        assert torch.equal(y, acc * 0.5)
        y_far = torch.full((1, C_, H, W), SENT, device=dev)

        def launch(rel):
            rel.op.nchw = y_far.data_ptr()
            call(rel.op)
        for fam, rel in far_runs(arena, d, [got], pre, END_FAMS, launch, expect=ends_shapes(what)):
            assert torch.equal(y_far, y), (what, fam)
            same_as_compact(arena, rel, pre, '%s %s' % (what, fam))
            y_far.fill_(SENT)
        return
    pre = [got.t.clone()]
    call(d)
    assert torch.equal(got.t.view(torch.uint8), ref.t.view(torch.uint8)), what     # halo and padding: the sentinel in both
    assert not bool((got.t[:, :, 1:h + 1, 1:w + 1, :C_] == SENT).any())
    post = [got.t.clone()]
    for fam, rel in far_runs(arena, d, [got], pre, END_FAMS, lambda rel: call(rel.op), expect=ends_shapes(what)):
        assert torch.equal(got.t, post[0])
        same_as_compact(arena, rel, post, '%s %s' % (what, fam))


# ----------------------------------------------------------------------------------------------------------------
# refusals: nothing is launched
# ----------------------------------------------------------------------------------------------------------------

def refused(arena, call, words):
    """call() returns a status of the C ABI: ESR_ERR_INVALID (-1) or ESR_ERR_UNSUPPORTED (-3), with a message that
    names the limit"""
    _, L = _mods()
    rc = call()
    msg = L.lib().esr_last_error().decode()
    assert rc in (-1, -3), (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


@pytest.mark.gpu
def test_views_beyond_a_limit_are_refused(dev, arena):
    """conv: a plane of `in` at the 2^31 line, and the PACK branch on the far batch; the fp16 weight gradients on the
    far group, on two near-limit planes and (packed tiles) on the far batch; the chain's dense scratch on the far
    group.  The arena holds the operands and is scanned afterwards: no byte moved."""
    E, L = _mods()
    st = C.c_void_p(E.current_stream())
    lib = L.lib()
    placed = []

    def far(op, bufs, fam, table=None):
        rel = FV.relocate(op, bufs, fam, arena, table=table)
        placed.extend(rel.used)
        return rel

    # conv: the near-limit plane with one more pixel of pitch
    f = Fwd(dev, 'far_refuse_plane', 'fp16', 3, 32, 32, '3x3', 13, 40, 0, lre())
    rel = far(f.c, fwd_bufs(f), 'plane')
    ok = rel.op
    bad = type(ok).from_buffer_copy(ok)
    bad.in_.wp = FV.plane_wp(f.xin.Hp) + 1
    refused(arena, lambda: lib.esr_conv_forward(C.byref(bad), st), ['plane', '2^31'])
    # conv, PACK branch: the images of a tile through (bi - b) * (int)batch_stride
    f2 = Fwd(dev, 'far_refuse_pack', 'fp16', 3, 64, 64, 's2', 8, 8, 0, lre())
    add_ksplit(f2, dev)
    rel2 = far(f2.c, fwd_bufs(f2), 'batch')
    refused(arena, lambda: lib.esr_conv_forward(C.byref(rel2.op), st), ['batch_stride', '2^31'])
    f3 = Fwd(dev, 'far_refuse_pack_plane', 'fp16', 3, 32, 32, 's2', 8, 8, 0, lre())
    add_ksplit(f3, dev)
    rel3 = far(f3.c, fwd_bufs(f3), 'plane')            # the images of the tile on top of a plane just below the limit
    refused(arena, lambda: lib.esr_conv_forward(C.byref(rel3.op), st), ['batch_stride', '2^31'])
    # fp16 weight gradients: 32-bit offsets across the groups of an image (and the images of a packed tile)
    for case, fam in ((('fp16', 3, 64, 64, 3, 1, 0, 13, 40), 'group'), (('fp16', 3, 32, 32, 3, 1, 0, 13, 40), 'plane'),
                      (('fp16', 3, 64, 64, 4, 2, 0, 3, 6), 'batch')):
        rig = WgradRig(dev, case)
        dw = torch.full((rig.cout * rig.cin * 16,), SENT, device=dev)
        db = torch.full((rig.cout,), SENT, device=dev)
        assert wgrad16_grid(case[1], case[7], case[8], case[3], case[2], case[4], case[5], case[6])['packed'] == (fam == 'batch')
        rw = far(rig.op(dw, db), [rig.gin, rig.xin], fam)
        refused(arena, lambda: lib.esr_conv_wgrad(C.byref(rw.op), st), ['32-bit', '2^31'])
        refused(arena, lambda: lib.esr_conv_wgrad_multi(C.byref(rw.op), 1, st), ['32-bit', '2^31'])
        torch.cuda.synchronize()
        assert (dw == SENT).all() and (db == SENT).all()
    # the chain: its dense scratch (the view the launcher can read) and a block table (esr_rdb_chain_check on the host copy)
    xa, xb, dn = (g32(dev, 'fp16', 1, n, 16, 32) for n in (64, 64, 128))
    blocks = (L.esr_rdb_block * 1)()
    blocks[0].x_in, blocks[0].x_out = xa.view(0, 64), xb.view(0, 64)
    ws_bytes = lib.esr_rdb_workspace_bytes(1, 16, 32)
    ws = torch.zeros((ws_bytes + 3) // 4, dtype=torch.int32, device=dev)
    ch = L.esr_rdb_chain()
    ch.dtype, ch.B, ch.H, ch.W, ch.n_blocks, ch.mode, ch.sigma = L.ESR_F16, 1, 16, 32, 1, 0, 0.1
    ch.dense = dn.view(0, 128)
    ch.workspace, ch.workspace_bytes = ws.data_ptr(), ws_bytes
    dev_blocks = E.upload_table(blocks, dev)                      # (never read: every launch below is refused first)
    ch.blocks = dev_blocks.data_ptr()
    assert lib.esr_rdb_chain_check(C.byref(ch), C.addressof(blocks)) == 0, lib.esr_last_error()
    # the dense scratch's eight groups one group stride past what a 32-bit offset holds — all of them, and their
    # int32 / uint32 aliases, inside the arena
    gs7 = ((1 << 31) // 7 + 4095) // 4096 * 4096
    bad = type(ch).from_buffer_copy(ch)
    bad.dense.ptr, bad.dense.group_stride, bad.dense.batch_stride = arena.t.data_ptr() + FV.PTR_OFF, gs7, 8 * gs7
    assert FV.PTR_OFF + 8 * gs7 + FV.TAIL <= arena.n and 7 * gs7 >= 1 << 31
    refused(arena, lambda: lib.esr_rdb_forward(C.byref(bad), st), ['dense', '2^31'])
    refused(arena, lambda: lib.esr_rdb_chain_check(C.byref(bad), None), ['dense', '2^31'])
    nd = type(ch).from_buffer_copy(ch)                            # the block table's views on the far group
    nd.dense = L.esr_g32()
    relc = far(nd, [xa, xb], 'group', table=blocks)
    refused(arena, lambda: lib.esr_rdb_chain_check(C.byref(ch), C.addressof(relc.table)), ['x_in', '2^31'])
    # the dense-block weight gradients: the block table again
    sin, sq = g32(dev, 'fp16', 1, 64, 16, 32), g32(dev, 'fp16', 1, 64, 16, 32)
    wb = (L.esr_rdb_wgrad_block * 1)()
    wb[0].in_, wb[0].q = sin.view(0, 64), sq.view(0, 64)
    rwg = L.esr_rdb_wgrad()
    rwg.dtype, rwg.B, rwg.H, rwg.W, rwg.n_blocks = L.ESR_F16, 1, 16, 32, 1
    relw = far(rwg, [sin, sq], 'group', table=wb)
    refused(arena, lambda: lib.esr_rdb_wgrad_check(C.byref(rwg), C.addressof(relw.table)), ['`in` of block 0', '2^31'])

    # the near-limit plane under the chain and under the dense-block weight gradients: their views have four and more
    # groups, each a plane just below 2^31 — past the arena, so the views are only described (both checks are host
    # functions that launch nothing and never follow a pointer)
    def plane_view(buf, ngroups):
        v = buf.view(0, ngroups * buf.cpg)
        v.wp = FV.plane_wp(buf.Hp)
        v.group_stride = buf.Hp * v.wp * 32
        v.batch_stride = ngroups * v.group_stride
        return v
    pblocks = (L.esr_rdb_block * 1)()
    pblocks[0].x_in, pblocks[0].x_out = plane_view(xa, 4), plane_view(xb, 4)
    refused(arena, lambda: lib.esr_rdb_chain_check(C.byref(ch), C.addressof(pblocks)), ['x_in of block 0', '2^31'])
    pd = type(ch).from_buffer_copy(ch)
    pd.dense = plane_view(dn, 8)
    refused(arena, lambda: lib.esr_rdb_chain_check(C.byref(pd), None), ['dense', '2^31'])
    pwb = (L.esr_rdb_wgrad_block * 1)()
    pwb[0].in_, pwb[0].q = plane_view(sin, 12), plane_view(sq, 14)
    refused(arena, lambda: lib.esr_rdb_wgrad_check(C.byref(rwg), C.addressof(pwb)), ['`in` of block 0', '2^31'])
    # the packed transposed 4x4/s2 conv (upsample == 2 with ksplit) on the far batch: the images of a tile again
    w = q(rnd((64, 64, 4, 4), 'far.refuse.ts2.w', scale=1.0 / 32), 'fp16')
    dp = E.DgradPack([('c', w.to(dev))], 'fp16', dev, {'c': {'ts2': True}})
    dp.ensure(E.current_stream())
    gin, tout = g32(dev, 'fp16', 3, 64, 4, 4), g32(dev, 'fp16', 3, 64, 8, 8, SENT)
    ct = E._conv(L.ESR_F16, 3, 8, 8, gin.view(0), 64, tout.view(0, 64), dp.entries['c'], L.ACT_NONE, ks=4, stride=1, upsample=2)
    ct.bias = None
    tws = torch.zeros(2 * 3 * 8 * 8 * 64, device=dev)
    ct.ksplit, ct.split_ws = 2, tws.data_ptr()
    ops = L.OpList()
    ops.add_conv(ct)
    run(ops)                                                      # compact: the packed launch is accepted ...
    assert not bool((region(tout)[0] == SENT).any())
    relt = far(ct, [gin, tout], 'batch')                          # ... and refused with `in` on the far batch
    refused(arena, lambda: lib.esr_conv_forward(C.byref(relt.op), st), ['batch_stride', '2^31'])
    torch.cuda.synchronize()
    try:
        assert arena.scan(placed)
    finally:
        arena.t.fill_(FV.FILL)
