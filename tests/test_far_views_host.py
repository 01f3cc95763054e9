"""What tests/test_gpu_far_views.py relies on, proved without a GPU: the arena property of every launched case (no
32-bit truncation of a legal offset leaves the arena), that every family crosses the lines it claims, the dispatch
branch every conv case pins, and the engine's side of the address limits (DESIGN.md "Address widths")."""
import ctypes as C

import pytest
import torch

from tests import far_views as FV
from tests import test_gpu_far_views as T


def launched():
    """(what, family, shapes) of every relocation the GPU file launches"""
    for c in T.CONV_CASES:
        for fam in c[11]:
            yield 'conv ' + c[0], fam, T.conv_shapes(c)
    for c in T.TS2_CASES:
        for fam in c[8]:
            yield 'ts2 ' + c[0], fam, T.ts2_shapes(c)
    for c in T.CHAIN_CASES:
        yield 'chain ' + c[0], 'batch', T.chain_shapes(c)
    yield 'band form', 'batch', T.band_shapes()
    for fam, ngrp in sorted({f for _, f in T.POOL_CASES}):
        for what, shapes in T.nn_shapes((fam, ngrp)).items():
            yield what, fam, shapes
    for case, fams in T.WG_FAR:
        for fam in fams:
            yield 'wgrad %s' % (case,), fam, T.wg_shapes(case)
    yield 'wgrad multi', 'batch', [s for c in T.WG_MULTI for s in T.wg_shapes(c)]
    for n in (1, 3):
        yield 'rdb_wgrad %d' % n, 'batch', T.rdb_wgrad_shapes(n)
    for what in T.ENDS:
        for fam in T.END_FAMS:
            yield what, fam, T.ends_shapes(what)


def test_g32_dims_restated():
    from esrganplus_amd import _lib as L
    for H, W in ((1, 1), (13, 40), (32, 32), (33, 64), (20, 70), (339, 510)):
        assert FV.g32_dims(H, W) == L.g32_dims(H, W)


def test_every_launched_case_stays_inside_the_arena():
    n = 0
    for what, fam, shapes in launched():
        fbs = FV.plan(fam, shapes)
        assert FV.fits(fbs, T.ARENA_BYTES), (what, fam)
        assert FV.PTR_OFF >= (1 << 31) + (64 << 20)
        # windows of one case never overlap
        spans = sorted((lo, hi) for fb in fbs for *_, lo, hi in fb.windows()) if fam != 'plane' else []
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), (what, fam)
        n += 1
    assert n > 80 and T.ARENA_BYTES <= FV.ARENA_MAX == 9 << 30


def test_the_property_is_not_vacuous():
    """a fifth far group, a fourth far image or a third near-limit plane would leave the arena: such cases are Unfit or
    fail fits(), so they are never launched"""
    d = FV.g32_dims(13, 40)
    for fam, shape in (('group', (1, 5) + d), ('batch', (4, 2) + d), ('plane', (1, 3) + d)):
        with pytest.raises(FV.Unfit):
            FV.plan(fam, [shape])
    fb = FV.FarBuf('group', 0, 1, 5, d[0], d[1], d[0] * d[1] * 32, FV.FAR, d[1])
    assert not FV.fits([fb], T.ARENA_BYTES)
    # and the truncations are what a missing cast computes
    assert FV.i32(FV.FAR) == FV.FAR - (1 << 32) and FV.u32(2 * FV.FAR) == 2 << 20 and FV.i32(3 * FV.FAR) == FV.FAR - (1 << 32) + (2 << 20)


def test_every_family_crosses_the_line_it_claims():
    d = FV.g32_dims(13, 40)
    # far batch, B = 3: image 1 wholly in [2^31, 2^32) (differs from its int32 truncation), image 2 past 2^32 (differs
    # from both truncations)
    fbs = FV.plan('batch', [(3, 2) + d])
    assert FV.crossings(fbs)[:2] == (2, 2)
    # far group, 4 groups: group 1 past 2^31, groups 2 and 3 past 2^32
    fbs = FV.plan('group', [(1, 4) + d])
    assert FV.crossings(fbs)[:2] == (1, 2)
    for fb in fbs:
        for b, g, lo, hi in fb.windows():
            o = lo - fb.base
            assert (FV.i32(o) != o) == (g >= 1) and (FV.u32(o) != o) == (g >= 2)
    # near-limit plane: the plane ends within 1 MiB below 2^31 (its last row begins one pitch lower), group 1 lies beyond
    fbs = FV.plan('plane', [(1, 2) + d])
    mid, far, near = FV.crossings(fbs)
    assert 0 < (1 << 31) - fbs[0].gs <= 1 << 20 and (1 << 31) - near <= fbs[0].wp * 32 + (1 << 20)
    (_, _, lo1, hi1), = [w for w in fbs[0].windows() if w[1] == 1]
    assert (1 << 31) - (1 << 20) <= lo1 < 1 << 31 < hi1 < 1 << 32       # group 1: its first row straddles 2^31, the rest beyond
    assert fbs[0].wp == 1766022 and fbs[0].gs == 38 * 1766022 * 32       # H = 13: Hp = 38 rows of esr_g32_dims
    assert (fbs[0].Hp * (fbs[0].wp + 1) * 32) >= 1 << 31                 # one more pixel of pitch is refused


def test_far_conv_cases_pin_their_branches():
    from tests.test_gpu_conv_backward import ts2_branch
    for c in T.CONV_CASES:
        assert T.conv_branch(c) == c[10], c[0]
    for c in T.TS2_CASES:
        assert ts2_branch(c[2], c[5], c[6], T.cdiv(c[3], 32)) == c[7], c[0]
    seen = {(c[1], c[5], c[10]) for c in T.CONV_CASES}
    for rw in (1, 2, 4):          # 3x3 on 1-, 2- and 4-row tiles: plain and pipelined loop, and the fused 1x1
        for loop in ('pipe', 'plain', '1x1'):
            assert ('fp16', '3x3', (rw, loop, 1)) in seen, (rw, loop)
    for k in (('fp32', '3x3', (4, 'pipe', 1)), ('fp32', '3x3', (4, 'plain', 1)), ('fp32', '3x3', (4, '1x1', 1))):
        assert k in seen
    for p in ('fp16', 'fp32'):
        for kind in ('1x1', 'ups', 'sub'):
            assert {(p, kind, 'one'), (p, kind, 'two')} <= seen
        assert {(p, 's2', 'wide'), (p, 's2', 'plain')} <= seen
    # every family is launched in both precisions, and the PACK branch on a far family
    fams = {(c[1], f) for c in T.CONV_CASES for f in c[11]}
    assert fams == {(p, f) for p in ('fp16', 'fp32') for f in FV.FAMILIES}
    assert any(c[12] == 'ksplit' and 'group' in c[11] for c in T.CONV_CASES)
    used = {k for c in T.CONV_CASES for k in c[9]} | {c[12] for c in T.CONV_CASES}
    assert {'res1', 'res2', 'aux', 'z1', 'bwd3'} <= used


def test_relocate_rewrites_views_without_a_device():
    """relocate on 'meta' buffers (no arena): pointers, strides and the group / row / batch decomposition"""
    from esrganplus_amd import engine as E, _lib as L
    g = E.G32(3, 64, 13, 40, 'fp16', 'meta')
    base = 0x7f00_0000_0000

    class T_:
        def __init__(self, n):
            self.n = n

        def data_ptr(self):
            return base

        def numel(self):
            return self.n

        def element_size(self):
            return 1
    g.t = T_(g.B * g.bs)
    c = L.esr_conv()
    v = L.esr_g32()
    v.ptr, v.batch_stride, v.group_stride, v.wp, v.ngroups = base + 2 * g.gs + 5 * g.Wp * 32, g.bs, g.gs, g.Wp, 2
    c.in_ = v
    for fam in ('batch', 'group'):
        rel = FV.relocate(c, [g], fam, None)
        fb = rel.fbs[0]
        assert fb.ng == 4
        w = rel.op.in_
        assert (w.batch_stride, w.group_stride, w.wp, w.ngroups) == (fb.bs, fb.gs, fb.wp, 2)
        assert w.ptr == FV.PTR_OFF + fb.base + 2 * fb.gs + 5 * fb.wp * 32
        assert not rel.op.out.ptr
    with pytest.raises(FV.Unfit):
        FV.relocate(c, [g], 'plane', None)


def test_banded_trunk_buffers_take_the_image_limit():
    """The banded chain keeps the tall buffer's group stride in its band views, and the chain kernels reach the four
    groups of a band through 32-bit offsets: a tall, narrow fp16 image whose planes pass the plane check but whose four
    planes pass 2^31 bytes is refused before anything is allocated (device 'meta': nothing could be).  A 4100 x 4100
    image is too wide for bands at all (its trunk runs per conv, plane by plane) and is not refused."""
    from esrganplus_amd import engine as E
    H, W = 16000, 2720
    geom = E.rdb_band_geometry(H, W)
    assert geom is not None
    S, m, n = geom
    E.G32(1, 64, n * S + 2 * m, W, 'fp16', 'meta')                     # the plane check alone lets it through
    with pytest.raises(ValueError, match='32-bit offsets'):
        E.band_buffers(1, geom, W, 'fp16', 'meta')
    tall, mid, dense = E.band_buffers(1, E.rdb_band_geometry(339, 510), 510, 'fp16', 'meta')
    assert tall[0].t.device.type == 'meta'
    assert E.rdb_band_geometry(4100, 4100) is None
    E.G32(1, 192, 4100, 4100, 'fp16', 'meta')


def test_engine_limits_are_never_looser_than_the_abi():
    """A buffer the engine accepts under its per-image rule passes the chain's and the dense-block weight gradients'
    host-side checks; one they refuse, the engine refuses.  (The conv and per-conv weight-gradient launchers state the
    same sums — plane < 2^31, image < 2^31 — and are exercised on the GPU.)"""
    from esrganplus_amd import engine as E, _lib as L
    lib = L.lib()
    fake = 0x7f00_0000_0000

    def chain_ok(buf, H):
        ch = L.esr_rdb_chain()
        ch.dtype, ch.B, ch.H, ch.W, ch.n_blocks, ch.mode = buf.esr_dtype, 1, H, buf.W, 1, 0
        blocks = (L.esr_rdb_block * 1)()
        for name in ('x_in', 'x_out', 'res2'):
            v = getattr(blocks[0], name)
            v.ptr, v.batch_stride, v.group_stride, v.wp, v.ngroups = fake, buf.bs, buf.gs, buf.Wp, buf.ng
        return lib.esr_rdb_chain_check(C.byref(ch), C.addressof(blocks)) == 0
    for prec, cpg in (('fp16', 16), ('fp32', 8)):
        ng = 64 // cpg
        for W in (40, 2720):
            Wp = FV.g32_dims(1, W)[1]
            # heights around the one where ng planes reach 2^31 bytes
            h_lim = (1 << 31) // (ng * Wp * 32)
            for H in (h_lim - 70, h_lim - 38, h_lim - 6, h_lim + 26, h_lim + 58):
                try:
                    buf = E.G32(1, 64, H, W, prec, 'meta', image_limit=True)
                    accepted = True
                except ValueError:
                    buf, accepted = E.G32(1, 64, H, W, prec, 'meta'), False
                abi = chain_ok(buf, H)
                assert abi or not accepted, (prec, W, H)
                assert accepted == (buf.ng * buf.gs < 1 << 31)
                assert abi == accepted, (prec, W, H)          # the same sum on both sides
    # the dense-block weight gradients: an image past 2^32 - 16 bytes, or outside batch_stride
    rw = L.esr_rdb_wgrad()
    rw.dtype, rw.B, rw.H, rw.W, rw.n_blocks = L.ESR_F16, 1, 16, 32, 1
    wb = (L.esr_rdb_wgrad_block * 1)()
    gs = 38 * 34 * 32
    for v, n in ((wb[0].in_, 12), (wb[0].q, 14)):
        v.ptr, v.batch_stride, v.group_stride, v.wp, v.ngroups = fake, n * gs, gs, 34, n
    assert lib.esr_rdb_wgrad_check(C.byref(rw), C.addressof(wb)) == 0, lib.esr_last_error()
    wb[0].q.batch_stride = 13 * gs
    assert lib.esr_rdb_wgrad_check(C.byref(rw), C.addressof(wb)) == -3
    assert b'batch_stride' in lib.esr_last_error()
    wb[0].q.batch_stride = 14 * gs
    wb[0].in_.group_stride, wb[0].in_.batch_stride = FV.FAR, 12 * FV.FAR
    assert lib.esr_rdb_wgrad_check(C.byref(rw), C.addressof(wb)) == -3 and b'2^32' in lib.esr_last_error()


class _StubPack:
    """what Builder reads of a WeightPack — the convs' names and shapes — without a device"""

    class Ent:
        def __init__(self, w):
            self.cout, self.cin, self.ks = int(w.shape[0]), int(w.shape[1]), int(w.shape[2])
            self.w_ptr = self.bias_ptr = 0x1000
            self.subpix = False

    def __init__(self, net):
        self.entries = {k[:-7]: self.Ent(v) for k, v in net.state_dict().items() if k.endswith('.weight') and v.dim() == 4}


def _x1_plan(H, W):
    from esrganplus_amd import architecture as arch, engine as E
    net = arch.RRDBNet(3, 3, 64, 1, upscale=1).eval().set_precision('fp16')
    bld = E.Builder(_StubPack(net), 1, H, W, 'fp16', torch.device('meta'), False, net.variant, 'net', 1, scale=1)
    return bld.rrdbnet(3, 3, False)


def test_x1_plans_of_huge_images_on_meta():
    """The whole fp16 RRDBNet(3, 3, 64, 1, upscale=1) plan on device 'meta' (nothing can be allocated).  1 x 3 x 4100 x 4100:
    too wide for bands, so the trunk is per-conv launches — no chain op, every plane below 2^31 — which the kernels
    address correctly, and the plan builds.  1 x 3 x 16000 x 2720: the banded trunk, whose four tall planes pass 2^31:
    the ValueError about 32-bit offsets, before allocation."""
    from esrganplus_amd import engine as E, _lib as L
    P = _x1_plan(4100, 4100)
    assert not P.chain_ops and all(o.kind != L.OP_RDB_CHAIN for o in P.ops.ops)
    g = [b for b in P.bufs if isinstance(b, E.G32)]
    assert g and all(b.t.device.type == 'meta' and b.gs < 1 << 31 for b in g) and max(b.bs for b in g) > 1 << 32
    with pytest.raises(ValueError, match='32-bit offsets'):
        _x1_plan(16000, 2720)
