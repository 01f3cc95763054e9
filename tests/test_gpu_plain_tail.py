"""The PLAIN instantiations of conv_kernel (csrc/conv_plain.h): fp16 forward layers that are bias + activation into one
output run a kernel that holds nothing but that epilogue.  Every case runs the op twice through the C ABI: once with
debug_flags 512, which makes the library refuse the call unless it goes to a plain kernel, and once with a store
flavour (debug_flags 8: non-temporal stores, same values), which keeps it on the general kernel.  The two results must
be equal bit for bit, sentinels included, and the plain one within test_gpu_conv_forward's gate of the float64
reference (fp16: 6e-4 of the reference's largest magnitude, G32 and NCHW alike; worst measured on an MI355X: 4.1e-4
into G32, 4.8e-7 into fp32 NCHW).

Shapes: whole 16x32 tiles with seams, ragged maps, each activation, an odd third cout block, NCHW outputs of 1, 3 and
16 channels with sentinel floats behind them, the sub-pixel up-conv on whole and ragged input tiles and with an odd
cout block.  At batch 2 the 3x3 dispatch takes 4-row tiles; the same shapes run with debug_flags 256 | 64 on the
16-row tiles and the plain K loop of the x4 forward's tail, and two larger batches reach its two-cout-blocks-per-wave
kernel.  The first test pins that, without a GPU."""
import pytest
import torch

from tests.test_gpu_conv_backward import conv3_branch
from tests.test_gpu_conv_forward import SENT, TOL, Fwd, _mods, cdiv, dev, rel_err, run  # noqa: F401

PLAIN, GENERAL = 512, 8         # esr_conv.debug_flags: refuse unless plain / a store flavour keeps the general kernel
T16 = 256 | 64                  # 16-row tiles, plain K loop: the geometry of the 512^2 tail at these small sizes

G32 = dict(act='lrelu')
# name, B, cin, cout, kind, H, W (the OUTPUT map), debug_flags, spec
CASES = []
for tag, fl in (('', 0), ('_t16', T16)):
    CASES += [
        ('pt_whole' + tag, 2, 64, 64, '3x3', 32, 64, fl, G32),                    # 2 x 2 whole tiles: seams
        ('pt_ragged' + tag, 2, 64, 64, '3x3', 24, 40, fl, G32),                   # ragged in both directions
        ('pt_none' + tag, 2, 64, 64, '3x3', 16, 32, fl, dict(act='none')),
        ('pt_relu' + tag, 2, 64, 64, '3x3', 16, 32, fl, dict(act='relu')),
        ('pt_c96' + tag, 2, 64, 96, '3x3', 24, 40, fl, G32),                      # odd third cout block
        ('pt_nchw3_whole' + tag, 2, 64, 3, '3x3', 32, 64, fl, dict(act='none', out=False, nchw=3)),
        ('pt_nchw3_ragged' + tag, 2, 64, 3, '3x3', 24, 40, fl, dict(act='lrelu', out=False, nchw=3)),
        ('pt_nchw1' + tag, 2, 64, 1, '3x3', 24, 40, fl, dict(act='relu', out=False, nchw=1)),
        ('pt_nchw16' + tag, 2, 64, 16, '3x3', 24, 40, fl, dict(act='none', out=False, nchw=16)),
    ]
CASES += [
    # two cout blocks per wave (>= 256 workgroups of a pair): whole tiles, and a wave with nothing to compute next to one
    # with a full pair on a ragged map; NCHW past one half-wave and past one cout block
    ('pt_whole_pair', 64, 64, 64, '3x3', 32, 64, 256, G32),
    ('pt_c96_pair', 32, 64, 96, '3x3', 24, 40, 256, G32),
    ('pt_nchw35_pair', 64, 64, 40, '3x3', 24, 40, 256, dict(act='lrelu', out=False, nchw=35)),
    ('pt_sub_whole', 2, 64, 64, 'sub', 32, 64, 0, G32),                           # input 16 x 32: whole 8 x 32 tiles
    ('pt_sub_ragged', 2, 64, 64, 'sub', 24, 80, 0, G32),                          # input 12 x 40: a short last row group
    ('pt_sub_c96', 2, 64, 96, 'sub', 24, 80, 0, G32),
    ('pt_sub_none', 2, 64, 64, 'sub', 24, 80, 0, dict(act='none')),
]


def branch(c):
    name, B, cin, cout, kind, H, W, fl, spec = c
    return conv3_branch('fp16', B, H, W, cdiv(cout, 32), fl) if kind == '3x3' else ('sub', cdiv(cout, 32))


def test_cases_reach_the_tail_kernels():
    """which 3x3 instantiation each case reaches (the dispatch restated in test_gpu_conv_backward.conv3_branch): 4-row
    tiles at batch 2, and the three kernels of the x4 forward's tail — 16-row tiles with the plain K loop, one cout block
    (HR_conv1), one of two (small grids) and two per wave with an even and an odd number of cout blocks"""
    seen = {(branch(c), cdiv(c[3], 32), bool(c[8].get('nchw'))) for c in CASES}
    for k in (((1, 'pipe', 1), 1, True), ((1, 'plain', 1), 2, False), ((1, 'plain', 1), 3, False),
              ((4, 'plain', 1), 1, True), ((4, 'plain', 1), 2, False), ((4, 'plain', 1), 3, False),
              ((4, 'plain', 2), 2, False), ((4, 'plain', 2), 3, False), ((4, 'plain', 2), 2, True),
              (('sub', 2), 2, False), (('sub', 3), 3, False)):
        assert k in seen, k
    # whole-tile maps of more than one tile and maps ragged in both directions, for both kinds
    for kind, th in (('3x3', 16), ('sub', 16)):         # the sub-pixel tile is 8 x 32 of INPUT = 16 x 64 of output
        tw = 32 if kind == '3x3' else 64
        cs = [c for c in CASES if c[4] == kind]
        assert any(c[5] % th == 0 and c[6] % tw == 0 and c[5] > th for c in cs), kind
        assert any(c[5] % th and c[6] % tw for c in cs), kind
    assert {c[8]['act'] for c in CASES if not c[8].get('nchw')} == {'lrelu', 'relu', 'none'}
    assert {c[8]['act'] for c in CASES if c[8].get('nchw')} == {'lrelu', 'relu', 'none'}
    assert {c[8]['nchw'] for c in CASES if c[8].get('nchw')} >= {1, 3, 16}


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_plain_kernel_equals_general_kernel(dev, case):
    name, B, cin, cout, kind, H, W, fl, spec = case
    f = Fwd(dev, name, 'fp16', B, cin, cout, kind, H, W, fl | PLAIN, spec)
    res = f.run()                                       # raises if the dispatch does not take a plain kernel
    e = f.check(res)
    print('plain %s: err/scale %.2e (gate %.1e)' % (name, e, TOL['fp16']))
    g = Fwd(dev, name, 'fp16', B, cin, cout, kind, H, W, fl | GENERAL, spec)
    ref = g.run()
    g.check(ref)
    assert res.keys() == ref.keys()
    for k in res:
        assert torch.equal(bits(res[k]), bits(ref[k])), '%s %s: plain and general kernels differ' % (name, k)


@pytest.mark.gpu
def test_flag_512_refuses_what_is_not_plain(dev):
    """the routing assertion above is not vacuous: a residual, a second output, an fp32 layer, a store flavour and a
    split-K layer are refused under debug_flags 512, and the outputs keep their sentinel"""
    E, L = _mods()
    for what, prec, kind, shape, fl, spec in (
            ('res1', 'fp16', '3x3', (2, 64, 64, 24, 40), 0, dict(act='lrelu', res1=(0.2, None))),
            ('aux', 'fp16', '3x3', (2, 64, 64, 24, 40), 0, dict(act='lrelu', aux=32)),
            ('g32 and nchw', 'fp16', '3x3', (2, 64, 3, 24, 40), 0, dict(act='none', nchw=3)),
            ('alpha', 'fp16', '3x3', (2, 64, 64, 24, 40), 0, dict(act='lrelu', alpha=0.5)),
            ('fp32', 'fp32', '3x3', (2, 64, 64, 24, 40), 0, dict(act='lrelu')),
            ('fp32 sub', 'fp32', 'sub', (2, 64, 64, 24, 80), 0, dict(act='lrelu')),
            ('flavour', 'fp16', '3x3', (2, 64, 64, 24, 40), GENERAL, dict(act='lrelu'))):
        B, cin, cout, H, W = shape
        f = Fwd(dev, 'pt_refuse ' + what, prec, B, cin, cout, kind, H, W, fl | PLAIN, spec)
        ops = L.OpList()
        ops.add_conv(f.c)
        with pytest.raises(L.HipExtensionError):
            ops.run(E.current_stream())
        torch.cuda.synchronize()
        for nm, buf, *_ in f.checks:
            assert (buf.t.float().cpu() == SENT).all(), (what, nm)


def is_plain(c, L):
    """launch()'s host test of csrc/conv_mfma.hip on a recorded op"""
    one_out = bool(c.out.ptr) != (c.nchw_out_c > 0)
    return (c.dtype == 0 and not c.w1x1 and not c.res1.ptr and not c.res2.ptr and not c.aux_out.ptr and not c.mask.ptr and
            not c.out3.ptr and c.noise_mode == L.NOISE_OFF and c.alpha == 1.0 and one_out and c.ksplit <= 1 and
            not (c.debug_flags & 0x18))


@pytest.mark.gpu
def test_x4_forward_plain_equals_general(dev, monkeypatch):
    """RRDBNet x4 (nb = 1, fp16, 1 x 3 x 16 x 32 LR) through its launch plan: with the store flavour on every conv
    (ESR_DBG=8: general kernels) and as dispatched.  The plan's convs on the 2x and 4x maps — the two up-convs, HR_conv0,
    HR_conv1 — are plain (the head conv also stores the trunk's shortcut, LR_conv adds it: general); flagged 512 the
    library confirms it, and the output is the same bits."""
    from esrganplus_amd import architecture as arch, synth
    _, L = _mods()
    sd = synth.rrdbnet_state_dict(nb=1, seed=5)
    x = synth.image_batch(5, 1, 3, 16, 32, name='plain_tail.x').to(dev)
    out = {}
    for flag in ('8', '0'):
        monkeypatch.setenv('ESR_DBG', flag)
        net = arch.RRDBNet(3, 3, 64, 1).to(dev).eval().set_precision('fp16')
        net.load_state_dict(sd, strict=True)
        with torch.no_grad():
            out[flag] = net(x).float().cpu()
    assert torch.isfinite(out['0']).all() and out['0'].shape == (1, 3, 64, 128)
    assert torch.equal(bits(out['0']), bits(out['8']))
    plan = next(iter(net._plans.values()))
    convs = [o.u.conv for o in plan.ops.ops if o.kind == L.OP_CONV]
    tail = [c for c in convs if c.H > 16]
    assert len(tail) == 4 and all(is_plain(c, L) for c in tail)
    for o in plan.ops.ops:
        if o.kind == L.OP_CONV and is_plain(o.u.conv, L):
            o.u.conv.debug_flags |= PLAIN
    plan.ops._arr = None
    plan.ops.drop_graph()
    with torch.no_grad():
        again = net(x).float().cpu()
    assert torch.equal(bits(again), bits(out['0']))
