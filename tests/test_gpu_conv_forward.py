"""The forward convolution outside the fused RDB chain (esr_conv_forward: conv_kernel<..., BWD=false> and the
instantiations launch() routes a forward op to), op by op through the C ABI.  Every result is compared with float64
torch on the CPU, on the values the kernel actually reads: fp16 activations, weights, residuals and explicit z
rounded to fp16, the bias in fp32, and for the sub-pixel up-conv the pre-summed taps rounded to the storage type.

The first section restates the dispatch heuristics and the epilogue routing of csrc/conv_mfma.hip in Python and pins
which case reaches which branch, so a later change that drops one fails there instead of silently narrowing the test.
Those pins, and the check of the sub-pixel reference against nearest-x2 + 3x3, run without a GPU.  The GPU sections
run every branch (ragged maps, a short last tile, cin 3, cout 3, a ragged third cout block, a 1x1-pixel image; off
the recipe: cin 1 and 2, a second input group of one channel, cout 1 and 20, nchw_out_c = 1), every
epilogue stage alone and combined in the order esrgan_hip.h documents, in-place and in-slice stores, partial views,
Philox noise against its explicit form, and the refusals.  Every G32 output is pre-filled with a sentinel: the zero
ring, the rows and columns past the map, the groups past the view and the padding lanes must hold what they held.

Error bounds are relative to the reference's largest magnitude.  fp32: 4e-6, the backward file's gate.  fp16: every
stage runs in fp32 on exact fp16 operands (an fp16 conv storing fp32 NCHW is within 3e-7), so the error is the
round-to-nearest of the stored result, at most 2^-11 = 4.9e-4 of the scale, plus fp32 round-off: 6e-4, tighter
than the backward file's 1.5e-3.  Worst measured on an MI355X: fp32 9.7e-7, fp16 4.5e-4; on the off-recipe channel
counts alone fp32 6.0e-7 (cout 20), fp16 3.9e-4 (cout 1)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.pack_refs import subpix_conv, subpix_taps      # esr_pack.ups_fwd's pre-summed taps, shared with the pack tests
from tests.test_gpu_conv_backward import (SENT, SLOPE, _mods, cdiv, check_buffer, conv3_branch, dev, g32, q,  # noqa: F401
                                          rel_err, rnd, run, s2_branch, upload)

TOL = {'fp32': 4e-6, 'fp16': 6e-4}
SIGMA = 0.1                     # esr_conv.sigma as engine._conv sets it
TAIL = 4096                     # sentinel floats past an fp32 NCHW output
KS = {'3x3': 3, '1x1': 1, 'ups': 3, 'sub': 3, 's2': 4}


def f32(v):
    """a scalar as the kernel holds it (fp32)"""
    return float(np.float32(v))


def in_map(kind, H, W):
    """input map of a conv whose OUTPUT is H x W"""
    return {'ups': (H // 2, W // 2), 'sub': (H // 2, W // 2), 's2': (2 * H, 2 * W)}.get(kind, (H, W))


# ----------------------------------------------------------------------------------------------------------------
# 1. dispatch pins (CPU arithmetic only)
# ----------------------------------------------------------------------------------------------------------------

def fwd_branch(prec, B, H, W, cout, kind, flags=0, n1x1=0):
    """dispatch<T> of csrc/conv_mfma.hip for a forward op (H x W: the output map)"""
    cbk = cdiv(cout, 32)
    if kind == '3x3':
        rw, loop, ncw = conv3_branch(prec, B, H, W, cbk, flags)
        return rw, '1x1' if n1x1 else loop, ncw
    if kind == 's2':
        return s2_branch(W, cbk)
    return 'one' if cbk == 1 else 'two'                # 1x1, nearest-x2 gather, sub-pixel


def epi_route(prec, cout, spec):
    """which epilogue a forward op runs: launch() picks the BWD instantiation for alpha != 1 without res1 and for a
    residual view narrower than both the cout blocks and `out`; epilogue_block<BWD=false, HAS1X1=false> then takes its
    straight-line path for bias + act into `out` alone or `nchw_out` alone"""
    cpg, gpb = (16, 2) if prec == 'fp16' else (8, 4)
    cbk = cdiv(cout, 32)
    out_ng = 0 if spec.get('out', True) is False else spec.get('out_ng', cdiv(cout, cpg))
    r1, r2 = spec.get('res1'), spec.get('res2')

    def narrow(r):
        if r is None:
            return False
        ng = r[1] if r[1] is not None else cdiv(cout, cpg)
        return ng < cbk * gpb and ng < out_ng
    if (r1 is None and spec.get('alpha', 1.0) != 1.0) or narrow(r1) or narrow(r2):
        return 'bwd'
    if spec.get('w1x1'):
        return 'general'
    nchw = spec.get('nchw', 0)
    plain = r1 is None and r2 is None and spec.get('aux') is None and 'z1' not in spec and 'z2' not in spec
    if plain and out_ng and not nchw:
        return 'fast_g32'
    if plain and not out_ng and nchw:
        return 'fast_nchw'
    return 'general'


# branch cases: name, prec, B, cin, cout, kind, H, W (the OUTPUT map), debug_flags, act, expected branch
BR_CASES = [
    ('f16_r1_pipe', 'fp16', 2, 40, 24, '3x3', 13, 40, 0, 'lrelu', (1, 'pipe', 1)),
    ('f16_r1_plain', 'fp16', 3, 32, 72, '3x3', 13, 40, 0, 'relu', (1, 'plain', 1)),      # ragged third cout block
    ('f16_r1_h4clamp', 'fp16', 100, 32, 16, '3x3', 3, 64, 0, 'none', (1, 'pipe', 1)),
    ('f16_r1_cin3', 'fp16', 2, 3, 64, '3x3', 34, 36, 0, 'lrelu', (1, 'plain', 1)),
    ('f16_r1_cout3', 'fp16', 3, 32, 3, '3x3', 10, 40, 0, 'lrelu', (1, 'pipe', 1)),
    ('f16_r1_1px', 'fp16', 3, 32, 40, '3x3', 1, 1, 0, 'lrelu', (1, 'plain', 1)),
    ('f16_r2_pipe', 'fp16', 40, 32, 16, '3x3', 20, 40, 0, 'lrelu', (2, 'pipe', 1)),
    ('f16_r2_plain', 'fp16', 20, 48, 64, '3x3', 20, 40, 0, 'relu', (2, 'plain', 1)),
    ('f16_r2_h8clamp', 'fp16', 49, 32, 128, '3x3', 6, 64, 0, 'lrelu', (2, 'plain', 1)),
    ('f16_r4_plain_grid', 'fp16', 97, 16, 32, '3x3', 17, 33, 0, 'lrelu', (4, 'plain', 1)),
    ('f16_r4_pipe_flag', 'fp16', 2, 24, 32, '3x3', 20, 40, 256, 'lrelu', (4, 'pipe', 1)),
    ('f16_r4_plain_flag', 'fp16', 2, 24, 32, '3x3', 20, 40, 256 | 64, 'none', (4, 'plain', 1)),
    ('f16_r4_ncw1', 'fp16', 3, 72, 72, '3x3', 18, 33, 256, 'lrelu', (4, 'plain', 1)),
    ('f16_r4_ncw2', 'fp16', 16, 32, 256, '3x3', 17, 33, 0, 'lrelu', (4, 'plain', 2)),
    ('f32_pipe', 'fp32', 2, 24, 24, '3x3', 13, 40, 0, 'lrelu', (4, 'pipe', 1)),
    ('f32_pipe_flag', 'fp32', 97, 16, 32, '3x3', 17, 33, 128, 'relu', (4, 'pipe', 1)),
    ('f32_plain_flag', 'fp32', 2, 24, 24, '3x3', 13, 40, 64, 'none', (4, 'plain', 1)),
    ('f32_plain_grid', 'fp32', 97, 16, 32, '3x3', 17, 33, 0, 'lrelu', (4, 'plain', 1)),
    ('f32_ncw1', 'fp32', 3, 72, 72, '3x3', 18, 33, 0, 'lrelu', (4, 'plain', 1)),
    ('f32_ncw2', 'fp32', 16, 32, 256, '3x3', 17, 33, 0, 'lrelu', (4, 'plain', 2)),
    ('f32_cin3', 'fp32', 2, 3, 64, '3x3', 34, 36, 0, 'lrelu', (4, 'plain', 1)),
    ('f32_1px', 'fp32', 3, 32, 40, '3x3', 1, 1, 0, 'lrelu', (4, 'plain', 1)),
    # off-recipe channel counts: one and two channels in a group, a second group of ONE channel (17 fp16, 9 fp32),
    # one output channel, 20 output channels (a ragged second fp16 group / third fp32 group)
    ('f16_cin1', 'fp16', 2, 1, 64, '3x3', 13, 40, 0, 'lrelu', (1, 'plain', 1)),
    ('f16_cin2', 'fp16', 2, 2, 24, '3x3', 13, 40, 0, 'lrelu', (1, 'pipe', 1)),
    ('f16_cin17', 'fp16', 2, 17, 40, '3x3', 13, 40, 0, 'lrelu', (1, 'plain', 1)),
    ('f16_cout1', 'fp16', 2, 32, 1, '3x3', 13, 40, 0, 'lrelu', (1, 'pipe', 1)),
    ('f16_cout20', 'fp16', 2, 40, 20, '3x3', 13, 40, 0, 'none', (1, 'pipe', 1)),
    ('f16_cin1_r4', 'fp16', 2, 1, 64, '3x3', 13, 40, 256, 'lrelu', (4, 'plain', 1)),
    ('f32_cin1', 'fp32', 2, 1, 64, '3x3', 13, 40, 0, 'lrelu', (4, 'plain', 1)),
    ('f32_cin2', 'fp32', 2, 2, 24, '3x3', 13, 40, 0, 'lrelu', (4, 'pipe', 1)),
    ('f32_cin9', 'fp32', 2, 9, 40, '3x3', 13, 40, 0, 'lrelu', (4, 'plain', 1)),
    ('f32_cout1', 'fp32', 2, 32, 1, '3x3', 13, 40, 0, 'lrelu', (4, 'pipe', 1)),
    ('f32_cout20', 'fp32', 2, 40, 20, '3x3', 13, 40, 0, 'none', (4, 'pipe', 1)),
    ('f16_ups_one', 'fp16', 3, 24, 32, 'ups', 26, 40, 0, 'lrelu', 'one'),
    ('f16_ups_two', 'fp16', 2, 32, 72, 'ups', 18, 70, 0, 'lrelu', 'two'),
    ('f16_ups_1px', 'fp16', 2, 32, 40, 'ups', 2, 2, 0, 'lrelu', 'two'),
    ('f32_ups_one', 'fp32', 3, 24, 3, 'ups', 26, 40, 0, 'relu', 'one'),
    ('f32_ups_two', 'fp32', 2, 32, 72, 'ups', 18, 70, 0, 'lrelu', 'two'),
    ('f16_sub_one', 'fp16', 3, 24, 32, 'sub', 26, 70, 0, 'lrelu', 'one'),
    ('f16_sub_two', 'fp16', 2, 3, 72, 'sub', 18, 40, 0, 'lrelu', 'two'),
    ('f16_sub_1px', 'fp16', 2, 32, 40, 'sub', 2, 2, 0, 'none', 'two'),
    ('f32_sub_one', 'fp32', 3, 24, 3, 'sub', 26, 70, 0, 'lrelu', 'one'),
    ('f32_sub_two', 'fp32', 2, 32, 72, 'sub', 18, 40, 0, 'relu', 'two'),
    ('f16_s2_wide', 'fp16', 3, 24, 48, 's2', 9, 34, 0, 'lrelu', 'wide'),
    ('f16_s2_plain', 'fp16', 2, 32, 72, 's2', 9, 20, 0, 'lrelu', 'plain'),
    ('f16_s2_1px', 'fp16', 2, 32, 3, 's2', 1, 1, 0, 'lrelu', 'plain'),
    ('f32_s2_wide', 'fp32', 3, 24, 48, 's2', 9, 34, 0, 'relu', 'wide'),
    ('f32_s2_plain', 'fp32', 2, 32, 72, 's2', 9, 70, 0, 'lrelu', 'plain'),
    ('f16_1x1_one', 'fp16', 3, 24, 32, '1x1', 11, 40, 0, 'lrelu', 'one'),
    ('f16_1x1_two', 'fp16', 2, 48, 72, '1x1', 11, 40, 0, 'none', 'two'),
    ('f16_1x1_1px', 'fp16', 2, 3, 3, '1x1', 1, 1, 0, 'lrelu', 'one'),
    ('f32_1x1_one', 'fp32', 3, 24, 32, '1x1', 11, 40, 0, 'relu', 'one'),
    ('f32_1x1_two', 'fp32', 2, 48, 72, '1x1', 11, 40, 0, 'lrelu', 'two'),
]

# epilogue cases: name, prec, B, cin, cout, H, W, debug_flags, spec (3x3 convs).  spec keys: act; w1x1 (input
# channels of the fused 1x1); aux (channel offset of the aux_out view in a wider buffer); res1 / res2 ((alpha or beta,
# view groups or None)); alpha / beta (without res1 / res2); z1 / z2 (explicit z: view groups or None); nchw (nchw_out_c);
# out (False: no G32 output); out_ng (groups of the out view)
EPI_CASES = [
    ('f16_1x1_r1', 'fp16', 2, 96, 32, 13, 40, 0, dict(act='lrelu', w1x1=64, aux=32), 'general'),
    ('f16_1x1_r2', 'fp16', 40, 96, 32, 20, 40, 0, dict(act='lrelu', w1x1=64, aux=32), 'general'),
    ('f16_1x1_r4', 'fp16', 2, 96, 32, 13, 40, 256, dict(act='lrelu', w1x1=64, aux=32), 'general'),
    ('f16_1x1_r4_grid', 'fp16', 97, 96, 24, 17, 33, 0, dict(act='lrelu', w1x1=64), 'general'),
    ('f16_1x1_full', 'fp16', 3, 64, 32, 13, 40, 0, dict(act='lrelu', w1x1=64, aux=32), 'general'),
    ('f32_1x1', 'fp32', 2, 96, 32, 13, 40, 0, dict(act='lrelu', w1x1=64, aux=32), 'general'),
    ('f32_1x1_full', 'fp32', 3, 64, 24, 13, 40, 0, dict(act='lrelu', w1x1=64, aux=32), 'general'),
    ('f16_aux_plain', 'fp16', 2, 32, 64, 13, 40, 0, dict(act='lrelu', aux=32), 'general'),
    ('f16_res1_relu', 'fp16', 2, 32, 72, 13, 40, 0, dict(act='relu', res1=(0.2, None)), 'general'),
    ('f16_res12_lrelu', 'fp16', 3, 40, 72, 13, 40, 0, dict(act='lrelu', res1=(0.2, None), res2=(0.7, None)), 'general'),
    ('f32_res12_none', 'fp32', 2, 40, 72, 13, 40, 0, dict(act='none', res1=(0.2, None), res2=(0.7, None)), 'general'),
    ('f32_res2_relu', 'fp32', 2, 32, 40, 13, 40, 0, dict(act='relu', res2=(0.7, None)), 'general'),
    ('f16_alpha_only', 'fp16', 2, 32, 72, 13, 40, 0, dict(act='lrelu', alpha=0.5), 'bwd'),
    ('f32_alpha_only', 'fp32', 2, 32, 40, 13, 40, 0, dict(act='none', alpha=0.5, beta=0.25), 'bwd'),
    ('f16_beta_only', 'fp16', 2, 32, 40, 13, 40, 0, dict(act='lrelu', beta=0.25, z1=None), 'general'),
    ('f16_z1', 'fp16', 2, 32, 72, 13, 40, 0, dict(act='lrelu', z1=None), 'general'),
    ('f16_z2', 'fp16', 2, 32, 72, 13, 40, 0, dict(act='lrelu', z2=None), 'general'),
    ('f16_z12', 'fp16', 2, 32, 72, 13, 40, 0, dict(act='none', z1=None, z2=None), 'general'),
    ('f32_z12', 'fp32', 2, 32, 40, 13, 40, 0, dict(act='lrelu', z1=None, z2=None), 'general'),
    ('f16_all', 'fp16', 2, 96, 32, 13, 40, 0,
     dict(act='lrelu', w1x1=64, aux=32, res1=(0.2, None), z1=None, res2=(0.7, None), z2=None, nchw=20), 'general'),
    ('f32_all', 'fp32', 2, 96, 32, 13, 40, 0,
     dict(act='lrelu', w1x1=64, aux=32, res1=(0.2, None), z1=None, res2=(0.7, None), z2=None, nchw=20), 'general'),
    ('f16_partial', 'fp16', 2, 32, 64, 13, 40, 0,
     dict(act='lrelu', res1=(0.2, 3), res2=(0.7, 2), z1=1, z2=3), 'bwd'),
    ('f32_partial', 'fp32', 2, 32, 64, 13, 40, 0, dict(act='none', res1=(1.0, 5), z2=6), 'bwd'),
    ('f16_out_narrow', 'fp16', 2, 32, 64, 13, 40, 0, dict(act='lrelu', res1=(0.2, 3), out_ng=3), 'general'),
    ('f16_nchw_only', 'fp16', 2, 32, 40, 13, 40, 0, dict(act='lrelu', out=False, nchw=35), 'fast_nchw'),
    ('f32_nchw_only', 'fp32', 3, 32, 40, 13, 40, 0, dict(act='relu', out=False, nchw=35), 'fast_nchw'),
    ('f16_nchw3', 'fp16', 2, 32, 3, 13, 40, 0, dict(act='lrelu', out=False, nchw=3), 'fast_nchw'),
    ('f16_nchw_out', 'fp16', 2, 32, 40, 13, 40, 0, dict(act='lrelu', nchw=35), 'general'),
    ('f32_nchw_res', 'fp32', 2, 32, 72, 13, 40, 0, dict(act='lrelu', res1=(1.0, None), nchw=20), 'general'),
    ('f16_nchw3_res', 'fp16', 2, 32, 3, 13, 40, 0, dict(act='none', res1=(1.0, None), nchw=3), 'general'),
    # nchw_out_c = 1 (a single-channel generator's last conv), alone and next to a G32 output
    ('f16_nchw1', 'fp16', 2, 32, 1, 13, 40, 0, dict(act='lrelu', out=False, nchw=1), 'fast_nchw'),
    ('f32_nchw1', 'fp32', 2, 32, 1, 13, 40, 0, dict(act='none', out=False, nchw=1), 'fast_nchw'),
    ('f16_nchw1_out', 'fp16', 2, 32, 1, 13, 40, 0, dict(act='none', nchw=1), 'general'),
    ('f32_nchw1_out', 'fp32', 2, 32, 1, 13, 40, 0, dict(act='lrelu', nchw=1), 'general'),
]


def epi_branch(c):
    name, prec, B, cin, cout, H, W, flags, spec, _ = c
    return fwd_branch(prec, B, H, W, cout, '3x3', flags, spec.get('w1x1', 0))


def test_forward_cases_reach_every_branch():
    for c in BR_CASES:
        assert fwd_branch(c[1], c[2], c[6], c[7], c[4], c[5], c[8]) == c[10], c[0]
        assert epi_route(c[1], c[4], dict(act=c[9])) == 'fast_g32', c[0]
    seen = {(c[1], c[5], c[10], cdiv(c[4], 32) == 1) for c in BR_CASES}
    seen |= {(c[1], '3x3', epi_branch(c), True) for c in EPI_CASES if c[8].get('w1x1')}
    want = [('fp16', '3x3', (rw, loop, 1), one) for rw in (1, 2) for loop, one in (('pipe', True), ('plain', False))]
    want += [('fp16', '3x3', (rw, '1x1', 1), True) for rw in (1, 2, 4)]
    want += [(p, '3x3', (4, 'pipe', 1), True) for p in ('fp16', 'fp32')]
    want += [(p, '3x3', (4, 'plain', 1), one) for p in ('fp16', 'fp32') for one in (True, False)]
    want += [(p, '3x3', (4, 'plain', 2), False) for p in ('fp16', 'fp32')]
    want += [('fp32', '3x3', (4, '1x1', 1), True)]
    want += [(p, k, b, b == 'one') for p in ('fp16', 'fp32') for k in ('ups', 'sub', '1x1') for b in ('one', 'two')]
    want += [(p, 's2', b, False) for p in ('fp16', 'fp32') for b in ('wide', 'plain')]
    for k in want:
        assert k in seen, k

    def reached(prec, **kw):
        return any(c[1] == prec and all(f(c) for f in kw.values()) for c in BR_CASES if c[5] == '3x3')

    def grid_rw(c):                                    # rows per wave from the grid size alone
        t = cdiv(c[7], 32) * cdiv(c[6], 16) * c[2] * cdiv(c[4], 32)
        return 1 if t <= 128 else (2 if t <= 384 else 4)
    for rw in (1, 2):
        # by grid size, and by the H <= 4 / H <= 8 clamps on a grid that alone would pick larger tiles
        assert reached('fp16', a=lambda c: c[10][0] == rw, b=lambda c: grid_rw(c) == rw, d=lambda c: c[6] > 8)
        assert reached('fp16', a=lambda c: c[10][0] == rw, b=lambda c: grid_rw(c) > rw)
    assert reached('fp16', a=lambda c: c[10][0] == 4, b=lambda c: c[8] == 0)
    assert reached('fp16', a=lambda c: c[10][0] == 4, b=lambda c: c[8] & 256, d=lambda c: grid_rw(c) < 4)
    # fp32 pipelined: by default and by flag 128 on a grid of > 256 tiles; plain: by flag 64 and by > 256 tiles
    assert reached('fp32', a=lambda c: c[10][1] == 'pipe', b=lambda c: c[8] == 0)
    assert reached('fp32', a=lambda c: c[10][1] == 'pipe', b=lambda c: c[8] & 128)
    assert reached('fp32', a=lambda c: c[4] <= 32 and c[10][1] == 'plain', b=lambda c: c[8] & 64)
    assert reached('fp32', a=lambda c: c[4] <= 32 and c[10][1] == 'plain', b=lambda c: c[8] == 0)
    # the fused 1x1 on 1x1-wide reads (n1x1 < cin) and on the whole input
    assert {c[3] == c[8]['w1x1'] for c in EPI_CASES if c[8].get('w1x1')} == {True, False}
    # shapes: ragged maps, cin 3, cout 3, a ragged third cout block, a 1x1-pixel image (per precision)
    for p in ('fp16', 'fp32'):
        cs = [c for c in BR_CASES if c[1] == p]
        assert any(c[6] % 16 and c[7] % 32 and c[6] > 16 and c[7] > 32 for c in cs), p
        assert any(c[3] == 3 for c in cs) and any(c[4] == 3 for c in cs), p
        # off the recipe: cin 1 and 2, cout 1 and 20, and a last input group that holds ONE channel, on 3x3 convs
        cpg = 16 if p == 'fp16' else 8
        for cin in (1, 2, cpg + 1):
            assert any(c[3] == cin and c[5] == '3x3' for c in cs), (p, 'cin', cin)
        for cout in (1, 20):
            assert any(c[4] == cout and c[5] == '3x3' for c in cs), (p, 'cout', cout)
        assert any(cdiv(c[4], 32) == 3 and c[4] % 32 for c in cs), p
        assert any(c[6] == 1 and c[7] == 1 for c in cs), p


def test_epilogue_cases_route_as_pinned():
    for c in EPI_CASES:
        assert epi_route(c[1], c[4], c[8]) == c[9], c[0]
        if c[8].get('w1x1'):
            assert cdiv(c[4], 32) == 1 and c[3] >= c[8]['w1x1'], c[0]
    routes = {c[9] for c in EPI_CASES}
    assert routes == {'general', 'bwd', 'fast_nchw'}
    # the BWD instantiation for alpha without res1, and for residual views narrower than the cout blocks and out;
    # a residual as narrow as `out` stays on the forward path
    assert any(c[9] == 'bwd' and 'alpha' in c[8] and 'res1' not in c[8] for c in EPI_CASES)
    assert any(c[9] == 'bwd' and c[8].get('res1', (1, None))[1] for c in EPI_CASES)
    assert any(c[9] == 'general' and c[8].get('out_ng') and c[8].get('res1', (1, None))[1] for c in EPI_CASES)
    assert epi_route('fp16', 64, dict(res2=(0.2, 3))) == 'bwd'
    # nchw_out below cout, and nchw_out_c = cout = 3, on both paths
    assert any(c[9] == 'fast_nchw' and c[8]['nchw'] == 3 == c[4] for c in EPI_CASES)
    assert any(c[9] == 'general' and c[8].get('nchw') == 3 == c[4] for c in EPI_CASES)
    assert any(c[9] == 'general' and 0 < c[8].get('nchw', 0) < c[4] for c in EPI_CASES)
    assert any(c[9] == 'fast_nchw' and 0 < c[8].get('nchw', 0) < c[4] for c in EPI_CASES)
    # nchw_out_c = cout = 1 on both paths, in both precisions
    for p in ('fp16', 'fp32'):
        for route in ('fast_nchw', 'general'):
            assert any(c[1] == p and c[9] == route and c[8].get('nchw') == 1 == c[4] for c in EPI_CASES), (p, route)
    # activations with the residual stages
    assert {c[8]['act'] for c in EPI_CASES if 'res1' in c[8] or 'res2' in c[8]} == {'relu', 'lrelu', 'none'}


# ----------------------------------------------------------------------------------------------------------------
# references
# ----------------------------------------------------------------------------------------------------------------


def test_subpix_reference_is_nearest_x2_conv3():
    """the sub-pixel restatement the GPU cases use equals nearest-x2 + 3x3 conv in float64"""
    w = rnd((5, 7, 3, 3), 'subpix.w').double()
    x = rnd((2, 7, 5, 6), 'subpix.x').double()
    want = F.conv2d(F.interpolate(x, scale_factor=2, mode='nearest'), w, padding=1)
    got = subpix_conv(x, subpix_taps(w))
    assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item()


def act_ref(v, act):
    if act == 'lrelu':
        return torch.where(v > 0, v, v * SLOPE)
    if act == 'relu':
        return v.clamp_min(0)
    return v


def conv_ref(kind, prec, x, w, b):
    """float64 acc + bias of the stored operands"""
    x = x.double()
    if kind == 'sub':
        y = subpix_conv(x, q(subpix_taps(w.float()), prec).double())
    elif kind == 'ups':
        y = F.conv2d(F.interpolate(x, scale_factor=2, mode='nearest'), w.double(), padding=1)
    else:
        y = F.conv2d(x, w.double(), stride=2 if kind == 's2' else 1, padding=(KS[kind] - 1) // 2)
    return y + b.double()[None, :, None, None]


def cut(t, ng, cpg):
    """a residual / z as a view of ng groups reads it: channels past the view count as zero"""
    if ng is None:
        return t
    t = t.clone()
    t[:, ng * cpg:] = 0
    return t


# ----------------------------------------------------------------------------------------------------------------
# the rig: one forward op on G32 buffers
# ----------------------------------------------------------------------------------------------------------------

ACTS = {'none': 0, 'lrelu': 1, 'relu': 2}
_REFS = {}


class Fwd:
    """the stored operands of one forward conv, its G32 / NCHW outputs pre-filled with the sentinel, the op, and the
    float64 reference of every output on the first and last image"""

    def __init__(self, dev, name, prec, B, cin, cout, kind, H, W, flags, spec):
        E, L = _mods()
        self.name, self.prec, self.B, self.cin, self.cout, self.H, self.W = name, prec, B, cin, cout, H, W
        self.spec, self.idx = spec, [0, B - 1]
        dt, _, cpg = E._dt(prec)
        self.cpg = cpg
        Hi, Wi = in_map(kind, H, W)
        ks = KS[kind]
        n1 = spec.get('w1x1', 0)
        x = q(rnd((B, cin, Hi, Wi), 'fw.x', name), prec)
        w = q(rnd((cout, cin, ks, ks), 'fw.w', name, scale=1.0 / np.sqrt(cin * ks * ks)), prec)
        b = rnd((cout,), 'fw.b', name, scale=0.5)
        convs = [('c', w.to(dev), b.to(dev))]
        if n1:
            w1 = q(rnd((cout, n1, 1, 1), 'fw.w1', name, scale=1.0 / np.sqrt(n1)), prec)
            convs.append(('w1', w1.to(dev), None))
        self.wp = E.WeightPack(convs, prec, dev, ('c',) if kind == 'sub' else ())
        st = E.current_stream()
        self.wp.ensure(st, force=True)
        # input; 'slice': the output is a channel slice of the input buffer, past the cin_groups the K loop reads
        if spec.get('slice'):
            self.xin = g32(dev, prec, B, cin + cdiv(cout, 32) * 32 + 32, Hi, Wi)
            self.xin.t[:, cin // cpg:] = SENT
        else:
            self.xin = g32(dev, prec, B, cin, Hi, Wi)
        upload(self.xin, x)
        kw = {'ups': dict(upsample=1), 'sub': dict(upsample=1), 's2': dict(stride=2)}.get(kind, {})
        c = E._conv(dt, B, H, W, self.xin.view(0, cin), cin, None, self.wp.entries['c'], ACTS[spec.get('act', 'lrelu')],
                    **kw)
        c.debug_flags |= flags
        if n1:
            c.w1x1, c.n1x1_groups = self.wp.entries['w1'].w_ptr, n1 // cpg
        self.c, self.checks, self.bufs = c, [], {}
        idx = self.idx
        # float64 reference, cached per case: v = act(acc + bias); [aux = v]; v += acc_1x1
        if name not in _REFS:
            v = act_ref(conv_ref(kind, prec, x[idx], w, b), spec.get('act', 'lrelu'))
            aux = v
            if n1:
                v = v + F.conv2d(x[idx, :n1].double(), w1.double())
            _REFS[name] = (aux, v)
        aux, v = _REFS[name]
        self.ref_aux = aux

        def operand(key, ng):
            t = q(rnd((B, cout, H, W), 'fw.' + key, name), prec)
            buf = g32(dev, prec, B, cout, H, W)
            upload(buf, t)
            self.bufs[key] = buf
            return buf.view(0, cout) if ng is None else buf.view(0, ng * cpg), cut(t[idx].double(), ng, cpg)

        if 'res1' in spec:
            a, ng = spec['res1']
            c.res1, r1 = operand('res1', ng)
            c.alpha = a
            v = v * f32(a) + r1
        elif 'alpha' in spec:
            c.alpha = spec['alpha']
            v = v * f32(spec['alpha'])
        if 'beta' in spec:                  # beta without res2: ignored
            c.beta = spec['beta']
        zs = []
        for which in ('z1', 'z2'):
            if which in spec:
                view, z = operand(which, spec[which])
                setattr(c, which, view)
                zs.append(z)
                c.noise_mode = L.NOISE_EXPLICIT
            else:
                zs.append(None)
        if zs[0] is not None:
            v = v * (1 + f32(SIGMA) * zs[0])
        if 'res2' in spec:
            bt, ng = spec['res2']
            c.res2, r2 = operand('res2', ng)
            c.beta = bt
            v = v * f32(bt) + r2
        if zs[1] is not None:
            v = v * (1 + f32(SIGMA) * zs[1])
        self.ref_out = v
        # outputs, each with a whole cout block of sentinel groups past its view: a store that ignores the view's
        # ngroups lands there, inside the allocation
        if spec.get('aux') is not None:
            off = spec['aux']
            self.aux = g32(dev, prec, B, off + cdiv(cout, 32) * 32 + 32, H, W, SENT)
            c.aux_out = self.aux.view(off, cout)
            self.checks.append(('aux', self.aux, off, cout, aux))
        if spec.get('slice'):
            c.out = self.xin.view(cin, cout)
            self.checks.append(('out', self.xin, cin, cout, v))
        elif spec.get('out', True) is not False:
            on = min(cout, spec.get('out_ng', cdiv(cout, cpg)) * cpg)
            self.out = g32(dev, prec, B, cdiv(on, 32) * 32 + 32, H, W, SENT)
            c.out = self.out.view(0, on)
            self.checks.append(('out', self.out, 0, on, v[:, :on]))
        self.nchw = None
        if spec.get('nchw'):
            nc = spec['nchw']
            self.nchw = torch.full((B * nc * H * W + TAIL,), SENT, device=dev)
            c.nchw_out_c, c.nchw_out = nc, self.nchw.data_ptr()

    def run(self):
        """run the op; every output as a CPU tensor (G32 buffers whole)"""
        _, L = _mods()
        ops = L.OpList()
        ops.add_conv(self.c)
        run(ops)
        res = {what: buf.t.float().cpu() for what, buf, *_ in self.checks}
        if self.nchw is not None:
            res['nchw'] = self.nchw.cpu()
        return res

    def check(self, res, before=None):
        """every output against the reference; nothing written outside its view. Returns the worst error."""
        worst, idx, H, W = 0.0, self.idx, self.H, self.W
        for what, buf, c0, C_, ref in self.checks:
            t = res[what]
            g0, ng = c0 // self.cpg, cdiv(C_, self.cpg)
            got = t[:, g0:g0 + ng, 1:H + 1, 1:W + 1, :].permute(0, 1, 4, 2, 3).reshape(self.B, ng * self.cpg, H, W)
            e = rel_err(got[idx, :C_], ref)
            assert e <= TOL[self.prec], '%s %s: err/scale %.3e' % (self.name, what, e)
            worst = max(worst, e)
            if c0 == 0 and before is None:
                check_buffer(buf, C_, '%s %s' % (self.name, what))
            else:
                # a view into a wider buffer: only the image pixels of its groups may change
                assert (got[:, C_:] == 0).all(), '%s %s: padding lanes not zero' % (self.name, what)
                old = before[what] if before is not None else torch.full_like(t, SENT)
                keep = torch.ones(t.shape, dtype=torch.bool)
                keep[:, g0:g0 + ng, 1:H + 1, 1:W + 1, :] = False
                assert torch.equal(t[keep], old[keep]), '%s %s: wrote outside its view' % (self.name, what)
        if self.nchw is not None:
            nc, n = self.spec['nchw'], self.B * self.spec['nchw'] * H * W
            got = res['nchw'][:n].reshape(self.B, nc, H, W)
            e = rel_err(got[idx], self.ref_out[:, :nc])
            assert e <= TOL[self.prec], '%s nchw: err/scale %.3e' % (self.name, e)
            assert (res['nchw'][n:] == SENT).all(), '%s: wrote past nchw_out_c channels' % self.name
            worst = max(worst, e)
        return worst


# ----------------------------------------------------------------------------------------------------------------
# 2. every forward branch
# ----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('case', BR_CASES, ids=[c[0] for c in BR_CASES])
def test_branch_matches_fp64(dev, case):
    """bias + activation into one G32 output (the straight-line epilogue) on every dispatch branch; a second run
    is bit-identical (the forward has no atomics)"""
    name, prec, B, cin, cout, kind, H, W, flags, act, _ = case
    f = Fwd(dev, name, prec, B, cin, cout, kind, H, W, flags, dict(act=act))
    res = f.run()
    e = f.check(res)
    print('fwd %s: err/scale %.2e' % (name, e))
    res2 = f.run()
    assert all(torch.equal(res[k], res2[k]) for k in res), name


# ----------------------------------------------------------------------------------------------------------------
# 3. epilogue stages
# ----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('case', EPI_CASES, ids=[c[0] for c in EPI_CASES])
def test_epilogue_matches_fp64(dev, case):
    """v = act(acc + bias); [aux_out = v]; v += acc_1x1; v = v*alpha + res1; v *= 1 + sigma*z1; v = v*beta + res2;
    v *= 1 + sigma*z2; out = v; nchw_out = the first nchw_out_c channels.  Residual / z views with fewer groups than
    the output add zero past their view; alpha without res1 scales v.  Bit-identical on a second run."""
    name, prec, B, cin, cout, H, W, flags, spec, _ = case
    f = Fwd(dev, name, prec, B, cin, cout, '3x3', H, W, flags, spec)
    res = f.run()
    e = f.check(res)
    print('epilogue %s: err/scale %.2e' % (name, e))
    res2 = f.run()
    assert all(torch.equal(res[k], res2[k]) for k in res), name


@pytest.mark.gpu
@pytest.mark.parametrize('prec', ['fp16', 'fp32'])
def test_inplace_rrdb_tail(dev, prec):
    """out and res2 the same view (the RRDB tail, done in place): bit-identical to the out-of-place result"""
    spec = dict(act='none', res1=(0.2, None), res2=(0.2, None))
    name = 'inplace_' + prec
    f = Fwd(dev, name, prec, 3, 64, 64, '3x3', 13, 40, 0, spec)
    ref = f.run()
    e = f.check(ref)
    g = Fwd(dev, name, prec, 3, 64, 64, '3x3', 13, 40, 0, spec)
    r2 = g.bufs['res2']
    g.c.out = r2.view(0, 64)
    before = r2.t.float().cpu()
    _, L = _mods()
    ops = L.OpList()
    ops.add_conv(g.c)
    run(ops)
    after = r2.t.float().cpu()
    H, W = 13, 40
    ng = cdiv(64, r2.cpg)
    assert torch.equal(after[:, :ng, 1:H + 1, 1:W + 1], ref['out'][:, :ng, 1:H + 1, 1:W + 1])
    keep = torch.ones(after.shape, dtype=torch.bool)
    keep[:, :ng, 1:H + 1, 1:W + 1] = False
    assert torch.equal(after[keep], before[keep])
    print('inplace %s: err/scale %.2e' % (prec, e))


@pytest.mark.gpu
@pytest.mark.parametrize('prec', ['fp16', 'fp32'])
def test_store_into_input_slice(dev, prec):
    """`out` is a channel slice of the very buffer the K loop reads (the dense concat: conv k of a dense block writes
    channels 64 + 32 k of its input buffer): the input channels, the groups past the slice and the ring stay as they
    were"""
    for name, cin, H, W, flags, spec in (('slice_r1_' + prec, 96, 13, 40, 0, dict(act='lrelu')),
                                         ('slice_1x1_' + prec, 96, 13, 40, 256, dict(act='lrelu', w1x1=64)),
                                         ('slice_res_' + prec, 160, 20, 40, 0, dict(act='lrelu', res1=(1.0, None)))):
        f = Fwd(dev, name, prec, 2, cin, 32, '3x3', H, W, flags, dict(spec, slice=True))
        before = {'out': f.xin.t.float().cpu()}
        res = f.run()
        e = f.check(res, before)
        print('slice %s: err/scale %.2e' % (name, e))


@pytest.mark.gpu
@pytest.mark.parametrize('prec', ['fp16', 'fp32'])
def test_philox_noise(dev, prec):
    """Philox z1 / z2 (layer1 != layer2, three cout blocks) against explicit z from esr_fill_noise: fp32 bit-identical
    to the explicit run, fp16 within the gate of the float64 reference on the fp32 z; seed_dev holding the seed gives
    bit for bit the `seed` result"""
    from esrganplus_amd import ops as O
    _, L = _mods()
    B, cin, cout, H, W, seed, l1, l2 = 2, 32, 72, 13, 40, 0x1234_5678_9abc, 5, 9
    spec = dict(act='lrelu', res1=(0.2, None), res2=(0.7, None))
    name = 'philox_' + prec
    f = Fwd(dev, name, prec, B, cin, cout, '3x3', H, W, 0, spec)
    f.c.noise_mode, f.c.seed, f.c.layer1, f.c.layer2 = L.NOISE_PHILOX, seed, l1, l2
    z = [O.philox_normal((B, cout, H, W), seed, lid, dev).cpu() for lid in (l1, l2)]
    # reference: the explicit-z order of the epilogue on the fp32 z the kernel draws
    r1 = q(rnd((B, cout, H, W), 'fw.res1', name), prec)[f.idx].double()
    r2 = q(rnd((B, cout, H, W), 'fw.res2', name), prec)[f.idx].double()
    zi = [t[f.idx].double() for t in z]
    v = _REFS[name][1] * f32(0.2) + r1
    v = v * (1 + f32(SIGMA) * zi[0])
    v = v * f32(0.7) + r2
    v = v * (1 + f32(SIGMA) * zi[1])
    f.checks = [('out', f.out, 0, cout, v)]
    res = f.run()
    e = f.check(res)
    print('philox %s: err/scale %.2e' % (prec, e))
    # seed through device memory (a wrong by-value seed must not matter)
    sd = torch.tensor([seed], dtype=torch.int64, device=dev)
    f.c.seed_dev, f.c.seed = sd.data_ptr(), seed + 1
    assert torch.equal(f.run()['out'], res['out'])
    if prec == 'fp32':
        g = Fwd(dev, name, prec, B, cin, cout, '3x3', H, W, 0, spec)
        for which, t in (('z1', z[0]), ('z2', z[1])):
            buf = g32(dev, prec, B, cout, H, W)
            upload(buf, t)
            g.bufs[which] = buf
            setattr(g.c, which, buf.view(0, cout))
        g.c.noise_mode = L.NOISE_EXPLICIT
        assert torch.equal(g.run()['out'], res['out'])


# ----------------------------------------------------------------------------------------------------------------
# 4. refusals
# ----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_refusals(dev):
    """configurations esr_conv_forward refuses before anything runs: the outputs stay at the sentinel"""
    E, L = _mods()
    scratch = []

    def mask_no_out2(f):
        f.c.mask = f.xin.view(0)

    def stat_sums(f):
        s = torch.zeros(2, 64, dtype=torch.float64, device=dev)
        scratch.append(s)
        f.c.stat_sums, f.c.stat_groups, f.c.stat_C = s.data_ptr(), 1, f.cout

    def w1x1(f):
        f.c.w1x1, f.c.n1x1_groups = f.wp.entries['c'].w_ptr, 1

    def ksplit_res(f):
        ws = torch.zeros(2 * f.B * f.H * f.W * 64, device=dev)
        r = g32(dev, f.prec, f.B, f.cout, f.H, f.W)
        scratch.extend([ws, r])
        f.c.ksplit, f.c.split_ws, f.c.res1 = 2, ws.data_ptr(), r.view(0)

    def setter(**kw):
        return lambda f: [setattr(f.c, k, v) for k, v in kw.items()]

    for what, (prec, B, cin, cout, kind, H, W), edit in (
            ('1x1 with two cout blocks', ('fp16', 2, 32, 64, '3x3', 13, 40), w1x1),
            ('1x1 on a 1x1 conv', ('fp16', 2, 32, 32, '1x1', 13, 40), w1x1),
            ('1x1 on a sub-pixel conv', ('fp32', 2, 16, 32, 'sub', 14, 40), w1x1),
            ('odd output, nearest-x2', ('fp16', 2, 32, 32, 'ups', 13, 40), None),
            ('odd output, sub-pixel', ('fp16', 2, 32, 32, 'sub', 14, 39), None),
            ('mask without out2', ('fp16', 2, 32, 32, '3x3', 13, 40), mask_no_out2),
            ('stat_sums without ksplit', ('fp16', 2, 32, 32, '3x3', 13, 40), stat_sums),
            ('ks 5', ('fp32', 2, 16, 32, '3x3', 13, 40), setter(ks=5)),
            ('3x3 stride 2', ('fp16', 2, 32, 32, '3x3', 13, 40), setter(stride=2)),
            ('ksplit with res1', ('fp16', 4, 64, 64, 's2', 8, 8), ksplit_res)):
        f = Fwd(dev, 'refuse ' + what, prec, B, cin, cout, kind, H, W, 0, dict(act='lrelu'))
        if edit is not None:
            edit(f)
        ops = L.OpList()
        ops.add_conv(f.c)
        with pytest.raises(L.HipExtensionError):
            ops.run(E.current_stream())
        torch.cuda.synchronize()
        for name, buf, *_ in f.checks:
            assert (buf.t.float().cpu() == SENT).all(), (what, name)
