"""The backward pass of every convolution outside the fused RDB chain, op by op through the C ABI: weight gradients
(esr_conv_wgrad: wgrad_kernel for fp32, wgrad16_kernel for fp16; esr_conv_wgrad_multi through runs of OP_WGRAD ops;
esr_grad_unpermute) and input gradients (the conv kernel on DgradPack operands with its activation-mask epilogue).
Every result is compared with float64 torch autograd on the CPU, on the values the kernels actually read (fp16
operands rounded to fp16, the stored fp16 mask).  The shapes are chosen so that every branch of the dispatch
heuristics is reached: the first section restates those heuristics in Python and pins which case reaches which branch,
so a later change that drops one fails there instead of silently narrowing the test.  Those pins, and the check of the
reference adjoint used for the up-convs, run without a GPU.

Error bounds are relative to the reference's largest magnitude, a few times the worst error measured on an MI355X.
Weight gradients are fp32 sums of products of stored values: both precisions at 2e-6 (worst 6.1e-7 fp32 — the bias
gradient of a cout-1 conv —, 3.0e-7 fp16; cin 1, cin 9 / 17 and cout 1 otherwise at most 5.3e-7 / 1.7e-7).
Input gradients: fp32 at 4e-6 (worst 8.2e-7); fp16 at 1.5e-3, where rounding the stored fp16 result alone costs up to
2^-11 of the scale (worst 4.2e-4); the input gradients of cin-1 and cin-9 / cin-17 convs, into G32 and into fp32 NCHW
(nchw_out_c = 1), at most 6.8e-7 fp32 and 2.6e-4 fp16.  The `exit` cases run the epilogue's third stage as engine.exit_to_conv uses it below
an RRDB boundary — res2 with beta != 1, Philox noise on out and on out3 = v * gamma * (1 + sigma z3), the mask next to
res2 — at the same bounds (worst 3.5e-4 fp16, 1.1e-7 fp32), in fp32 also bit for bit against explicit z2 / z3."""
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

SENT = 1234.0          # exactly representable in fp16: marks G32 elements a kernel must not write
SLOPE = 0.2            # ESR_LRELU_SLOPE
SIGMA = 0.1            # GaussianNoise sigma (engine.SIGMA, what _conv sets)
TOL_WG = 2e-6          # weight gradients, both precisions (fp32 accumulation of exact products)
TOL_DG = {'fp32': 4e-6, 'fp16': 1.5e-3}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _mods():
    from esrganplus_amd import engine as E, _lib as L
    return E, L


def cdiv(a, b):
    return (a + b - 1) // b


def seed_of(*args):
    return zlib.crc32(repr(args).encode())


def rnd(shape, *key, scale=1.0):
    g = np.random.default_rng(seed_of(*key))
    return torch.from_numpy(g.standard_normal(shape, dtype=np.float32) * np.float32(scale))


def q(t, prec):
    """the values a tensor of this precision stores"""
    return t.half().float() if prec == 'fp16' else t.float()


# ----------------------------------------------------------------------------------------------------------------
# 1. dispatch pins (CPU arithmetic only)
# ----------------------------------------------------------------------------------------------------------------

def pack_wl(S, W):
    return 2 if (W <= 4 and S == 1) else (3 if W <= 8 else 4)


def wgrad16_grid(B, H, W, cout, cin, ks, S, ups, min_wgs=64, min_rows=8, cap_rows=32):
    """wgrad16_grid + wgrad16_packed of csrc/wgrad.hip (H, W: the gradient's map, cin: the forward input channels)"""
    strips, coblocks, ciblocks = cdiv(W, 32), cdiv(cout, 32), cdiv(cdiv(cin, 16), 2)
    nco = 2 if (coblocks >= 2 or S == 2) else 1
    nci = 4 // nco
    gy, gz = cdiv(ciblocks, nci), cdiv(coblocks, nco)
    rows = min(cdiv(H, 4) * 4, cap_rows)
    want = max(4, (H * B * strips * gy * gz // 8192) // 4 * 4)
    rows = min(rows, want)
    while rows > min_rows and B * strips * cdiv(H, rows) * gy * gz < min_wgs:
        rows = ((rows // 2 + 3) // 4) * 4
    rchunks = cdiv(H, rows)
    packed = not ups and W <= 16 and B > 1 and (S == 2 or (ks == 3 and cout > 32))
    ipw = min(32 >> pack_wl(S, W) if packed else 1, B)
    while ipw < B and ipw < 0x7FFF and cdiv(B, 2 * ipw) * strips * rchunks * gy * gz >= min_wgs:
        ipw *= 2
    return dict(nco=nco, gx=cdiv(B, ipw) * strips * rchunks, gy=gy, gz=gz, rows=rows, rchunks=rchunks, ipw=ipw,
                packed=packed, strips=strips)


def batch_grid(B, H, W, cout, cin, ks):
    """the grid esr_conv_wgrad_multi gives one batchable conv, and its kind (0/1: 3x3 NCO 1/2, 2/3: 1x1 NCO 1/2)"""
    g = wgrad16_grid(B, H, W, cout, cin, ks, 1, False, 64, 32, 1 << 30)
    return g, (0 if ks == 3 else 2) + (1 if g['nco'] == 2 else 0)


def conv3_branch(prec, B, H, W, cbk, flags=0):
    """dispatch of the 3x3/s1 conv (csrc/conv_mfma.hip): (rows per wave: tiles of 4 rw rows, K loop, NCW)"""
    tiles = cdiv(W, 32) * cdiv(H, 16) * B
    rw = 1 if tiles * cbk <= 128 else (2 if tiles * cbk <= 384 else 4)
    if H <= 4:
        rw = 1
    elif H <= 8 and rw > 2:
        rw = 2
    if (flags & 256) or prec == 'fp32':
        rw = 4
    if prec == 'fp16' and rw < 4:
        return rw, 'pipe' if cbk == 1 else 'plain', 1
    if cbk == 1:
        pipe = True if flags & 128 else (False if flags & 64 else tiles <= 256)
        return 4, 'pipe' if pipe else 'plain', 1
    return 4, 'plain', 1 if tiles * ((cbk + 1) // 2) < 256 else 2


def ts2_branch(B, H, W, cbk):
    """transposed 4x4/s2 (upsample == 2, no ksplit): one cout block / the ts2_one rule / two blocks per wave"""
    if cbk == 1:
        return 'one'
    tiles = cdiv(W, 64) * cdiv(H, 16) * B
    return 'ts2_one' if tiles * ((cbk + 1) // 2) < 256 else 'ncw2'


def s2_branch(W, cbk):
    """4x4/s2 conv (the up-convs' adjoint): the wide 8x64 tile for at most two cout blocks on maps wider than 32"""
    return 'wide' if cbk <= 2 and W > 32 else 'plain'


# weight gradient, one op: prec, B, cin, cout, ks, stride, upsample, H, W (H x W: the gradient's map)
WG_CASES = [
    ('fp32', 2, 24, 40, 3, 1, 0, 13, 40),
    ('fp32', 2, 16, 24, 3, 1, 1, 12, 36),
    ('fp32', 3, 3, 32, 1, 1, 0, 9, 33),
    ('fp32', 2, 24, 3, 4, 2, 0, 9, 20),
    ('fp16', 2, 48, 32, 3, 1, 0, 37, 33),       # NCO 1, three fp16 groups, 10 row chunks (the last of one row)
    ('fp16', 2, 64, 72, 3, 1, 0, 20, 70),       # NCO 2, a ragged third cout block, three column strips
    ('fp16', 3, 32, 3, 3, 1, 0, 10, 40),        # cout 3
    ('fp16', 2, 3, 64, 3, 1, 0, 34, 36),        # cin 3
    ('fp16', 2, 64, 64, 3, 1, 1, 20, 66),       # upsample, NCO 2
    ('fp16', 2, 32, 32, 3, 1, 1, 14, 40),       # upsample, NCO 1
    ('fp16', 2, 48, 32, 1, 1, 0, 11, 40),       # 1x1, NCO 1
    ('fp16', 2, 64, 96, 1, 1, 0, 9, 33),        # 1x1, NCO 2
    ('fp16', 2, 48, 64, 4, 2, 0, 9, 20),        # 4x4/s2 on maps wider than 16: the two 8-tap launches
    ('fp16', 3, 64, 40, 4, 2, 0, 17, 34),
    ('fp16', 33, 256, 32, 3, 1, 0, 7, 10),      # unpacked small maps: two images per workgroup, B odd
    ('fp16', 37, 256, 64, 1, 1, 0, 5, 12),      # 1x1 small maps: four images per workgroup, B not a multiple
    ('fp16', 5, 64, 64, 3, 1, 0, 8, 8),         # packed (cross-check of test_gpu_wgrad_small_maps)
    ('fp16', 6, 64, 64, 4, 2, 0, 3, 6),         # packed stride 2
    # off-recipe channel counts: cin 1, a second input group of ONE channel (17 fp16, 9 fp32), cout 1; the 4x4/s2 form
    # with one input and with one output channel
    ('fp32', 2, 1, 40, 3, 1, 0, 13, 40),
    ('fp32', 2, 9, 24, 3, 1, 0, 13, 40),
    ('fp32', 2, 24, 1, 3, 1, 0, 13, 40),
    ('fp32', 2, 1, 24, 4, 2, 0, 9, 20),
    ('fp16', 2, 1, 64, 3, 1, 0, 13, 40),
    ('fp16', 2, 17, 32, 3, 1, 0, 13, 40),
    ('fp16', 3, 32, 1, 3, 1, 0, 10, 40),
    ('fp16', 2, 1, 64, 4, 2, 0, 9, 20),
    ('fp16', 2, 64, 1, 4, 2, 0, 9, 20),
]


def wg_id(c):
    return '%s-B%d-%dto%d-k%ds%d%s-%dx%d' % (c[0], c[1], c[2], c[3], c[4], c[5], 'u' if c[6] else '', c[7], c[8])


def test_wgrad_cases_reach_every_branch():
    seen = set()
    for prec, B, cin, cout, ks, st, ups, H, W in WG_CASES:
        if prec == 'fp32':
            seen.add(('fp32', ks, st, ups))
            seen |= {('fp32 cin', cin), ('fp32 cout', cout), ('fp32 cin', cin, ks, st)}
            continue
        g = wgrad16_grid(B, H, W, cout, cin, ks, st, ups)
        seen.add(('fp16', ks, st, ups, g['nco'], g['packed']))
        if not g['packed']:
            seen.add(('ipw>1', B % g['ipw'] != 0) if g['ipw'] > 1 else ('ipw=1',))
        seen.add(('ragged W', W % 32 != 0 and W > 32))
        seen.add(('ragged H', H % 4 != 0 and g['rchunks'] > 1 and H > 32))
        seen.add(('cin', cin))
        seen.add(('cout', cout))
        seen.add(('odd groups', cdiv(cin, 16) % 2 == 1 and cin > 16))
        seen.add(('one-channel last group', cin > 16 and cin % 16 == 1))
        seen |= {('cin', cin, ks, st), ('cout', cout, ks, st)}
    for k in [('fp32', 3, 1, 0), ('fp32', 3, 1, 1), ('fp32', 1, 1, 0), ('fp32', 4, 2, 0),
              ('fp16', 3, 1, 0, 1, False), ('fp16', 3, 1, 0, 2, False), ('fp16', 3, 1, 1, 2, False),
              ('fp16', 3, 1, 1, 1, False), ('fp16', 1, 1, 0, 1, False), ('fp16', 1, 1, 0, 2, False),
              ('fp16', 4, 2, 0, 2, False), ('fp16', 3, 1, 0, 2, True), ('fp16', 4, 2, 0, 2, True),
              ('ipw>1', True), ('ragged W', True), ('ragged H', True), ('cin', 3), ('cout', 3), ('odd groups', True),
              # off the recipe: one input / output channel (3x3 and the 4x4/s2 form), a last group of ONE channel
              ('cin', 1), ('cout', 1), ('one-channel last group', True), ('cin', 1, 3, 1), ('cout', 1, 3, 1),
              ('cin', 1, 4, 2), ('cout', 1, 4, 2), ('fp32 cin', 1), ('fp32 cin', 9), ('fp32 cout', 1),
              ('fp32 cin', 1, 4, 2)]:
        assert k in seen, k


# input gradient: name, prec, B, cin, cout, kind, H, W (H x W: the FORWARD conv's input = the input gradient's map),
# debug_flags, epilogue, special (DgradPack), expected branch
DG_CASES = [
    ('f32_pipe', 'fp32', 2, 24, 40, '3x3', 13, 40, 0, 'plain', None, (4, 'pipe', 1)),
    ('f32_plain', 'fp32', 2, 24, 40, '3x3', 13, 40, 64, 'plain', None, (4, 'plain', 1)),
    ('f32_ncw1', 'fp32', 2, 72, 16, '3x3', 18, 33, 0, 'plain', None, (4, 'plain', 1)),
    ('f32_ncw2', 'fp32', 16, 256, 32, '3x3', 17, 33, 0, 'plain', None, (4, 'plain', 2)),
    ('f16_rows4', 'fp16', 2, 32, 40, '3x3', 20, 40, 0, 'plain', None, (1, 'pipe', 1)),
    ('f16_rows8', 'fp16', 40, 32, 16, '3x3', 20, 40, 0, 'plain', None, (2, 'pipe', 1)),
    ('f16_rows16', 'fp16', 97, 32, 16, '3x3', 17, 33, 0, 'plain', None, (4, 'plain', 1)),
    ('f16_h4_clamp', 'fp16', 100, 32, 16, '3x3', 3, 64, 0, 'plain', None, (1, 'pipe', 1)),
    ('f16_h8_clamp', 'fp16', 49, 128, 32, '3x3', 6, 64, 0, 'plain', None, (2, 'plain', 1)),
    ('f16_flag256_pipe', 'fp16', 2, 32, 40, '3x3', 20, 40, 256 | 128, 'plain', None, (4, 'pipe', 1)),
    ('f16_flag256_plain', 'fp16', 2, 32, 40, '3x3', 20, 40, 256 | 64, 'plain', None, (4, 'plain', 1)),
    ('f16_ncw1', 'fp16', 2, 72, 48, '3x3', 18, 33, 256, 'plain', None, (4, 'plain', 1)),
    ('f16_ncw2', 'fp16', 16, 256, 32, '3x3', 17, 33, 0, 'plain', None, (4, 'plain', 2)),
    ('f16_1x1_one', 'fp16', 2, 24, 48, '1x1', 11, 40, 0, 'plain', None, 1),
    ('f16_1x1_two', 'fp16', 2, 48, 64, '1x1', 11, 40, 0, 'plain', None, 2),
    ('f32_1x1_two', 'fp32', 2, 48, 64, '1x1', 11, 40, 0, 'plain', None, 2),
    ('f16_ups_narrow', 'fp16', 2, 64, 48, 'ups', 10, 20, 0, 'plain', None, 'plain'),
    ('f16_ups_wide', 'fp16', 2, 64, 48, 'ups', 10, 40, 0, 'plain', None, 'wide'),
    ('f32_ups_wide', 'fp32', 2, 48, 32, 'ups', 6, 34, 0, 'plain', None, 'wide'),
    ('f16_ts2_one', 'fp16', 2, 24, 64, 'ts2', 18, 40, 0, 'plain', None, 'one'),
    ('f16_ts2_one_rule', 'fp16', 2, 96, 64, 'ts2', 18, 40, 0, 'plain', None, 'ts2_one'),
    ('f16_ts2_ncw2', 'fp16', 16, 256, 32, 'ts2', 64, 66, 0, 'plain', None, 'ncw2'),
    ('f32_ts2_ncw2', 'fp32', 16, 256, 32, 'ts2', 64, 66, 0, 'plain', None, 'ncw2'),
    ('f16_mask_lrelu', 'fp16', 2, 40, 48, '3x3', 13, 40, 0, 'mask_lrelu', None, (1, 'plain', 1)),
    ('f16_mask_relu', 'fp16', 2, 40, 48, '3x3', 13, 40, 0, 'mask_relu', None, (1, 'plain', 1)),
    ('f32_mask_lrelu', 'fp32', 2, 40, 48, '3x3', 13, 40, 0, 'mask_lrelu', None, (4, 'plain', 1)),
    ('f16_mask_ts2', 'fp16', 2, 24, 64, 'ts2', 18, 40, 0, 'mask_lrelu', None, 'one'),
    ('f16_general_res1', 'fp16', 2, 96, 48, '3x3', 13, 40, 0, 'general1', None, (1, 'plain', 1)),
    ('f16_general_res2', 'fp16', 2, 96, 48, '3x3', 13, 40, 0, 'general2', None, (1, 'plain', 1)),
    ('f32_general_res2', 'fp32', 2, 96, 48, '3x3', 13, 40, 0, 'general2', None, (4, 'plain', 1)),
    ('f16_sum_fold', 'fp16', 2, 64, 48, '3x3', 13, 40, 0, 'plain', (32, 0, 32), (1, 'plain', 1)),
    # off-recipe channel counts.  nchw_*: fea_conv's input gradient as the training plan's exit issues it (no G32
    # output, nchw_out_c = the forward cin = 1); cin17 / cin9: the input gradient's second group holds ONE channel
    ('f16_nchw_cin1', 'fp16', 2, 1, 64, '3x3', 13, 40, 0, 'nchw', None, (1, 'pipe', 1)),
    ('f32_nchw_cin1', 'fp32', 2, 1, 64, '3x3', 13, 40, 0, 'nchw', None, (4, 'pipe', 1)),
    ('f16_nchw_cin3', 'fp16', 2, 3, 64, '3x3', 13, 40, 0, 'nchw', None, (1, 'pipe', 1)),
    ('f16_cin1', 'fp16', 2, 1, 40, '3x3', 13, 40, 0, 'plain', None, (1, 'pipe', 1)),
    ('f32_cin1', 'fp32', 2, 1, 40, '3x3', 13, 40, 0, 'plain', None, (4, 'pipe', 1)),
    ('f16_cin17', 'fp16', 2, 17, 40, '3x3', 13, 40, 0, 'plain', None, (1, 'pipe', 1)),
    ('f32_cin9', 'fp32', 2, 9, 40, '3x3', 13, 40, 0, 'plain', None, (4, 'pipe', 1)),
    ('f16_exit', 'fp16', 2, 96, 48, '3x3', 13, 40, 0, 'exit', None, (1, 'plain', 1)),
    ('f32_exit', 'fp32', 2, 96, 48, '3x3', 13, 40, 0, 'exit', None, (4, 'plain', 1)),
]


def dg_branch(prec, B, cin, cout, kind, H, W, flags):
    cbk = cdiv(cin, 32)
    if kind == '3x3':
        return conv3_branch(prec, B, H, W, cbk, flags)
    if kind == '1x1':
        return 1 if cbk == 1 else 2
    if kind == 'ups':
        return s2_branch(W, cbk)
    return ts2_branch(B, H, W, cbk)


def test_dgrad_cases_reach_every_branch():
    for name, prec, B, cin, cout, kind, H, W, flags, epi, special, want in DG_CASES:
        assert dg_branch(prec, B, cin, cout, kind, H, W, flags) == want, name
    got = {(c[1], c[5], c[11]) for c in DG_CASES}
    for k in [('fp32', '3x3', (4, 'pipe', 1)), ('fp32', '3x3', (4, 'plain', 1)), ('fp32', '3x3', (4, 'plain', 2)),
              ('fp16', '3x3', (1, 'pipe', 1)), ('fp16', '3x3', (2, 'pipe', 1)), ('fp16', '3x3', (4, 'plain', 1)),
              ('fp16', '3x3', (4, 'pipe', 1)), ('fp16', '3x3', (1, 'plain', 1)), ('fp16', '3x3', (2, 'plain', 1)),
              ('fp16', '3x3', (4, 'plain', 2)), ('fp16', '1x1', 1), ('fp16', '1x1', 2),
              ('fp16', 'ups', 'plain'), ('fp16', 'ups', 'wide'), ('fp16', 'ts2', 'one'), ('fp16', 'ts2', 'ts2_one'),
              ('fp16', 'ts2', 'ncw2')]:
        assert k in got, k
    # 16-row fp16 tiles reached by grid size alone, and by debug_flags 256 on a grid that would take 4-row tiles
    assert any(c[1] == 'fp16' and c[8] == 0 and c[11] == (4, 'plain', 1) for c in DG_CASES)
    assert any(c[1] == 'fp16' and c[8] & 256 and conv3_branch('fp16', c[2], c[6], c[7], cdiv(c[3], 32))[0] == 1
               for c in DG_CASES if c[5] == '3x3')
    # the H <= 4 / H <= 8 clamps change what the grid size alone picks
    for name, rw in (('f16_h4_clamp', 1), ('f16_h8_clamp', 2)):
        c = next(c for c in DG_CASES if c[0] == name)
        tiles = cdiv(c[7], 32) * cdiv(c[6], 16) * c[2]
        assert rw < (1 if tiles * cdiv(c[3], 32) <= 128 else (2 if tiles * cdiv(c[3], 32) <= 384 else 4)), name
    epis = {c[9] for c in DG_CASES}
    assert {'mask_lrelu', 'mask_relu', 'general1', 'general2', 'exit'} <= epis
    assert {c[1] for c in DG_CASES if c[9] == 'exit'} == {'fp16', 'fp32'}
    assert any(c[10] for c in DG_CASES)
    # off the recipe, per precision: the input gradient of a forward-cin-1 conv into fp32 NCHW (nchw_out_c = 1) and
    # into G32, and of a conv whose last input group holds ONE channel
    for p, cpg in (('fp16', 16), ('fp32', 8)):
        cs = [c for c in DG_CASES if c[1] == p and c[5] == '3x3']
        assert any(c[3] == 1 and c[9] == 'nchw' for c in cs), p
        assert any(c[3] == 1 and c[9] == 'plain' for c in cs), p
        assert any(c[3] == cpg + 1 for c in cs), p


# batched weight gradients: one run of OP_WGRAD ops (B, cin, cout, ks, upsample, H, W, tap_major)
MULTI_SHAPES = {
    'a': (2, 64, 32, 3, 0, 12, 40),     # 3x3 NCO 1
    'b': (2, 48, 64, 3, 0, 9, 33),      # 3x3 NCO 2
    'c': (2, 64, 32, 1, 0, 12, 40),     # 1x1 NCO 1
    'd': (2, 48, 72, 1, 0, 9, 33),      # 1x1 NCO 2
    'u': (2, 32, 48, 3, 1, 12, 40),     # upsample: not batchable
}
MULTI_RUN = ['a', 'b', 'u'] + ['c', 'd', 'a', 'b'] * 5           # 23 ops: 2 batched, 1 single, 20 = 18 + 2 batched


def test_multi_run_reaches_every_batch_kind_and_splits():
    kinds = {batch_grid(*(MULTI_SHAPES[k][i] for i in (0, 5, 6, 2, 1, 3)))[1] for k in MULTI_RUN if not MULTI_SHAPES[k][4]}
    assert kinds == {0, 1, 2, 3}
    runs, cur = [], 0
    for k in MULTI_RUN:
        if MULTI_SHAPES[k][4]:
            runs.append(cur)
            cur = 0
        else:
            cur += 1
    runs.append(cur)
    assert runs[0] >= 2 and max(runs) > 18 and max(runs) % 18 >= 2     # the long run splits into two batches
    assert len(MULTI_RUN) <= 24                                         # one esr_conv_wgrad_multi call (ESR_WGRAD_RUN_MAX)


# ----------------------------------------------------------------------------------------------------------------
# references
# ----------------------------------------------------------------------------------------------------------------

def ups_dgrad_kernel(w):
    """[cin][cout][4][4] kernel of the 4x4/s2/p1 conv over g that is the adjoint of nearest-x2 + 3x3 conv with the
    OIHW weights w (esr_pack.ups_dgrad): tap ky collects the forward rows {2}, {1,2}, {0,1}, {0} (same for kx)"""
    rows = [(2, 2), (1, 2), (0, 1), (0, 0)]
    w = w.double()
    k = torch.zeros(w.shape[1], w.shape[0], 4, 4, dtype=torch.float64)
    for ky, (r0, r1) in enumerate(rows):
        for kx, (c0, c1) in enumerate(rows):
            k[:, :, ky, kx] = w[:, :, r0:r1 + 1, c0:c1 + 1].sum((2, 3)).t()
    return k


def test_ups_dgrad_reference_is_the_adjoint():
    """the reference the up-conv input-gradient cases use equals autograd through F.interpolate + conv2d"""
    w = rnd((5, 7, 3, 3), 'ups_adj.w').double()
    x = rnd((2, 7, 5, 6), 'ups_adj.x').double().requires_grad_(True)
    g = rnd((2, 5, 10, 12), 'ups_adj.g').double()
    F.conv2d(F.interpolate(x, scale_factor=2, mode='nearest'), w, padding=1).backward(g)
    got = F.conv2d(g, ups_dgrad_kernel(w), stride=2, padding=1)
    assert (got - x.grad).abs().max().item() <= 1e-12 * x.grad.abs().max().item()


def wgrad_ref(x, g, ks, st, ups):
    """float64 (dW OIHW, db) of conv2d(x) [nearest-x2 first when ups] for the upstream gradient g"""
    xi = F.interpolate(x.double(), scale_factor=2, mode='nearest') if ups else x.double()
    w = torch.zeros(g.shape[1], x.shape[1], ks, ks, dtype=torch.float64, requires_grad=True)
    F.conv2d(xi, w, stride=st, padding=(ks - 1) // 2).backward(g.double())
    return w.grad, g.double().sum((0, 2, 3))


def rel_err(got, ref):
    return (got.double() - ref.double()).abs().max().item() / max(ref.abs().max().item(), 1e-30)


# ----------------------------------------------------------------------------------------------------------------
# G32 helpers
# ----------------------------------------------------------------------------------------------------------------

def run(ops):
    E, _ = _mods()
    ops.run(E.current_stream())
    torch.cuda.synchronize()


def g32(dev, prec, B, C_, H, W, fill=None):
    E, _ = _mods()
    b = E.G32(B, C_, H, W, prec, dev)
    if fill is not None:
        b.t.fill_(fill)
    return b


def layout_op(ops, buf, nchw, C_, to_g32):
    _, L = _mods()
    lo = L.esr_layout()
    lo.dtype, lo.to_g32 = buf.esr_dtype, to_g32
    lo.B, lo.C, lo.H, lo.W = buf.B, C_, buf.H, buf.W
    lo.nchw, lo.g32 = nchw.data_ptr(), buf.view(0, C_)
    ops.add(L.OP_LAYOUT, 'layout', lo)


def upload(buf, x):
    _, L = _mods()
    xd = x.float().contiguous().to(buf.t.device)
    ops = L.OpList()
    layout_op(ops, buf, xd, int(x.shape[1]), 1)
    run(ops)


def download(buf, C_):
    _, L = _mods()
    out = torch.empty(buf.B, C_, buf.H, buf.W, device=buf.t.device)
    ops = L.OpList()
    layout_op(ops, buf, out, C_, 0)
    run(ops)
    return out.cpu()


def region(buf):
    """all channel lanes of the image pixels as NCHW (padding lanes included), and every other element of the buffer"""
    t = buf.t.float().cpu()
    H, W = buf.H, buf.W
    inner = t[:, :, 1:H + 1, 1:W + 1, :].permute(0, 1, 4, 2, 3).reshape(buf.B, buf.ng * buf.cpg, H, W)
    rest = torch.ones(t.shape, dtype=torch.bool)
    rest[:, :, 1:H + 1, 1:W + 1, :] = False
    return inner, t[rest]


# ----------------------------------------------------------------------------------------------------------------
# 2. weight gradient, one op
# ----------------------------------------------------------------------------------------------------------------

class WgradRig:
    """saved input and upstream gradient of one conv in G32 buffers, its float64 reference, and esr_wgrad ops on them"""
    _refs = {}

    def __init__(self, dev, case):
        E, L = _mods()
        prec, B, cin, cout, ks, st, ups, H, W = case
        self.dev, self.case, self.prec = dev, case, prec
        self.B, self.cin, self.cout, self.ks, self.st, self.ups, self.H, self.W = B, cin, cout, ks, st, ups, H, W
        Hi, Wi = (H // 2, W // 2) if ups else (H * st, W * st)
        x = q(rnd((B, cin, Hi, Wi), 'wg.x', case), prec)
        g = q(rnd((B, cout, H, W), 'wg.g', case), prec)
        if case not in WgradRig._refs:
            WgradRig._refs[case] = wgrad_ref(x, g, ks, st, ups)
        self.ref_w, self.ref_b = WgradRig._refs[case]
        self.xin, self.gin = g32(dev, prec, B, cin, Hi, Wi), g32(dev, prec, B, cout, H, W)
        upload(self.xin, x)
        upload(self.gin, g)
        self.dt = E._dt(prec)[0]

    def op(self, dw, db, scale=1.0, tap_major=0):
        _, L = _mods()
        wg = L.esr_wgrad()
        wg.dtype, wg.ks, wg.stride, wg.upsample = self.dt, self.ks, self.st, self.ups
        wg.B, wg.H, wg.W, wg.cout, wg.cin = self.B, self.H, self.W, self.cout, self.cin
        wg.g, wg.in_ = self.gin.view(0, self.cout), self.xin.view(0, self.cin)
        wg.dw, wg.dbias, wg.scale, wg.tap_major = dw.data_ptr(), db.data_ptr() if db is not None else None, scale, tap_major
        return wg

    def run(self, det, dw0=None, db0=0.0, bias=True, scale=1.0, tap_major=0):
        """(dw as OIHW, db or None) of one esr_conv_wgrad on buffers pre-filled with dw0 / db0"""
        E, L = _mods()
        n = self.cout * self.cin * self.ks * self.ks
        if dw0 is None:
            dw0 = torch.zeros(n)
        elif tap_major:
            dw0 = dw0.reshape(self.cout, self.cin, -1).permute(2, 0, 1)
        dw = dw0.reshape(-1).clone().to(self.dev)
        db = torch.full((self.cout,), db0, device=self.dev) if bias else None
        ops = L.OpList()
        ops.add(L.OP_WGRAD, 'wgrad', self.op(dw, db, scale, tap_major))
        arena = E.attach_wgrad_arena(ops, self.dev) if det else None
        assert (arena is not None) == det
        run(ops)
        dw = dw.cpu()
        dw = dw.reshape(self.ks * self.ks, self.cout, self.cin).permute(1, 2, 0) if tap_major else dw
        return dw.reshape(self.cout, self.cin, self.ks, self.ks), (db.cpu() if bias else None)


_WG_ERRS = {}


@pytest.mark.gpu
@pytest.mark.parametrize('det', [True, False], ids=['det', 'atomic'])
@pytest.mark.parametrize('case', WG_CASES, ids=wg_id)
def test_wgrad_matches_fp64(dev, case, det):
    """dW and db of every wgrad instantiation against float64 autograd; the deterministic form is bit-identical run to
    run and the atomic form agrees with it"""
    rig = WgradRig(dev, case)
    dw, db = rig.run(det)
    ew, eb = rel_err(dw, rig.ref_w), rel_err(db, rig.ref_b)
    print('wgrad %s %s: dW err/scale %.2e, db %.2e' % (wg_id(case), 'det' if det else 'atomic', ew, eb))
    assert ew <= TOL_WG and eb <= TOL_WG, (ew, eb)
    if det:
        dw2, db2 = rig.run(True)
        assert torch.equal(dw, dw2) and torch.equal(db, db2)
        _WG_ERRS[case] = (dw, db)
    elif case in _WG_ERRS:
        dwd, dbd = _WG_ERRS[case]
        assert rel_err(dw, dwd) <= TOL_WG and rel_err(db, dbd) <= TOL_WG


WG_CONTRACT = [
    ('fp32', 2, 24, 40, 3, 1, 0, 13, 40),
    ('fp16', 2, 48, 32, 3, 1, 0, 37, 33),
    ('fp16', 2, 64, 64, 3, 1, 1, 20, 66),
    ('fp16', 2, 64, 96, 1, 1, 0, 9, 33),
    ('fp16', 2, 48, 64, 4, 2, 0, 9, 20),
    ('fp16', 6, 64, 64, 4, 2, 0, 3, 6),
]


@pytest.mark.gpu
@pytest.mark.parametrize('det', [True, False], ids=['det', 'atomic'])
@pytest.mark.parametrize('case', WG_CONTRACT, ids=wg_id)
def test_wgrad_contract(dev, case, det):
    """dbias = NULL leaves no bias write; scale multiplies; results ADD to what dW / db hold; tap_major = 1 lays dW out
    as [tap][cout][cin] (fp16 only)"""
    rig = WgradRig(dev, case)
    dw, db = rig.run(det, bias=False)
    assert db is None and rel_err(dw, rig.ref_w) <= TOL_WG
    s = 1.0 / 1024
    dw0 = rnd(tuple(rig.ref_w.shape), 'wg.dw0', case, scale=rig.ref_w.abs().max().item() * s)
    db0 = 0.375 * rig.ref_b.abs().max().item() * s
    dw, db = rig.run(det, dw0=dw0, db0=db0, scale=s)
    assert rel_err(dw - dw0, rig.ref_w * s) <= 2 * TOL_WG, rel_err(dw - dw0, rig.ref_w * s)
    assert rel_err(db - db0, rig.ref_b * s) <= 2 * TOL_WG
    if case[0] == 'fp16':
        dw, db = rig.run(det, tap_major=1, dw0=dw0, db0=db0)
        assert rel_err(dw - dw0, rig.ref_w) <= 2 * TOL_WG and rel_err(db - db0, rig.ref_b) <= 2 * TOL_WG


@pytest.mark.gpu
def test_wgrad_refusals(dev):
    """tap_major with fp32, an fp16 partial arena that is too small, and an unsupported ks / stride are errors before
    anything runs: the gradient buffers stay untouched"""
    E, L = _mods()
    for case, edit in ((('fp32', 2, 24, 40, 3, 1, 0, 13, 40), dict(tap_major=1)),
                       (('fp16', 2, 48, 32, 3, 1, 0, 37, 33), 'small_arena'),
                       (('fp16', 2, 48, 64, 4, 2, 0, 9, 20), 'small_arena'),
                       (('fp16', 2, 48, 32, 3, 1, 0, 37, 33), dict(stride=2)),
                       (('fp32', 2, 24, 40, 3, 1, 0, 13, 40), dict(ks=5))):
        rig = WgradRig(dev, case)
        dw = torch.full((rig.cout * rig.cin * 16,), SENT, device=dev)
        db = torch.full((rig.cout,), SENT, device=dev)
        wg = rig.op(dw, db)
        ops = L.OpList()
        if edit == 'small_arena':
            ops.add(L.OP_WGRAD, 'wgrad', wg)
            arena = E.attach_wgrad_arena(ops, dev)
            ops.ops[0].u.wgrad.partial_elems = arena.numel() // 2
            ops._arr = None
        else:
            for k, v in edit.items():
                setattr(wg, k, v)
            ops.add(L.OP_WGRAD, 'wgrad', wg)
        with pytest.raises(L.HipExtensionError):
            ops.run(E.current_stream())
        torch.cuda.synchronize()
        assert (dw.cpu() == SENT).all() and (db.cpu() == SENT).all(), (case, edit)


# ----------------------------------------------------------------------------------------------------------------
# 3. batched weight gradients
# ----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_wgrad_multi_run(dev):
    """One list of 23 consecutive OP_WGRAD ops (all four batch kinds, an up-conv in the middle, a run of 20 batchable
    ops that splits at WG_BATCH_MAX, tap_major on every third): every gradient matches its float64 reference and its
    own single-op result, with one shared deterministic arena (bit-identical twice) and with atomics"""
    E, L = _mods()
    rigs = {k: WgradRig(dev, ('fp16', B, cin, cout, ks, 1, ups, H, W))
            for k, (B, cin, cout, ks, ups, H, W) in MULTI_SHAPES.items()}
    singles = {k: r.run(True) for k, r in rigs.items()}

    def run_list(det):
        ops, outs = L.OpList(), []
        for i, k in enumerate(MULTI_RUN):
            r = rigs[k]
            dw = torch.zeros(r.cout * r.cin * r.ks * r.ks, device=dev)
            db = torch.zeros(r.cout, device=dev)
            tm = int(i % 3 == 1)
            ops.add(L.OP_WGRAD, 'wgrad', r.op(dw, db, tap_major=tm))
            outs.append((k, dw, db, tm))
        arena = E.attach_wgrad_arena(ops, dev) if det else None
        assert (arena is not None) == det
        run(ops)
        res = []
        for k, dw, db, tm in outs:
            r = rigs[k]
            dw = dw.cpu()
            dw = dw.reshape(r.ks * r.ks, r.cout, r.cin).permute(1, 2, 0) if tm else dw
            res.append((k, dw.reshape(r.cout, r.cin, r.ks, r.ks), db.cpu()))
        return res

    d1, d2, at = run_list(True), run_list(True), run_list(False)
    worst = 0.0
    for (k, dw, db), (_, dw2, db2), (_, dwa, dba) in zip(d1, d2, at):
        r = rigs[k]
        assert torch.equal(dw, dw2) and torch.equal(db, db2), k
        for w_, b_ in ((dw, db), (dwa, dba)):
            e = max(rel_err(w_, r.ref_w), rel_err(b_, r.ref_b))
            worst = max(worst, e)
            assert e <= TOL_WG, (k, e)
            assert rel_err(w_, singles[k][0]) <= TOL_WG and rel_err(b_, singles[k][1]) <= TOL_WG, k
    print('wgrad multi: worst err/scale %.2e' % worst)


# ----------------------------------------------------------------------------------------------------------------
# 4. esr_grad_unpermute
# ----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('pairs', [True, False], ids=['pairs', 'elements'])
def test_grad_unpermute(dev, pairs):
    """tap-major slots of ntap 9, 1 and 16 and different sizes rewritten into OIHW: an exact data move (numpy
    transpose); flat elements outside every slot stay untouched"""
    E, L = _mods()
    slots = [(0, 40, 24, 9), (9000, 3, 64, 1), (9200, 64, 48, 16), (60500, 32, 3, 9), (61500, 72, 64, 1), (66200, 5, 7, 16)]
    n = 67000
    flat = torch.full((n,), SENT, device=dev)
    tmg = E.TapMajorGrads(flat)
    for off, co, ci, nt in slots:
        tmg.slot(off, co, ci, nt)
    src = rnd((n,), 'unperm.src')
    tmg.tm.copy_(src)
    up = tmg.op()
    assert up.n_pairs == sum(co * ci for _, co, ci, _ in slots)
    if not pairs:
        up.n_pairs = 0
    ops = L.OpList()
    ops.add(L.OP_UNPERMUTE, 'unpermute', up)
    run(ops)
    want = np.full(n, SENT, dtype=np.float32)
    s = src.numpy()
    for off, co, ci, nt in slots:
        m = co * ci * nt
        want[off:off + m] = s[off:off + m].reshape(nt, co, ci).transpose(1, 2, 0).reshape(-1)
    assert np.array_equal(flat.cpu().numpy(), want)


# ----------------------------------------------------------------------------------------------------------------
# 5. input gradient per dispatch branch
# ----------------------------------------------------------------------------------------------------------------

_DG_REFS = {}
_DG_ERRS = {}


def dgrad_ref(case, w, gy, idx):
    """float64 input gradient of the forward conv for images idx (w, gy: the stored values)"""
    name, prec, B, cin, cout, kind, H, W, flags, epi, special, _ = case
    gy = gy[idx].double()
    w = w.double()
    if special:
        dst, src, cnt = special
        w = w.clone()
        w[:, dst:dst + cnt] += w[:, src:src + cnt]
        w = q(w, prec).double()
    if kind == 'ups':
        return F.conv2d(gy, q(ups_dgrad_kernel(w), prec).double(), stride=2, padding=1)
    if kind == 'ts2':
        return F.conv_transpose2d(gy, w, stride=2, padding=1)
    return F.conv_transpose2d(gy, w, padding=1 if kind == '3x3' else 0)


def check_buffer(buf, C_, name):
    """inner lanes past C_ in the last written group are zero (the G32 invariant), groups past the view and every
    element outside the image hold the sentinel"""
    inner, rest = region(buf)
    cpad = cdiv(C_, buf.cpg) * buf.cpg
    assert (inner[:, C_:cpad] == 0).all(), '%s: padding lanes not zero' % name
    assert (inner[:, cpad:] == SENT).all(), '%s: wrote groups past the view' % name
    assert (rest == SENT).all(), '%s: wrote outside the image' % name


@pytest.mark.gpu
@pytest.mark.parametrize('case', DG_CASES, ids=[c[0] for c in DG_CASES])
def test_dgrad_matches_fp64(dev, case):
    """Input gradient of the forward conv (3x3 / 1x1 transposed, the up-conv adjoint, the transposed 4x4/s2) times
    act'(stored mask) against float64 autograd on the first and last image.  Output buffers are pre-filled with a
    sentinel: ragged tiles must not write the zero ring, the rows / columns past the map or the groups past the view."""
    E, L = _mods()
    name, prec, B, cin, cout, kind, H, W, flags, epi, special, _ = case
    dt = E._dt(prec)[0]
    ks = {'3x3': 3, '1x1': 1, 'ups': 3, 'ts2': 4}[kind]
    Ho, Wo = {'3x3': (H, W), '1x1': (H, W), 'ups': (2 * H, 2 * W), 'ts2': (H // 2, W // 2)}[kind]
    w = q(rnd((cout, cin, ks, ks), 'dg.w', name, scale=1.0 / np.sqrt(cout * ks * ks)), prec)
    gy = q(rnd((B, cout, Ho, Wo), 'dg.gy', name), prec)
    idx = [0, B - 1]
    if name not in _DG_REFS:
        _DG_REFS[name] = dgrad_ref(case, w, gy, idx)
    gx = _DG_REFS[name]

    sp = {}
    if special:
        sp['sum'] = special
    if kind == 'ups':
        sp['ups'] = True
    if kind == 'ts2':
        sp['ts2'] = True
    dp = E.DgradPack([('c', w.to(dev))], prec, dev, {'c': sp} if sp else {})
    st = E.current_stream()
    dp.ensure(st)
    gin = g32(dev, prec, B, cout, Ho, Wo)
    upload(gin, gy)
    kw = {'3x3': {}, '1x1': {}, 'ups': dict(ks=4, stride=2), 'ts2': dict(ks=4, stride=1, upsample=2)}[kind]
    c = E._conv(dt, B, H, W, gin.view(0), cout, None, dp.entries['c'], L.ACT_NONE, **kw)
    c.bias = None
    c.debug_flags |= flags
    cpg = gin.cpg
    extra = cdiv(cin, cpg) * cpg + cpg                                       # one whole group past the view
    out = g32(dev, prec, B, extra, H, W, SENT)
    checks = []                                                              # (buffer, channels, reference)
    nchw = None
    if epi == 'plain':
        c.out = out.view(0, cin)
        checks.append(('out', out, cin, gx))
    elif epi == 'nchw':
        nchw = torch.full((B * cin * H * W + 4096,), SENT, device=dev)
        c.nchw_out_c, c.nchw_out = cin, nchw.data_ptr()
    elif epi.startswith('mask'):
        act = L.ACT_RELU if epi == 'mask_relu' else L.ACT_LRELU
        m = rnd((B, cin, H, W), 'dg.mask', name)
        m = torch.where(m.abs() < 0.3, torch.zeros_like(m), m)              # exact zeros: act' of the negative side
        mk = g32(dev, prec, B, cin, H, W)
        upload(mk, m)
        m = q(m, prec)[idx].double()
        neg = 0.0 if act == L.ACT_RELU else SLOPE
        c.mask, c.out2, c.mask_cb_begin, c.mask_act = mk.view(0, cin), out.view(0, cin), 0, act
        checks.append(('out2', out, cin, gx * torch.where(m > 0, 1.0, neg)))
    elif epi == 'exit':
        # the slice-x conv that closes a block of the per-conv backward below an RRDB boundary (engine.exit_to_conv with
        # a skip_out), every stage at once: v = (acc * alpha + res1) * beta + res2;  v *= 1 + sigma z2;  out = v;
        # out2 = v * act'(mask) from cout block mask_cb_begin;  out3 = v * gamma * (1 + sigma z3) — z from the fused
        # Philox stream (layer2 != layer3), compared on the z esr_fill_noise reports for the same key
        from esrganplus_amd import ops as O
        f32 = lambda v_: float(np.float32(v_))
        mcb, alpha, beta, gamma, l2, l3, seed = 1, 0.2, 0.7, 0.2, 7, 91, 0x1234_5678_9abc
        cm = cin - 32 * mcb
        r1 = q(rnd((B, cin, H, W), 'dg.res1', name), prec)
        r2 = q(rnd((B, cin, H, W), 'dg.res2', name), prec)
        m = rnd((B, cm, H, W), 'dg.mask', name)
        m = torch.where(m.abs() < 0.3, torch.zeros_like(m), m)
        bufs = {}
        for key, t in (('res1', r1), ('res2', r2), ('mask', m)):
            bufs[key] = g32(dev, prec, B, t.shape[1], H, W)
            upload(bufs[key], t)
        z2, z3 = (O.philox_normal((B, cin, H, W), seed, lid, dev).cpu() for lid in (l2, l3))
        v = (gx * f32(alpha) + r1[idx].double()) * f32(beta) + r2[idx].double()
        v = v * (1 + f32(SIGMA) * z2[idx].double())
        out2 = g32(dev, prec, B, cdiv(cm, cpg) * cpg + cpg, H, W, SENT)
        out3 = g32(dev, prec, B, extra, H, W, SENT)
        c.alpha, c.res1 = alpha, bufs['res1'].view(0, cin)
        c.beta, c.res2 = beta, bufs['res2'].view(0, cin)
        c.noise_mode, c.seed, c.layer2, c.layer3 = L.NOISE_PHILOX, seed, l2, l3
        c.out, c.out3, c.gamma = out.view(0, cin), out3.view(0, cin), gamma
        c.mask, c.out2, c.mask_cb_begin, c.mask_act = bufs['mask'].view(0, cm), out2.view(0, cm), mcb, L.ACT_LRELU
        mq = q(m, prec)[idx].double()
        checks.append(('out', out, cin, v))
        checks.append(('out2', out2, cm, v[:, 32 * mcb:] * torch.where(mq > 0, 1.0, SLOPE)))
        checks.append(('out3', out3, cin, v * f32(gamma) * (1 + f32(SIGMA) * z3[idx].double())))
    else:
        # the general epilogue: v = acc * alpha + res1 [* beta + res2]; out = v; out2 = v * act'(mask) for cout blocks
        # >= mask_cb_begin, out2 / mask indexed from that block
        mcb, alpha, beta = 1, 0.2, 1.0
        cm = cin - 32 * mcb
        r1 = q(rnd((B, cin, H, W), 'dg.res1', name), prec)
        m = rnd((B, cm, H, W), 'dg.mask', name)
        m = torch.where(m.abs() < 0.3, torch.zeros_like(m), m)
        bufs = {}
        for key, t in (('res1', r1), ('mask', m)):
            bufs[key] = g32(dev, prec, B, t.shape[1], H, W)
            upload(bufs[key], t)
        v = gx * alpha + r1[idx].double()
        c.alpha, c.res1 = alpha, bufs['res1'].view(0, cin)
        if epi == 'general2':
            r2 = q(rnd((B, cin, H, W), 'dg.res2', name), prec)
            bufs['res2'] = g32(dev, prec, B, cin, H, W)
            upload(bufs['res2'], r2)
            c.res2, c.beta = bufs['res2'].view(0, cin), beta
            v = v * beta + r2[idx].double()
        out2 = g32(dev, prec, B, cdiv(cm, cpg) * cpg + cpg, H, W, SENT)
        c.out = out.view(0, cin)
        c.mask, c.out2, c.mask_cb_begin, c.mask_act = bufs['mask'].view(0, cm), out2.view(0, cm), mcb, L.ACT_LRELU
        mq = q(m, prec)[idx].double()
        checks.append(('out', out, cin, v))
        checks.append(('out2', out2, cm, v[:, 32 * mcb:] * torch.where(mq > 0, 1.0, SLOPE)))
    ops = L.OpList()
    ops.add_conv(c)
    run(ops)
    worst = 0.0
    for what, buf, C_, ref in checks:
        got = region(buf)[0][idx, :C_]
        e = rel_err(got, ref)
        worst = max(worst, e)
        assert e <= TOL_DG[prec], '%s %s: err/scale %.3e' % (name, what, e)
        check_buffer(buf, C_, '%s %s' % (name, what))
    if nchw is not None:
        n = B * cin * H * W
        got = nchw.cpu()
        worst = rel_err(got[:n].reshape(B, cin, H, W)[idx], gx)
        assert worst <= TOL_DG[prec], '%s nchw: err/scale %.3e' % (name, worst)
        assert (got[n:] == SENT).all(), '%s: wrote past nchw_out_c channels' % name
    print('dgrad %s: err/scale %.2e' % (name, worst))
    if epi == 'exit' and prec == 'fp32':
        # the same launch on explicit z2 / z3 holding that z: bit for bit the Philox result, in all three outputs
        first = [buf.t.clone() for _, buf, _, _ in checks]
        for _, buf, _, _ in checks:
            buf.t.fill_(SENT)
        for which, t in (('z2', z2), ('z3', z3)):
            bufs[which] = g32(dev, prec, B, cin, H, W)
            upload(bufs[which], t)
            setattr(c, which, bufs[which].view(0, cin))
        c.noise_mode = L.NOISE_EXPLICIT
        ops = L.OpList()
        ops.add_conv(c)
        run(ops)
        for (what, buf, _, _), t in zip(checks, first):
            assert torch.equal(buf.t, t), '%s %s: explicit z differs from the Philox stream' % (name, what)
