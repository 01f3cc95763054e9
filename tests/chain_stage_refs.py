"""Stage-local float64 references of one ResidualDenseBlock_5C (block.py:260-268) and of its backward in the form the
fused chains compute it (csrc/rdb_chain_kernel.h; include/esrgan_hip.h: esr_rdb_block).  Every stage is a function of
the inputs it is GIVEN: a caller that passes the values a kernel stored for the earlier stages gets, for each stage, what
that stage alone should have produced, so a rounding or a LeakyReLU-mask flip in one stage cannot leak into the
comparison of the next.  A caller that passes nothing gets the stages composed (tests/test_chain_stage_refs.py pins that
form to oracle.ref_torch and to autograd).  CPU, torch only.

Weights are the values the packed operands hold: the fp32 master rounded once to the storage type; in the backward the
master times float32(scale), with the fold_co0 sum added first, all in fp32, then rounded once (esr_pack.gather /
fold_co0 / one_t; tests/pack_refs.py: gather_piece).  Biases stay fp32."""
import torch
import torch.nn.functional as F

SLOPE = 0.2          # ESR_LRELU_SLOPE
SIGMA = 0.1          # GaussianNoise sigma
MASK_EXCLUDE = 1e-4  # |a_k| below this share of max|a_k|: the sign of the kernel's fp32 pre-activation is not pinned
MASK_SHARE = 5e-3    # at most this share of a stage's elements may be left out for it


def _key(p, name):
    return (p + '.' + name) if p else name


def _round(t, prec):
    if prec == 'fp16':
        return t.float().half().double()
    if prec == 'fp32':
        return t.float().double()
    return t.double()


def forward_weights(sd, p, prec):
    """{'w1'..'w5', 'b1'..'b5', 'w1x1'} of the dense block at prefix p of the state dict sd, float64; prec 'fp16' /
    'fp32': the weights as stored, None: the master unrounded"""
    W = {'w1x1': _round(sd[_key(p, 'conv1x1.weight')].detach().cpu(), prec)}
    for k in range(1, 6):
        W['w%d' % k] = _round(sd[_key(p, 'conv%d.0.weight' % k)].detach().cpu(), prec)
        W['b%d' % k] = sd[_key(p, 'conv%d.0.bias' % k)].detach().cpu().double()
    return W


def backward_weights(sd, p, prec='fp16'):
    """Forward-shaped (OIHW) weights whose transposes the backward chain's operands hold: 'w1'..'w4', 'w1x1'; 'w5' =
    master x 0.2; 'w5x2' = (conv5's x2 columns + its x4 columns) x 0.2 (the identity path x4 = lrelu(a4) + x2 folded
    in).  prec None: no rounding, float64 throughout."""
    m = lambda name: sd[_key(p, name)].detach().cpu()
    W = {'w1x1': _round(m('conv1x1.weight'), prec)}
    for k in range(1, 5):
        W['w%d' % k] = _round(m('conv%d.0.weight' % k), prec)
    w5 = m('conv5.0.weight')
    if prec is None:
        w5 = w5.double()
        W['w5'], W['w5x2'] = w5 * 0.2, (w5[:, 96:128] + w5[:, 160:192]) * 0.2
    else:
        w5, s = w5.float(), torch.tensor(0.2, dtype=torch.float32)
        W['w5'], W['w5x2'] = _round(w5 * s, prec), _round((w5[:, 96:128] + w5[:, 160:192]) * s, prec)
    return W


def lrelu(a):
    return torch.where(a > 0, a, a * SLOPE)


def lrelu_slope(m):
    """lrelu'(a) given m = (a > 0), float64"""
    one = torch.ones((), dtype=torch.float64)
    return torch.where(m, one, one * SLOPE)


def noise(v, z):
    """GaussianNoise: v (1 + sigma z); z None: off"""
    return v if z is None else v * (1.0 + SIGMA * z.double())


def forward_stages(W, x, x1=None, x2=None, x3=None, x4=None, z1=None, res2=None, z2=None):
    """a1..a5, x1..x4 and y of one dense block.  x1..x4 given: the stage that reads one reads the given values (its own
    output is still returned); None: the reference's own.  z1: the block's noise; res2 (the RRDB input, for the RDB3
    of an RRDB): y = noise2(y * 0.2 + res2)."""
    x = x.double()
    o = {}
    o['a1'] = F.conv2d(x, W['w1'], W['b1'], padding=1)
    o['x1'] = lrelu(o['a1'])
    x1 = o['x1'] if x1 is None else x1.double()
    o['a2'] = F.conv2d(torch.cat((x, x1), 1), W['w2'], W['b2'], padding=1)
    o['x2'] = lrelu(o['a2']) + F.conv2d(x, W['w1x1'])
    x2 = o['x2'] if x2 is None else x2.double()
    o['a3'] = F.conv2d(torch.cat((x, x1, x2), 1), W['w3'], W['b3'], padding=1)
    o['x3'] = lrelu(o['a3'])
    x3 = o['x3'] if x3 is None else x3.double()
    o['a4'] = F.conv2d(torch.cat((x, x1, x2, x3), 1), W['w4'], W['b4'], padding=1)
    o['x4'] = lrelu(o['a4']) + x2
    x4 = o['x4'] if x4 is None else x4.double()
    o['a5'] = F.conv2d(torch.cat((x, x1, x2, x3, x4), 1), W['w5'], W['b5'], padding=1)
    y = noise(o['a5'] * 0.2 + x, z1)
    if res2 is not None:
        y = noise(y * 0.2 + res2.double(), z2)
    o['y'] = y
    return o


def masks_of(stages):
    """m_k = (a_k > 0) of the float64 pre-activations, and per k the elements whose sign a kernel's fp32 sum does not
    pin: |a_k| < MASK_EXCLUDE max|a_k|"""
    m, unsure = {}, {}
    for k in range(1, 5):
        a = stages['a%d' % k]
        m[k] = a > 0
        unsure[k] = a.abs() < MASK_EXCLUDE * a.abs().max()
    return m, unsure


def _ct(g, w, c0, n):
    """conv_k^T restricted to forward input channels [c0, c0 + n): the gradient of that slice"""
    return F.conv_transpose2d(g, w[:, c0:c0 + n], padding=1)


def backward_stages(BW, g_t, m, g_a4=None, g_a3=None, g_x2=None, g_a2=None, g_a1=None,
                    res2=None, z1=None, z2=None, out_a=False):
    """The backward of one dense block from g_t = dL/d(0.2 conv5 + x) and the masks m[1..4] (bool: a_k > 0): g_a4, g_a3,
    the raw g_x2, g_a2, g_a1, g_x, and the exits of esr_rdb_block:
      out_a False: x_out = (g_x [+ res2]) (1 + sigma z1)
      out_a True : A' = (g_x + res2) (1 + sigma z2) -> 'out_a',  x_out = 0.2 A' (1 + sigma z1).
    g_a4 .. g_a1 / g_x2 given: the later stages read the given values.  The LeakyReLU is linear given the mask."""
    d = lambda k: lrelu_slope(m[k])
    g_t = g_t.double()
    o = {}
    o['g_a4'] = _ct(g_t, BW['w5'], 160, 32) * d(4)
    g_a4 = o['g_a4'] if g_a4 is None else g_a4.double()
    o['g_a3'] = (_ct(g_t, BW['w5'], 128, 32) + _ct(g_a4, BW['w4'], 128, 32)) * d(3)
    g_a3 = o['g_a3'] if g_a3 is None else g_a3.double()
    o['g_x2'] = _ct(g_t, BW['w5x2'], 0, 32) + _ct(g_a4, BW['w4'], 96, 32) + _ct(g_a3, BW['w3'], 96, 32)
    o['g_a2'] = o['g_x2'] * d(2)
    g_x2 = o['g_x2'] if g_x2 is None else g_x2.double()
    g_a2 = o['g_a2'] if g_a2 is None else g_a2.double()
    o['g_a1'] = (_ct(g_t, BW['w5'], 64, 32) + _ct(g_a4, BW['w4'], 64, 32) + _ct(g_a3, BW['w3'], 64, 32)
                 + _ct(g_a2, BW['w2'], 64, 32)) * d(1)
    g_a1 = o['g_a1'] if g_a1 is None else g_a1.double()
    o['g_x'] = (g_t + _ct(g_t, BW['w5'], 0, 64) + _ct(g_a4, BW['w4'], 0, 64) + _ct(g_a3, BW['w3'], 0, 64)
                + _ct(g_a2, BW['w2'], 0, 64) + _ct(g_a1, BW['w1'], 0, 64) + F.conv_transpose2d(g_x2, BW['w1x1']))
    v = o['g_x'] if res2 is None else o['g_x'] + res2.double()
    if out_a:
        o['out_a'] = noise(v, z2)
        v = 0.2 * o['out_a']
    o['x_out'] = noise(v, z1)
    return o


def rel_err(got, ref, keep=None):
    """largest |got - ref| over the elements of keep (all: None), relative to the reference's largest magnitude"""
    d = (got.double() - ref.double()).abs()
    if keep is not None:
        d = d * keep
    return d.max().item() / max(ref.abs().max().item(), 1e-30)


# ---- the cases of tests/test_gpu_chain_stages.py, here so that the host test can hold their seeds to MASK_SHARE ------

def randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


TORCH_SEED = 77      # torch.manual_seed before a step: functional._draw_seed's next draw is the step's Philox key
BLOCK_CASES = {
    # name: (module kind, input shape, training mode, weight seed, input seed, gradient seed)
    'a': ('rdb', (1, 64, 5, 3), True, 3, 105, 106),
    'b': ('rrdb_ti', (2, 64, 33, 70), True, 3, 115, 116),
    'd': ('rrdb', (2, 64, 24, 40), False, 3, 125, 126),
}
NET_CASE = dict(cls='RRDB_Net', nb=2, shape=(1, 3, 20, 36), wseed=8, gain=0.7, xseed=135, gseed=136)   # case c
INFER_CASE = dict(shape=(2, 64, 33, 70), wseed=3, xseed=145)                                            # mode 0


def block_module(kind):
    """the module of a block case, on the CPU (weight seed 3, parameters x 1.5: activations of order 1)"""
    from esrganplus_amd import block as B
    torch.manual_seed(3)
    m = B.ResidualDenseBlock_5C(64) if kind == 'rdb' else B.RRDB(64, extra_noise=(kind == 'rrdb_ti'))
    with torch.no_grad():
        for p_ in m.parameters():
            p_.mul_(1.5)
    return m


def block_prefixes(kind):
    return [''] if kind == 'rdb' else ['RDB1', 'RDB2', 'RDB3']


def emulate_blocks(sd, prefixes, x, zs=None, tails=None, z2s=None, prec='fp16'):
    """The blocks at `prefixes` composed with every stored stage rounded to prec — the reference's own stand-in for
    what a chain stores — and per block the share of a1..a4 elements masks_of would leave out.  zs: z1 per block;
    tails: {block index: index of the block whose input is its res2}; z2s: {block index: z2}."""
    shares, xs = [], [_round(x, prec)]
    for n, p in enumerate(prefixes):
        W = forward_weights(sd, p, prec)
        xin = xs[-1]
        s = forward_stages(W, xin)
        x1 = _round(s['x1'], prec)
        s = forward_stages(W, xin, x1)
        x2 = _round(s['x2'], prec)
        s = forward_stages(W, xin, x1, x2)
        x3 = _round(s['x3'], prec)
        s = forward_stages(W, xin, x1, x2, x3)
        x4 = _round(s['x4'], prec)
        res2 = xs[tails[n]] if tails and n in tails else None
        s = forward_stages(W, xin, x1, x2, x3, x4, z1=zs[n] if zs else None, res2=res2, z2=(z2s or {}).get(n))
        _, unsure = masks_of(s)
        shares.append(max(u.double().mean().item() for u in unsure.values()))
        xs.append(_round(s['y'], prec))
    return xs, shares
