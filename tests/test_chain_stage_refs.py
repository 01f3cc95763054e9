"""tests/chain_stage_refs.py pinned before it judges a kernel (no GPU): composed without any rounding, the forward stages
are oracle.ref_torch's dense block / RRDB in float64 and the backward stages are torch autograd through them — noise
on and off, the RRDB tail of both variants, the trunk exit with a skip gradient (out_a); two defects of the kind the
GPU test is for move a stage by far more than its bound; and the seeds of the GPU cases keep the share of elements whose
mask the reference cannot pin under its limit."""
import pytest
import torch

from oracle import ref_torch as RT
from tests import chain_stage_refs as R
from tests import noise_refs as NR

TOL = 1e-12
GPU_BOUND = 1.5e-3          # tests/test_gpu_chain_stages.py, fp16


def rel(a, b):
    return (a - b).abs().max().item() / b.abs().max().item()


def rrdb_sd(seed, prefix='t.0'):
    torch.manual_seed(seed)
    sd = {}
    for j in (1, 2, 3):
        p = '%s.RDB%d' % (prefix, j)
        sd[p + '.conv1x1.weight'] = torch.randn(32, 64, 1, 1, dtype=torch.float64) * 0.12
        for k in range(1, 6):
            cin, cout = 64 + 32 * (k - 1), 64 if k == 5 else 32
            sd[p + '.conv%d.0.weight' % k] = torch.randn(cout, cin, 3, 3, dtype=torch.float64) * (1.5 / (9 * cin) ** 0.5)
            sd[p + '.conv%d.0.bias' % k] = torch.randn(cout, dtype=torch.float64) * 0.1
    return sd


def zd(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize('noisy', [False, True])
def test_block_stages_equal_the_oracle_and_autograd(noisy):
    shape = (2, 64, 9, 11)
    sd, p = rrdb_sd(1), 't.0.RDB2'
    x = zd(shape, 2).requires_grad_(True)
    gy = zd(shape, 3)
    z = zd(shape, 4) if noisy else None
    y = RT.rdb_forward(x, sd, p, z)
    gx, = torch.autograd.grad((y * gy).sum(), x)
    W = R.forward_weights(sd, p, None)
    xs = x.detach().clone().requires_grad_(True)
    s = R.forward_stages(W, xs, z1=z)
    assert rel(s['y'].detach(), y.detach()) <= TOL
    ga = torch.autograd.grad((s['y'] * gy).sum(), [s['a%d' % k] for k in range(1, 5)] + [xs])
    m, _ = R.masks_of(s)
    b = R.backward_stages(R.backward_weights(sd, p, None), R.noise(gy, z), m)
    for k in range(1, 5):
        assert rel(b['g_a%d' % k], ga[k - 1]) <= TOL, k
    assert rel(b['g_x'], gx) <= TOL and rel(b['g_x'], ga[4]) <= TOL
    assert torch.equal(b['x_out'], b['g_x']) and 'out_a' not in b
    # raw g_x2 = g_a2 before its mask
    assert torch.equal(b['g_a2'], b['g_x2'] * R.lrelu_slope(m[2]))


@pytest.mark.parametrize('variant', ['codes', 'test_image'])
@pytest.mark.parametrize('noisy', [False, True])
def test_two_rrdbs_equal_the_oracle_and_autograd(variant, noisy):
    """Two RRDBs in a row, as the trunk runs them: the forward tail (res2, layer2) and every backward exit — plain,
    with the skip gradient added (the first block of the last RRDB to run), and with out_a (the RDB1 of RRDB 1, whose
    exit passes through the tail of RRDB 0)."""
    shape = (1, 64, 8, 10)
    sd = dict(rrdb_sd(5, 't.0'), **rrdb_sd(6, 't.1'))
    x = zd(shape, 7).requires_grad_(True)
    gy = zd(shape, 8)
    z1 = {(i, j): zd(shape, 10 + 3 * i + j) if noisy else None for i in range(2) for j in range(3)}
    z2 = {i: zd(shape, 20 + i) if (noisy and variant == 'test_image') else None for i in range(2)}
    t = x
    for i in range(2):
        t = RT.rrdb_forward(t, sd, 't.%d' % i, [z1[(i, j)] for j in range(3)] if noisy else None, z2[i])
    gx, = torch.autograd.grad((t * gy).sum(), x)
    # forward, block by block
    stages, u = {}, x.detach()
    for i in range(2):
        x_rrdb = u
        for j in range(3):
            W = R.forward_weights(sd, 't.%d.RDB%d' % (i, j + 1), None)
            stages[(i, j)] = R.forward_stages(W, u, z1=z1[(i, j)], res2=x_rrdb if j == 2 else None, z2=z2[i])
            u = stages[(i, j)]['y']
    assert rel(u, t.detach()) <= TOL
    # backward: entry through the tail of RRDB 1, then the six blocks
    A = R.noise(gy, z2[1])
    g_t = R.noise(0.2 * A, z1[(1, 2)])
    for i in (1, 0):
        for j in (2, 1, 0):
            m, _ = R.masks_of(stages[(i, j)])
            BW = R.backward_weights(sd, 't.%d.RDB%d' % (i, j + 1), None)
            if j > 0:
                b = R.backward_stages(BW, g_t, m, z1=z1[(i, j - 1)])
            elif i > 0:
                b = R.backward_stages(BW, g_t, m, res2=A, z1=z1[(i - 1, 2)], z2=z2[i - 1], out_a=True)
                A = b['out_a']
            else:
                b = R.backward_stages(BW, g_t, m, res2=A)
            g_t = b['x_out']
    assert rel(g_t, gx) <= TOL, rel(g_t, gx)


def test_defects_move_a_stage_by_ten_bounds():
    """the references have teeth at the GPU bound: one halo column of x2 missing from a tile's x3, and g_x2 stored after
    its mask instead of before"""
    kind, shape, _, _, xseed, gseed = R.BLOCK_CASES['b']
    sd = R.block_module(kind).state_dict()
    W = R.forward_weights(sd, 'RDB1', 'fp16')
    x = R.randn(shape, xseed)
    s = R.forward_stages(W, x)
    x2_cut = s['x2'].clone()
    x2_cut[:, :, 0:16, 32] = 0                                   # what the tile at (0, 0) takes from its right neighbour
    bad = s['x3'].clone()
    bad[:, :, 0:16, 31] = R.forward_stages(W, x, s['x1'], x2_cut)['x3'][:, :, 0:16, 31]
    assert R.rel_err(bad, s['x3']) >= 10 * GPU_BOUND
    m, _ = R.masks_of(s)
    b = R.backward_stages(R.backward_weights(sd, 'RDB1'), R.randn(shape, gseed), m)
    assert R.rel_err(b['g_a2'], b['g_x2']) >= 10 * GPU_BOUND


def philox_seed(torch_seed):
    torch.manual_seed(torch_seed)
    return int(torch.randint(0, 2 ** 62, (1,)).item())


def z_of(shape, seed, layer):
    return None if layer is None else torch.from_numpy(NR.normal(shape, seed, layer))


@pytest.mark.parametrize('case', sorted(R.BLOCK_CASES))
def test_block_cases_keep_the_excluded_share(case):
    kind, shape, train, _, xseed, _ = R.BLOCK_CASES[case]
    sd = R.block_module(kind).state_dict()
    pre = R.block_prefixes(kind)
    seed = philox_seed(R.TORCH_SEED)
    zs = [z_of(shape, seed, j) for j in range(len(pre))] if train else None
    z2s = {2: z_of(shape, seed, 3)} if (train and kind == 'rrdb_ti') else None
    _, shares = R.emulate_blocks(sd, pre, R.randn(shape, xseed), zs, {2: 0} if len(pre) == 3 else None, z2s)
    print('case %s: excluded share per block %s' % (case, ['%.2e' % s for s in shares]))
    assert max(shares) <= R.MASK_SHARE


def test_net_and_inference_cases_keep_the_excluded_share():
    import torch.nn.functional as F
    from esrganplus_amd import synth
    c = R.NET_CASE
    sd = synth.rrdbnet_state_dict(nb=c['nb'], seed=c['wseed'], gain=c['gain'])
    x = synth.image_batch(c['xseed'], *c['shape'], name='stages.x')
    q = lambda t_: t_.half().double()
    fea = q(F.conv2d(q(x), q(sd['model.0.weight']), sd['model.0.bias'].double(), padding=1))
    shape = (c['shape'][0], 64) + tuple(c['shape'][2:])
    seed = philox_seed(R.TORCH_SEED)
    pre = ['model.1.sub.%d.RDB%d' % (i, j) for i in range(c['nb']) for j in (1, 2, 3)]
    zs = [z_of(shape, seed, 4 * (n // 3) + n % 3) for n in range(len(pre))]
    z2s = {3 * i + 2: z_of(shape, seed, 4 * i + 3) for i in range(c['nb'])}
    _, shares = R.emulate_blocks(sd, pre, fea, zs, {3 * i + 2: 3 * i for i in range(c['nb'])}, z2s)
    assert max(shares) <= R.MASK_SHARE, shares
    c = R.INFER_CASE
    sd = R.block_module('rdb').state_dict()
    for prec in ('fp16', 'fp32'):
        _, shares = R.emulate_blocks(sd, [''], R.randn(c['shape'], c['xseed']), prec=prec)
        assert max(shares) <= R.MASK_SHARE, (prec, shares)
