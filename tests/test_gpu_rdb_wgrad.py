"""esr_rdb_wgrad_run (csrc/rdb_wgrad.hip): the six weight / bias gradients of a ResidualDenseBlock_5C
(block.py:239-268; autograd's conv backward-weight, SRRaGAN_model.py:140) in one pass, against
 (a) an fp64 torch evaluation of the same sums on the fp16-rounded operands (the oracle of this kernel: a weight
     gradient is a plain correlation, torch.nn.grad-free), and
 (b) the per-conv esr_conv_wgrad launches it replaces;
edge cases: ragged sizes, single rows / columns, several column strips and image groups; run-to-run bit identity;
several blocks through the DEVICE block array with loss scaling and a NULL db; the += contract; several images per task
(what images_per_task() picks once blocks x tasks fill the chip, as at the bench shape) with a ragged last image group;
a capped persistent grid (max_workgroups)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from esrganplus_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


COUTS, CINS = [32, 32, 32, 32, 64, 32], [64, 96, 128, 160, 192, 64]       # conv1..conv5, the 1x1
SLOT = 241856                    # floats of one task's partial sums: the six convs' weights and the five biases
assert SLOT == sum((9 if k < 5 else 1) * co * ci for k, (co, ci) in enumerate(zip(COUTS, CINS))) + sum(COUTS[:5])


def _upload(dev, B, H, W, seed):
    """One (in, q) input pair: the fp32 NCHW tensors and their fp16 G32 buffers."""
    from esrganplus_amd import _lib as L, engine as E
    x = synth.normal_like(seed, 'rw.in', (B, 192, H, W)).to(dev)
    q = (0.05 * synth.normal_like(seed, 'rw.q', (B, 224, H, W))).to(dev)
    bin_, bq = E.G32(B, 192, H, W, 'fp16', dev), E.G32(B, 224, H, W, 'fp16', dev)
    st = E.current_stream()
    for t, g, c in ((x, bin_, 192), (q, bq, 224)):
        lo = L.esr_layout()
        lo.dtype, lo.to_g32, lo.B, lo.C, lo.H, lo.W = L.ESR_F16, 1, B, c, H, W
        lo.nchw, lo.g32 = t.contiguous().data_ptr(), g.view(0, c)
        L.check(L.lib().esr_convert_layout(C.byref(lo), C.c_void_p(st)), 'layout')
    return x, q, bin_, bq


def _outputs(dev, tap_major=False):
    """Zeroed dw[0..5] and db[0..4] of one block; the five db are consecutive slices of one [192] buffer."""
    dws = [torch.zeros((9, co, ci) if tap_major and k < 5 else (co, ci, 3, 3) if k < 5 else (co, ci, 1, 1),
                       dtype=torch.float32, device=dev) for k, (co, ci) in enumerate(zip(COUTS, CINS))]
    dbs = list(torch.zeros(sum(COUTS[:5]), dtype=torch.float32, device=dev).split(COUTS[:5]))
    return dws, dbs


def _launch(dev, B, H, W, blocks, scale=1.0, tap_major=False, max_workgroups=0, skip_db=()):
    """One esr_rdb_wgrad_run over `blocks` = [(in G32, q G32, dws, dbs)]; skip_db: (block, conv) pairs whose db pointer
    is NULL.  Returns the image groups per block that the workspace size implies."""
    from esrganplus_amd import _lib as L, engine as E
    n = len(blocks)
    wbs = (L.esr_rdb_wgrad_block * n)()
    for i, (bin_, bq, dws, dbs) in enumerate(blocks):
        wbs[i].in_, wbs[i].q = bin_.view(0, 192), bq.view(0, 224)
        for k in range(6):
            wbs[i].dw[k] = dws[k].data_ptr()
        for k in range(5):
            wbs[i].db[k] = None if (i, k) in skip_db else dbs[k].data_ptr()
    blk_t = torch.frombuffer(bytearray(bytes(wbs)), dtype=torch.uint8).to(dev)
    need = int(L.lib().esr_rdb_wgrad_workspace_elems(B, H, W, n))
    arena = torch.empty(need, dtype=torch.float32, device=dev)
    rw = L.esr_rdb_wgrad()
    rw.dtype, rw.B, rw.H, rw.W, rw.n_blocks, rw.tap_major = L.ESR_F16, B, H, W, n, 1 if tap_major else 0
    rw.scale5, rw.scale, rw.blocks = 0.2, scale, blk_t.data_ptr()
    rw.partial, rw.partial_elems, rw.max_workgroups = arena.data_ptr(), need, max_workgroups
    L.check(L.lib().esr_rdb_wgrad_run(C.byref(rw), C.c_void_p(E.current_stream())), 'esr_rdb_wgrad_run')
    torch.cuda.synchronize()
    groups, rest = divmod(need - 1024, n * ((W + 31) // 32) * SLOT)
    assert rest == 0, (need, n, W)
    return groups


def _run(dev, B, H, W, seed, tap_major=False):
    x, q, bin_, bq = _upload(dev, B, H, W, seed)
    dws, dbs = _outputs(dev, tap_major)
    _launch(dev, B, H, W, [(bin_, bq, dws, dbs)], tap_major=tap_major)
    return x, q, dws, dbs, (bin_, bq)


def _reference(x, q):
    """fp64 correlation sums on the fp16-rounded operands."""
    xh, qh = x.half().double(), q.half().double()
    gsl = {4: (0, 64, 0.2), 3: (64, 32, 1.0), 2: (96, 32, 1.0), 1: (128, 32, 1.0), 0: (160, 32, 1.0)}   # conv k -> Q slice
    dws, dbs = [], []
    for k in range(5):
        c0, n, sc = gsl[k]
        g = qh[:, c0:c0 + n] * sc
        xin = xh[:, :64 + 32 * k]
        # dW[co, ci, kh, kw] = sum_b,y,x g[b, co, y, x] * xpad[b, ci, y + kh, x + kw]
        xp = F.pad(xin, (1, 1, 1, 1))
        H, W = g.shape[-2:]
        dw = torch.stack([torch.stack([torch.einsum('bohw,bihw->oi', g, xp[:, :, kh:kh + H, kw:kw + W]) for kw in range(3)], -1)
                          for kh in range(3)], -2)
        dws.append(dw)
        dbs.append(g.sum((0, 2, 3)))
    dws.append(torch.einsum('bohw,bihw->oi', qh[:, 192:224], xh[:, :64])[:, :, None, None])
    return dws, dbs


@pytest.mark.parametrize('shape', [(2, 16, 32), (1, 5, 7), (3, 33, 40), (1, 1, 1), (4, 12, 70), (9, 8, 32)])
def test_rdb_wgrad_matches_fp64_correlation(dev, shape):
    B, H, W = shape
    x, q, dws, dbs, _ = _run(dev, B, H, W, seed=3 + H)
    rdw, rdb = _reference(x, q)
    for k in range(6):
        a, r = dws[k].double(), rdw[k]
        err = (a - r).abs().max().item()
        scale = r.abs().max().item() + 1e-12
        # fp32 accumulation of exact fp16 products over B*H*W pixels
        assert err <= 2e-5 * scale + 1e-6, (k, err, scale)
    for k in range(5):
        err = (dbs[k].double() - rdb[k]).abs().max().item()
        assert err <= 2e-5 * (rdb[k].abs().max().item() + 1e-12) + 1e-6, (k, err)


def test_rdb_wgrad_tap_major_and_accumulate(dev):
    """tap_major: 3x3 gradients as [tap][cout][cin] (what esr_grad_unpermute rewrites).  (That a second call adds on
    top: test_rdb_wgrad_second_call_adds_on_top.)"""
    B, H, W = 2, 20, 36
    x, q, dws, dbs, _ = _run(dev, B, H, W, seed=11, tap_major=True)
    rdw, _ = _reference(x, q)
    for k in range(5):
        want = rdw[k].permute(2, 3, 0, 1).reshape(9, rdw[k].shape[0], rdw[k].shape[1])
        assert (dws[k].double() - want).abs().max().item() <= 2e-5 * want.abs().max().item() + 1e-6, k
    assert (dws[5].double() - rdw[5]).abs().max().item() <= 2e-5 * rdw[5].abs().max().item() + 1e-6


def test_rdb_wgrad_is_bit_identical_run_to_run_and_matches_per_conv_launches(dev):
    from esrganplus_amd import _lib as L, engine as E
    B, H, W = 4, 32, 64
    outs = [_run(dev, B, H, W, seed=21) for _ in range(2)]
    for a, b in zip(outs[0][2] + outs[0][3], outs[1][2] + outs[1][3]):
        assert torch.equal(a, b)
    # the per-conv fp16 kernel on the same G32 tensors (atomics: compare to rounding)
    x, q, dws, dbs, (bin_, bq) = outs[0]
    st = E.current_stream()
    spec = [(0, 160, 32, 64, 3, 1.0), (1, 128, 32, 96, 3, 1.0), (2, 96, 32, 128, 3, 1.0), (3, 64, 32, 160, 3, 1.0),
            (4, 0, 64, 192, 3, 0.2), (5, 192, 32, 64, 1, 1.0)]
    for k, c0, co, ci, ks, sc in spec:
        wg = L.esr_wgrad()
        wg.dtype, wg.ks, wg.stride, wg.upsample = L.ESR_F16, ks, 1, 0
        wg.B, wg.H, wg.W, wg.cout, wg.cin = B, H, W, co, ci
        wg.g, wg.in_ = bq.view(c0, co), bin_.view(0, ci)
        dw = torch.zeros((co, ci, ks, ks), dtype=torch.float32, device=dev)
        db = torch.zeros(co, dtype=torch.float32, device=dev)
        wg.dw, wg.dbias, wg.scale = dw.data_ptr(), (db.data_ptr() if k < 5 else None), sc
        L.check(L.lib().esr_conv_wgrad(C.byref(wg), C.c_void_p(st)), 'esr_conv_wgrad')
        torch.cuda.synchronize()
        assert (dw - dws[k]).abs().max().item() <= 1e-5 * dw.abs().max().item() + 1e-6, k
        if k < 5:
            assert (db - dbs[k]).abs().max().item() <= 1e-5 * db.abs().max().item() + 1e-6, k


def _check_block(dws, dbs, rdw, rdb, scale, what, skip_db=()):
    """every dw / db of one block against scale x the fp64 correlation, the bound of
    test_rdb_wgrad_matches_fp64_correlation: fp32 accumulation of exact fp16 products"""
    for k in range(6):
        r = rdw[k] * scale
        err = (dws[k].double() - r).abs().max().item()
        assert err <= 2e-5 * (r.abs().max().item() + 1e-12) + 1e-6, (what, 'dw', k, err)
    for k in range(5):
        if k in skip_db:
            continue
        r = rdb[k] * scale
        err = (dbs[k].double() - r).abs().max().item()
        assert err <= 2e-5 * (r.abs().max().item() + 1e-12) + 1e-6, (what, 'db', k, err)


def _many_blocks(dev, B, H, W, n_blocks, seed, **kw):
    """n_blocks blocks with their own dw / db over three input pairs in turn (three fp64 references, not n_blocks).
    Returns (outputs per block, the three pairs, image groups per block)."""
    pairs = [_upload(dev, B, H, W, seed + j) for j in range(3)]
    outs = [_outputs(dev) for _ in range(n_blocks)]
    blocks = [pairs[i % 3][2:] + outs[i] for i in range(n_blocks)]
    groups = _launch(dev, B, H, W, blocks, **kw)
    return outs, pairs, groups


def test_rdb_wgrad_three_blocks_loss_scale_and_null_db(dev):
    """Block indexing into the device array, scale != 1, and db[k] == NULL: conv2's bias gradient of block 1 is skipped
    and the buffer that would have received it (between that block's db of conv1 and conv3) keeps its sentinel."""
    B, H, W, scale, skip = 2, 5, 40, 0.5, (1, 1)
    pairs = [_upload(dev, B, H, W, 40 + j) for j in range(3)]
    outs = [_outputs(dev) for _ in range(3)]
    outs[skip[0]][1][skip[1]].fill_(123.0)
    groups = _launch(dev, B, H, W, [pairs[i][2:] + outs[i] for i in range(3)], scale=scale, skip_db=[skip])
    assert groups == B                                         # one image per task here
    for i in range(3):
        rdw, rdb = _reference(*pairs[i][:2])
        _check_block(outs[i][0], outs[i][1], rdw, rdb, scale, 'block %d' % i, skip_db=[skip[1]] if i == skip[0] else ())
    assert bool((outs[skip[0]][1][skip[1]] == 123.0).all())


@pytest.mark.parametrize('tap_major', [False, True])
def test_rdb_wgrad_second_call_adds_on_top(dev, tap_major):
    """dw / db are accumulated (+=): the pass is deterministic, so a second call into the same buffers leaves exactly
    s + s = 2 s (exact in fp32)."""
    B, H, W = 2, 20, 36
    x, q, bin_, bq = _upload(dev, B, H, W, 11)
    dws, dbs = _outputs(dev, tap_major)
    _launch(dev, B, H, W, [(bin_, bq, dws, dbs)], tap_major=tap_major)
    first = [t.clone() for t in dws + dbs]
    assert all(bool(t.any()) for t in first)
    _launch(dev, B, H, W, [(bin_, bq, dws, dbs)], tap_major=tap_major)
    for a, b in zip(first, dws + dbs):
        assert torch.equal(b, 2 * a)


# n_blocks, (B, H, W), images per task, image groups: shapes at which images_per_task() (csrc/rdb_wgrad.hip) leaves one
# image per task behind, n_blocks * 4 * strips * ceil(B / (2 ipw)) >= 1024, with a last group of ONE image
IPW_CASES = [(43, (5, 3, 40), 2, 3), (128, (9, 2, 8), 8, 2)]


@pytest.mark.parametrize('case', IPW_CASES, ids=lambda c: '%dblocks-ipw%d' % (c[0], c[2]))
def test_rdb_wgrad_several_images_per_task(dev, case):
    n_blocks, (B, H, W), ipw, groups = case
    assert (B + ipw - 1) // ipw == groups and B % ipw == 1
    outs, pairs, got_groups = _many_blocks(dev, B, H, W, n_blocks, seed=60 + n_blocks)
    assert got_groups == groups                                # the workspace says: `ipw` images per task
    refs = [_reference(x, q) for x, q, _, _ in pairs]
    for i in range(n_blocks):
        _check_block(outs[i][0], outs[i][1], *refs[i % 3], 1.0, 'block %d' % i)


def test_rdb_wgrad_capped_grid_is_bit_identical(dev):
    """max_workgroups = 32: a persistent grid strides over the tasks; slots are per task and reduced in a fixed order,
    so nothing changes."""
    n_blocks, (B, H, W), _, groups = IPW_CASES[0]
    a, _, ga = _many_blocks(dev, B, H, W, n_blocks, seed=60 + n_blocks)
    b, _, gb = _many_blocks(dev, B, H, W, n_blocks, seed=60 + n_blocks, max_workgroups=32)
    assert ga == gb == groups
    for i in range(n_blocks):
        for s, t in zip(a[i][0] + a[i][1], b[i][0] + b[i][1]):
            assert torch.equal(s, t)
    assert bool(a[0][0][0].any())
