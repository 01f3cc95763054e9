"""The dense operands of tests/pack_refs.py against the convolutions they stand for, in float64 on the CPU with torch's
own conv2d / conv_transpose2d / autograd, and the fragment permutation as a bijection.  tests/test_gpu_pack_layout.py
then compares the packer's bytes with these operands bit for bit."""
import types

import numpy as np
import torch
import torch.nn.functional as F

from tests import pack_refs as P

TOL = 1e-12


def rnd(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def as_conv(a, ks):
    """a dense operand [rows][K][taps] as a conv2d weight"""
    return torch.from_numpy(np.ascontiguousarray(a)).reshape(a.shape[0], a.shape[1], ks, ks)


def close(got, want):
    return (got - want).abs().max().item() <= TOL * want.abs().max().item()


def test_plain_operand_is_the_conv_weight():
    w = rnd((5, 7, 3, 3), 1)
    assert torch.equal(as_conv(P.plain(w.numpy()), 3), w)


def test_transpose_flip_1_is_the_input_gradient_conv():
    for ks in (3, 1):
        w, g = rnd((6, 5, ks, ks), 2), rnd((2, 6, 7, 9), 3)
        got = F.conv2d(g, as_conv(P.transposed(w.numpy(), 1), ks), padding=ks // 2)
        assert close(got, F.conv_transpose2d(g, w, padding=ks // 2))


def test_transpose_flip_2_is_the_transposed_stride_2_conv():
    """rows <-> K swapped, taps kept: operand[ci][co] IS conv_transpose2d's weight [co][ci], and that conv is the input
    gradient of the 4x4 / stride 2 forward conv"""
    w, g = rnd((6, 5, 4, 4), 4), rnd((2, 6, 3, 4), 5)
    a = as_conv(P.transposed(w.numpy(), 2), 4)
    got = F.conv_transpose2d(g, a.transpose(0, 1), stride=2, padding=1)
    x = torch.zeros(2, 5, 6, 8, dtype=torch.float64, requires_grad=True)
    (want,) = torch.autograd.grad(F.conv2d(x, w, stride=2, padding=1), x, g)
    assert close(got, want)


def test_sum_operand_folds_the_identity_path():
    """x4 = lrelu(a4) + x2: the gradient of channels [dst, dst + n) also collects that of channels [src, src + n)"""
    w, g = rnd((6, 12, 3, 3), 6), rnd((1, 6, 5, 6), 7)
    dst, src, n = 4, 8, 4
    got = F.conv2d(g, as_conv(P.transposed(w.numpy(), 1, (dst, src, n)), 3), padding=1)
    want = F.conv_transpose2d(g, w, padding=1)
    want[:, dst:dst + n] += want[:, src:src + n]
    assert close(got, want)


def test_ups_dgrad_operand_is_the_adjoint_of_nearest_x2_conv3():
    w, g = rnd((4, 5, 3, 3), 8), rnd((2, 4, 6, 10), 9)
    x = torch.zeros(2, 5, 3, 5, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(F.interpolate(x, scale_factor=2, mode='nearest'), w, padding=1)
    (want,) = torch.autograd.grad(y, x, g)
    got = F.conv2d(g, as_conv(P.ups_dgrad(w.numpy()), 4), stride=2, padding=1)
    assert close(got, want)


def test_ups_fwd_phases_are_nearest_x2_conv3():
    w, x = rnd((5, 7, 3, 3), 10), rnd((2, 7, 5, 6), 11)
    k = torch.stack([as_conv(a, 2) for a in P.ups_fwd(w.numpy())])
    want = F.conv2d(F.interpolate(x, scale_factor=2, mode='nearest'), w, padding=1)
    assert close(P.subpix_conv(x, k), want)


def fake_rdb(seed):
    """what block._rdb_gathers reads of a ResidualDenseBlock_5C(64): conv1..conv5[0].weight and conv1x1.weight"""
    m = types.SimpleNamespace(conv1x1=types.SimpleNamespace(weight=rnd((32, 64, 1, 1), seed)))
    for k in range(1, 6):
        w = rnd((64 if k == 5 else 32, 64 + 32 * (k - 1), 3, 3), seed + k)
        setattr(m, 'conv%d' % k, [types.SimpleNamespace(weight=w)])
    return m


def test_gather_operands_are_the_sums_of_the_later_convs_input_gradients():
    """Every gather spec of a dense block (block._rdb_gathers): one conv over the concatenated gradients = the sum over
    the pieces of conv_k^T restricted to the slice, times the piece's scale, the folded columns added."""
    from esrganplus_amd import block as B
    specs = [s for s in B._rdb_gathers('rdb', fake_rdb(20)) if s[1] != 'one_t']
    assert [s[0] for s in specs] == ['rdb.g4', 'rdb.g3', 'rdb.g2', 'rdb.g1', 'rdb.g0', 'rdb.c2', 'rdb.c0']
    folds = 0
    for n, (key, dst_cout, pieces) in enumerate(specs):
        gs = [rnd((1, pc[0].shape[0], 4, 5), 40 + 7 * n + j) for j, pc in enumerate(pieces)]
        a = P.gather_operand(dst_cout, [(pc[0].numpy(),) + tuple(pc[1:]) for pc in pieces])
        got = F.conv2d(torch.cat(gs, 1), as_conv(a, 3), padding=1)
        want = torch.zeros_like(got)
        for g, pc in zip(gs, pieces):
            w, co0, scale = pc[:3]
            cols = w[:, co0:co0 + dst_cout]
            if len(pc) > 3:
                cols = cols + w[:, pc[3]:pc[3] + dst_cout]
                folds += 1
            want += F.conv_transpose2d(g, cols, padding=w.shape[2] // 2) * float(np.float32(scale))
        assert close(got, want), key
    assert folds == 1                                        # .c2: conv5's x4 columns on its x2 columns


def test_one_t_operand_is_the_transposed_1x1_in_the_chain_k_order():
    w = rnd((32, 64, 1, 1), 30).numpy()
    a = P.one_t(w)
    order = [P.one_t_channel(k) for k in range(32)]
    assert sorted(order) == list(range(32))
    # chunk c of lane half h holds the eight channels 16 h + 8 c .. + 7 (include/esrgan_hip.h: esr_pack.one_t)
    assert order == [16 * h + 8 * c + e for c in range(2) for h in range(2) for e in range(8)]
    undone = np.zeros((64, 32))
    undone[:, order] = a[:, :, 0]
    assert np.array_equal(undone, w[:, :, 0, 0].T)


def test_pi_gives_every_lane_half_16_consecutive_couts():
    pi = P.pi_table()
    assert sorted(pi) == list(range(32))
    for h in range(2):
        for r in range(16):                                  # accumulator register r of half h = MFMA result row ...
            assert pi[(r & 3) + 8 * (r >> 2) + 4 * h] == 16 * h + r
    assert pi[:8] == [0, 1, 2, 3, 16, 17, 18, 19]


def test_to_fragments_is_a_bijection_onto_the_operand():
    for dtype, shape in (('fp16', (40, 20, 2)), ('fp32', (40, 20, 2)), ('fp16', (3, 8, 9)), ('fp32', (33, 9, 1))):
        rows, K, taps = shape
        a = np.arange(1, rows * K * taps + 1, dtype=np.float32).reshape(shape)       # distinct, exact in fp16 (<= 2048)
        v = P.fragment_values(a, dtype)
        cpg = P.CPG[dtype]
        cbs, nch = (rows + 31) // 32, (K + cpg - 1) // cpg
        assert v.shape == (cbs, nch, taps, 64, cpg // 2)
        assert P.to_fragments(a, dtype).size == cbs * nch * taps * 1024
        flat = v.astype(np.float64).reshape(-1)
        assert sorted(flat[flat != 0].tolist()) == list(range(1, a.size + 1))        # every element exactly once
        assert (flat == 0).sum() == flat.size - a.size                               # the rest is padding
        # and each one where the header says: lane 32 h + i, element e of fragment (cb, chunk, tap)
        pi = P.pi_table()
        for cb, chunk, tap, lane, e in [(0, 0, 0, 0, 0), (cbs - 1, nch - 1, taps - 1, 63, cpg // 2 - 1), (0, nch - 1, 0, 37, 1)]:
            h, i = lane // 32, lane % 32
            r, k = 32 * cb + pi[i], chunk * cpg + (cpg // 2) * h + e
            assert v[cb, chunk, tap, lane, e] == (a[r, k, tap] if r < rows and k < K else 0)
