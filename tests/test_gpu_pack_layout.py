"""The packed weight arena byte for byte (csrc/aux_kernels.hip: pack_kernel, pack_batch_kernel) against
tests/pack_refs.py: the dense operand of every esr_pack mode, written from include/esrgan_hip.h and pinned to the
convolution it stands for by tests/test_pack_refs.py, pushed through ONE fragment permutation.  Every entry goes through
both launches — esr_pack_conv_weights and a esr_pack_conv_weights_batch built with _lib.batch_pack_op — into an arena
pre-filled with 0xA5 that has room for ceil(max(cin, cout) / 32) cout blocks of the entry: the entry must be the
reference's bytes and every other byte must still be the sentinel.

Every expectation is bit-exact: the packer's arithmetic is at most a few fp32 adds in a stated order (sum_*, fold_co0,
ups_*), one fp32 multiply (gather scale) and one round-to-nearest-even conversion, and the reference does the same in
numpy float32 / astype(float16).  No mode needed a tolerance.  (fp16 gather pieces with scale = 0.2 did not match at
first, in the last bit of one or two weights per entry: the compiler had fused multiply and conversion into one
v_fma_mixlo_f16 — one rounding of the exact product instead of two — for two of a lane's eight elements only.  The
packer now keeps the two roundings apart for every element.)"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import pack_refs as P

pytestmark = pytest.mark.gpu

SENT = P.SENTINEL
TAIL = 4096                      # sentinel bytes past the generous size


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def weights(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * 0.1


def esr_pack_of(w, dtype, **fields):
    """w: contiguous fp32 OIHW on the device"""
    from esrganplus_amd import _lib as L, packs
    assert w.is_cuda and w.dtype == torch.float32 and w.is_contiguous()
    pk = L.esr_pack()
    pk.src, pk.cout, pk.cin, pk.ks, pk.dtype = w.data_ptr(), w.shape[0], w.shape[1], w.shape[2], packs._dt(dtype)[0]
    for k, v in fields.items():
        setattr(pk, k, v)
    return pk


def run(how, dev, cap, entries):
    """entries: [(esr_pack, byte offset of its dst in the arena)].  Returns the arena's `cap` bytes."""
    from esrganplus_amd import _lib as L, engine as E
    st = C.c_void_p(E.current_stream())
    arena = torch.full((cap,), SENT, dtype=torch.uint8, device=dev)
    for pk, off in entries:
        pk.dst = arena.data_ptr() + off
    if how == 'single':
        for pk, _ in entries:
            L.check(L.lib().esr_pack_conv_weights(C.byref(pk), st), 'esr_pack_conv_weights')
    else:
        bp, keep = L.batch_pack_op([pk for pk, _ in entries], dev)
        L.check(L.lib().esr_pack_conv_weights_batch(C.byref(bp), st), 'esr_pack_conv_weights_batch')
    torch.cuda.synchronize()
    return arena.cpu().numpy()


def expectation(cap, placed):
    """(want, owned): the arena image and the mask of the bytes the entries own.  placed: [(offset, bytes)]"""
    want, owned = np.full(cap, SENT, dtype=np.uint8), np.zeros(cap, dtype=bool)
    for off, b in placed:
        assert off + b.size <= cap and not owned[off:off + b.size].any()
        want[off:off + b.size] = b
        owned[off:off + b.size] = True
    return want, owned


def check(got, want, owned, what):
    bad = np.flatnonzero((got != want) & owned)
    assert bad.size == 0, '%s: %d packed bytes differ from the reference, first at byte %d' % (what, bad.size, bad[0])
    assert np.array_equal(got[owned], want[owned])
    hit = np.flatnonzero((got != SENT) & ~owned)
    assert hit.size == 0, '%s: %d bytes written outside the entry, first at byte %d (entry bytes: %d)' % (
        what, hit.size, hit[0], owned.sum())


def check_both_launches(dev, cap, entries, placed, what):
    want, owned = expectation(cap, placed)
    got = {how: run(how, dev, cap, entries) for how in ('single', 'batch')}
    for how in ('single', 'batch'):
        check(got[how], want, owned, '%s, %s launch' % (what, how))
    assert np.array_equal(got['single'], got['batch'])


def generous(entry_bytes, cout, cin):
    return entry_bytes * ((max(cout, cin) + 31) // 32) + TAIL


# mode -> (esr_pack fields, reference bytes of (OIHW numpy weights, dtype))
MODES = {
    'plain': ({}, lambda w, dt: P.to_fragments(P.plain(w), dt)),
    'tflip1': (dict(transpose_flip=1), lambda w, dt: P.to_fragments(P.transposed(w, 1), dt)),
    'tflip2': (dict(transpose_flip=2), lambda w, dt: P.to_fragments(P.transposed(w, 2), dt)),
    'sum': (dict(transpose_flip=1, sum_dst=32, sum_src=0, sum_count=32),
            lambda w, dt: P.to_fragments(P.transposed(w, 1, (32, 0, 32)), dt)),
    'ups_dgrad': (dict(transpose_flip=1, ups_dgrad=1, ks=4), lambda w, dt: P.to_fragments(P.ups_dgrad(w), dt)),
    'ups_fwd': (dict(ups_fwd=1), P.ups_fwd_fragments),
}

# mode, cout, cin, ks of the weights
CASES = [
    ('plain', 3, 8, 3), ('plain', 32, 24, 3), ('plain', 40, 64, 3),      # fp16: the batch kernel's vectorised path —
    #                       ragged cout (zero rows), a last half chunk past cin (zero fill), a second cout block
    ('plain', 32, 12, 3), ('plain', 5, 3, 3),                            # cin & 7: the per-piece path in the batch kernel
    ('plain', 64, 64, 1), ('plain', 32, 16, 4),
    ('tflip1', 48, 40, 3), ('tflip1', 48, 40, 1), ('tflip2', 48, 40, 4),
    ('sum', 64, 48, 3),              # rows 32..47 (the forward cin ends there) receive input channels 0..15
    ('sum', 48, 64, 3),              # cin 64, cout 48 as in test_gpu_conv_backward's f16_sum_fold: all 32 rows folded
    ('ups_dgrad', 32, 24, 3), ('ups_dgrad', 3, 64, 3),
    ('ups_fwd', 32, 24, 3), ('ups_fwd', 3, 64, 3),
]
FAST = {(3, 8), (32, 24), (40, 64)}


def takes_fast_path(pk):
    """the condition of pack_batch_kernel's hand-vectorised branch"""
    from esrganplus_amd import _lib as L
    return (pk.dtype == L.ESR_F16 and pk.ks == 3 and not (pk.transpose_flip or pk.gather or pk.ups_fwd or pk.one_t)
            and pk.cin & 7 == 0 and pk.src & 15 == 0)


@pytest.mark.parametrize('dtype', ['fp16', 'fp32'])
@pytest.mark.parametrize('case', CASES, ids=lambda c: '%s-%dx%d-k%d' % c)
def test_packed_bytes_are_the_reference_bytes(dev, case, dtype):
    mode, cout, cin, ks = case
    fields, ref = MODES[mode]
    w = weights((cout, cin, ks, ks), 100 + CASES.index(case))
    wd = w.to(dev)
    pk = esr_pack_of(wd, dtype, **fields)
    assert takes_fast_path(pk) == (mode == 'plain' and ks == 3 and dtype == 'fp16' and (cout, cin) in FAST)
    want = ref(w.numpy(), dtype)
    check_both_launches(dev, generous(want.size, cout, cin), [(pk, 0)], [(0, want)], '%s %s' % (case, dtype))


def test_misaligned_source_leaves_the_fast_path_and_still_matches(dev):
    """(32, 24) would take the vectorised branch; its source starts 4 bytes into an allocation, so the 16-byte loads
    are not possible and the batch kernel must take the per-piece path"""
    w = weights((32, 24, 3, 3), 300)
    big = torch.zeros(w.numel() + 8, dtype=torch.float32, device=dev)
    assert big.data_ptr() & 15 == 0
    wd = big[1:1 + w.numel()].view(w.shape)
    wd.copy_(w)
    pk = esr_pack_of(wd, 'fp16')
    assert pk.src & 15 == 4 and not takes_fast_path(pk)
    want = P.to_fragments(P.plain(w.numpy()), 'fp16')
    check_both_launches(dev, generous(want.size, 32, 24), [(pk, 0)], [(0, want)], 'misaligned source')


def test_mixed_batch_seams_off_the_workgroup_grid(dev):
    """Four entries in one batch launch — vectorised, per-piece fp16, fp32, ups_fwd — whose piece_begin values are no
    multiples of the 256-thread workgroup: the entry search and the local piece index at every seam (and the groups of
    nine threads of the vectorised path across them).  1 KB of sentinel between the entries."""
    from esrganplus_amd import _lib as L
    spec = [('fp16', (32, 24, 3, 3), {}, lambda w: P.to_fragments(P.plain(w), 'fp16')),
            ('fp16', (5, 3, 3, 3), {}, lambda w: P.to_fragments(P.plain(w), 'fp16')),
            ('fp32', (32, 16, 4, 4), {}, lambda w: P.to_fragments(P.plain(w), 'fp32')),
            ('fp16', (3, 64, 3, 3), dict(ups_fwd=1), lambda w: P.ups_fwd_fragments(w, 'fp16'))]
    entries, placed, keep, off, begin = [], [], [], 0, 0
    for n, (dtype, shape, fields, ref) in enumerate(spec):
        w = weights(shape, 400 + n)
        keep.append(w.to(dev))
        pk = esr_pack_of(keep[-1], dtype, **fields)
        want = ref(w.numpy())
        assert L.lib().esr_pack_pieces(C.byref(pk)) * 16 == want.size
        assert n == 0 or begin % 256 != 0, (n, begin)
        entries.append((pk, off))
        placed.append((off, want))
        off += want.size + 1024
        begin += want.size // 16
    assert begin % 256 != 0
    assert [takes_fast_path(pk) for pk, _ in entries] == [True, False, False, False]
    check_both_launches(dev, off + TAIL, entries, placed, 'mixed batch')


def gather_piece_placed(pk, piece, dtype):
    """[(offset, bytes)] of one gather piece: chunks [dst_chunk0, ..) of every cout block of the entry"""
    w, src_co0, scale = piece[:3]
    frag = P.fragment_values(P.gather_piece(w.detach().cpu().numpy(), src_co0, pk.dst_cout, scale, *piece[3:]), dtype)
    cbs, nch = frag.shape[:2]
    assert cbs == (pk.dst_cout + 31) // 32 and pk.dst_chunk0 + nch <= pk.dst_nchunks
    return [((cb * pk.dst_nchunks + pk.dst_chunk0) * 9 * 1024, np.ascontiguousarray(frag[cb]).view(np.uint8).reshape(-1))
            for cb in range(cbs)]


@pytest.mark.parametrize('dtype', ['fp16', 'fp32'])
def test_dense_block_gather_operands(dev, dtype):
    """The gather-form operands of one ResidualDenseBlock_5C(64) as production builds them (block._rdb_gathers through
    packs.DgradPack): .g4 .g3 .g2 .g1 .g0 .c2 .c0 and, in fp16, the transposed 1x1 .o1 — scale 0.2 on conv5's pieces,
    fold_co0 = 160 in .c2, the 1x1 at the centre tap of .g0, pieces at nonzero dst_chunk0.  First the whole arena of the
    pack's own batch launch, then every piece alone through both launches: the chunks of the entry that the piece
    does not own, and the cout blocks a forward-cin-sized grid would reach, keep the sentinel."""
    from esrganplus_amd import _lib as L, block as B, engine as E
    torch.manual_seed(5)
    m = B.ResidualDenseBlock_5C(64)
    with torch.no_grad():
        for p in m.parameters():
            p.normal_(0.0, 0.1)                                # (on the CPU: the same weights everywhere)
    m = m.to(dev)
    specs = B._rdb_gathers('rdb', m)
    assert [s[0] for s in specs] == ['rdb.' + k for k in ('g4', 'g3', 'g2', 'g1', 'g0', 'c2', 'c0', 'o1')]
    pack = E.DgradPack([], dtype, dev, {}, specs)
    pack.ensure(E.current_stream())
    torch.cuda.synchronize()
    arena, base = pack.arena.cpu().numpy(), pack.arena.data_ptr()
    seen = 0
    for key, dst_cout, pieces in specs:
        if dst_cout == 'one_t':
            if dtype != 'fp16':
                continue
            want = P.to_fragments(P.one_t(pieces.detach().cpu().numpy()), dtype)
        else:
            want = P.to_fragments(P.gather_operand(dst_cout, [(pc[0].detach().cpu().numpy(),) + tuple(pc[1:])
                                                              for pc in pieces]), dtype)
        off = pack.entries[key].w_ptr - base
        assert off == seen, key
        bad = np.flatnonzero(arena[off:off + want.size] != want)
        assert bad.size == 0, '%s: %d bytes differ, first at %d' % (key, bad.size, bad[0])
        seen += want.size
    assert seen == arena.size

    pks = pack._packs()
    flat = [(key, dst_cout, pc) for key, dst_cout, pieces in specs if dst_cout != 'one_t' for pc in pieces]
    assert len(pks) == len(flat) + (dtype == 'fp16') and all(pk.gather for pk in pks[:len(flat)])
    assert {pk.fold_co0 for pk in pks} == {0, 160} and any(pk.src_ks == 1 and pk.dst_chunk0 > 0 for pk in pks)
    for pk, (key, dst_cout, pc) in zip(pks, flat):
        entry = L.packed_weight_bytes(dst_cout, pk.dst_nchunks * pack.cpg, 3, pack.esr_dtype)
        what = '%s piece at chunk %d (%s)' % (key, pk.dst_chunk0, dtype)
        check_both_launches(dev, generous(entry, pk.cout, pk.cin), [(pk, 0)], gather_piece_placed(pk, pc, dtype), what)
    if dtype == 'fp16':
        pk, w1 = pks[-1], specs[-1][2]
        assert pk.one_t == 1
        want = P.to_fragments(P.one_t(w1.detach().cpu().numpy()), dtype)
        assert want.size == 4096
        check_both_launches(dev, generous(want.size, 64, 64), [(pk, 0)], [(0, want)], 'one_t')
