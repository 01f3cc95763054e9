"""What a packed weight arena should hold (csrc/aux_kernels.hip: pack_kernel, pack_batch_kernel), stated twice over:
the DENSE OPERAND of every esr_pack mode — the [rows][K][taps] matrix the MFMA conv multiplies with, written from the
semantics in include/esrgan_hip.h — and ONE permutation, ``to_fragments``, from a dense operand to the bytes of
  [cout_block][K chunk][kh][kw][lane 0..63][16 B].
Pure numpy / torch on the CPU.  The builders compute in the dtype of the weights they are given: float32 for the byte
comparison on the GPU (the packer's own arithmetic: one or a few fp32 adds in a stated order, one fp32 multiply, then
to_fragments' one rounding to the storage type), float64 for tests/test_pack_refs.py, which pins every operand to the
convolution it stands for."""
import numpy as np
import torch
import torch.nn.functional as F

SENTINEL = 0xA5
CPG = {'fp16': 16, 'fp32': 8}                   # K indices per chunk (two lane halves of 16 bytes each)
NP_DTYPE = {'fp16': np.float16, 'fp32': np.float32}


def pi_table():
    """pi[i]: the row (within its block of 32) that packed A row i holds.  The C/D map of v_mfma_*_32x32 puts result
    row (r & 3) + 8 (r >> 2) + 4 h into accumulator register r of lane half h (csrc/common.h); the epilogue wants that
    register to be cout 16 h + r, so that a lane's 16 registers are 16 consecutive channels."""
    pi = [None] * 32
    for h in range(2):
        for r in range(16):
            pi[(r & 3) + 8 * (r >> 2) + 4 * h] = 16 * h + r
    return pi


def fragment_values(A, dtype):
    """[cout_blocks][chunks][taps][64][EPL] values (in the storage type) of the dense operand A [rows][K][taps]: lane
    32 h + i, element e = A[32 cb + pi(i)][chunk * CPG + EPL * h + e][tap]; rows and K indices past A's are zero."""
    A = np.asarray(A, dtype=np.float32)
    rows, K, taps = A.shape
    cpg = CPG[dtype]
    epl = cpg // 2
    cbs, nch = (rows + 31) // 32, (K + cpg - 1) // cpg
    P = np.zeros((cbs * 32, nch * cpg, taps), dtype=np.float32)
    P[:rows, :K] = A
    P = P.reshape(cbs, 32, nch, cpg, taps)
    out = np.zeros((cbs, nch, taps, 64, epl), dtype=np.float32)
    pi = pi_table()
    for h in range(2):
        for i in range(32):
            for e in range(epl):
                out[:, :, :, 32 * h + i, e] = P[:, pi[i], :, epl * h + e, :]
    return out.astype(NP_DTYPE[dtype])           # fp16: round to nearest even, subnormals kept


def to_fragments(A, dtype):
    """The byte image (uint8, 1 KB per fragment) of the dense operand A [rows][K][taps]."""
    return np.ascontiguousarray(fragment_values(A, dtype)).view(np.uint8).reshape(-1)


# ---- dense operands.  w: OIHW weights [cout][cin][ks][ks] of the FORWARD conv (numpy, float32 or float64) --------------

def _taps(a):
    return np.ascontiguousarray(a).reshape(a.shape[0], a.shape[1], -1)


def plain(w):
    """forward conv: row = cout, K = cin"""
    return _taps(w)


def transposed(w, mode=1, sum=None):
    """esr_pack.transpose_flip: row = forward cin, K = forward cout; mode 1 rotates the taps by 180 degrees (the
    input-gradient conv), mode 2 keeps them (the operand of the transposed stride-2 conv).  sum = (dst, src, count):
    rows [dst, dst + count) additionally receive the weights of forward input channels [src, src + count)."""
    a = w.transpose(1, 0, 2, 3)
    if mode == 1:
        a = a[:, :, ::-1, ::-1]
    a = a.copy()
    if sum is not None:
        dst, src, n = sum
        n = min(n, a.shape[0] - dst)                          # (rows past the forward cin do not exist)
        a[dst:dst + n] = a[dst:dst + n] + a[src:src + n]
    return _taps(a)


UPS_DGRAD_ROWS = ((2,), (1, 2), (0, 1), (0,))    # 4x4 tap k collects these forward 3x3 rows (same for columns)


def ups_dgrad(w):
    """esr_pack.ups_dgrad: the 4x4 / stride 2 / pad 1 conv over g that is the adjoint of nearest-x2 + 3x3 conv; row =
    forward cin, K = forward cout; each tap sums its forward taps rows first, then columns."""
    cout, cin = w.shape[:2]
    a = np.zeros((cin, cout, 4, 4), dtype=w.dtype)
    for kh, rs in enumerate(UPS_DGRAD_ROWS):
        for kw, cs in enumerate(UPS_DGRAD_ROWS):
            s = np.zeros((cout, cin), dtype=w.dtype)
            for r in rs:
                for c in cs:
                    s = s + w[:, :, r, c]
            a[:, :, kh, kw] = s.T
    return _taps(a)


SUBPIX_ROWS = {0: ((0, 0), (1, 2)), 1: ((0, 1), (2, 2))}     # phase d: 3x3 rows summed into 2x2 tap 0 / 1


def subpix_taps(w):
    """[4][cout][cin][2][2] pre-summed taps of esr_pack.ups_fwd in w's dtype (a torch tensor), summed in the packer's
    order"""
    k = torch.zeros((4,) + tuple(w.shape[:2]) + (2, 2), dtype=w.dtype)
    for dy in (0, 1):
        for dx in (0, 1):
            for a, (r0, r1) in enumerate(SUBPIX_ROWS[dy]):
                for b, (c0, c1) in enumerate(SUBPIX_ROWS[dx]):
                    s = torch.zeros(w.shape[:2], dtype=w.dtype)
                    for r in range(r0, r1 + 1):
                        for c in range(c0, c1 + 1):
                            s = s + w[:, :, r, c]
                    k[2 * dy + dx, :, :, a, b] = s
    return k


def subpix_conv(x, k):
    """output pixel (2y+dy, 2x+dx) = 2x2 conv of phase (dy, dx) over input rows y-1+dy.., columns x-1+dx.."""
    B, _, h, w = x.shape
    out = torch.zeros(B, k.shape[1], 2 * h, 2 * w, dtype=x.dtype)
    xp = F.pad(x, (1, 1, 1, 1))
    for dy in (0, 1):
        for dx in (0, 1):
            out[:, :, dy::2, dx::2] = F.conv2d(xp, k[2 * dy + dx])[:, :, dy:dy + h, dx:dx + w]
    return out


def ups_fwd(w):
    """esr_pack.ups_fwd: four 2x2 operands [phase = 2 dy + dx][cout][cin][2 a + b], one per output phase"""
    return [_taps(k) for k in subpix_taps(torch.from_numpy(np.ascontiguousarray(w))).numpy()]


def ups_fwd_fragments(w, dtype):
    """phase-major: [phase][cout_block][chunk][2 a + b] fragments"""
    return np.concatenate([to_fragments(a, dtype) for a in ups_fwd(w)])


def gather_piece(w, src_co0, dst_cout, scale, fold_co0=0):
    """One esr_pack.gather piece, [dst_cout][forward couts][9]: row r is forward input channel src_co0 + r, K index c
    forward output channel c, taps rotated by 180 degrees, (+ the weights of input channel fold_co0 + r,) times
    float32(scale), rounded to w's dtype; a 1x1 kernel sits at the centre tap."""
    cout, _, ks, _ = w.shape
    sl = lambda c0: w[:, c0:c0 + dst_cout].transpose(1, 0, 2, 3)
    a = np.zeros((dst_cout, cout, 3, 3), dtype=w.dtype)
    if ks == 3:
        a[:] = sl(src_co0)[:, :, ::-1, ::-1]
        if fold_co0 > 0:
            a = a + sl(fold_co0)[:, :, ::-1, ::-1]
    else:
        a[:, :, 1, 1] = sl(src_co0)[:, :, 0, 0]
    return _taps(a * w.dtype.type(np.float32(scale)))


def gather_operand(dst_cout, pieces):
    """The whole gather-form operand of a slice: its pieces' K ranges end to end.  pieces: (w, src_co0, scale[, fold_co0])
    as packs.DgradPack takes them, w as numpy arrays."""
    return np.concatenate([gather_piece(pc[0], pc[1], dst_cout, pc[2], *pc[3:]) for pc in pieces], axis=1)


def one_t_channel(k):
    """esr_pack.one_t: the g_x2 channel at packed K index k = 16 c + 8 h + e (chunk c, lane half h, element e)"""
    c, h, e = k // 16, (k // 8) % 2, k % 8
    return 16 * h + 8 * c + e


def one_t(w1x1):
    """The transposed 1x1 of a dense block in the backward chain's K order, [64][32][1]: row = x channel"""
    w = w1x1.reshape(w1x1.shape[0], w1x1.shape[1])            # [32 g_x2 channels][64 x channels]
    return np.stack([w[one_t_channel(k)] for k in range(32)], axis=1)[:, :, None]
