"""The z of the fused GaussianNoise stream (csrc/common.h: philox4x32, philox_normal8), stated independently in numpy:
Philox-4x32 (Salmon, Moraes, Dror, Shaw, SC'11) in uint64 arithmetic with the round count as a parameter, then a float64
Box-Muller on 16-bit halves of each output word.  Element (b, c, y, x) of noise layer `layer` under `seed`:
  counter = (pixel index (b H + y) W + x, c // 8, layer, 0),  key = (seed low word, seed high word),
  word k = (c % 8) // 2:  u0 = ((word >> 16) + 1) / 2^16 in (0, 1],  u1 = (word & 0xffff) / 2^16 turns,
  z = sqrt(-2 ln u0) * (cos if c even else sin)(2 pi u1).
tests/test_noise_refs.py pins the generator at 10 rounds to the published Random123 known answers."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
LO = np.uint64(0xFFFFFFFF)
ROUNDS = 7                       # ESR_PHILOX_ROUNDS


def philox4x32(ctr, key, rounds=10):
    """ctr: four uint32 arrays (broadcastable), key: two integers.  Returns the four output words as uint64 arrays
    holding 32-bit values."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) & LO for c in ctr])
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    s32 = np.uint64(32)
    for _ in range(rounds):
        p0, p1 = M0 * c0, M1 * c2                       # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & LO, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & LO
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def normal(shape, seed, layer, rounds=ROUNDS):
    """float64 [B][C][H][W] z of (seed, layer)"""
    B, C_, H, W = shape
    noct = (C_ + 7) // 8
    pix = np.arange(B * H * W, dtype=np.uint64).reshape(B, 1, H, W)
    octs = np.arange(noct, dtype=np.uint64).reshape(1, noct, 1, 1)
    words = philox4x32((pix, octs, np.uint64(layer), np.uint64(0)), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF), rounds)
    z = np.empty((B, noct, 8, H, W), dtype=np.float64)
    for k, r in enumerate(words):
        u0 = ((r >> np.uint64(16)) + np.uint64(1)).astype(np.float64) / 65536.0
        ang = (r & np.uint64(0xFFFF)).astype(np.float64) * (2.0 * np.pi / 65536.0)
        rad = np.sqrt(-2.0 * np.log(u0))
        z[:, :, 2 * k] = rad * np.cos(ang)
        z[:, :, 2 * k + 1] = rad * np.sin(ang)
    return z.reshape(B, noct * 8, H, W)[:, :C_]
