"""tests/noise_refs.py pinned on the host: Philox-4x32 at 10 rounds against the three known answers published with
Random123 (kat_vectors: philox4x32 10), the Box-Muller's range and moments, and the round count the library uses — a
5-round stream fails the channel-correlation band tests/test_gpu_forward.py: test_philox_stream_statistics holds the
device stream to (its next Philox call, 8 channels on, is visibly correlated); 7 rounds pass it."""
import numpy as np

from tests import noise_refs as NR

KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_philox_known_answers():
    for ctr, key, want in KAT:
        got = tuple(int(w) for w in NR.philox4x32(ctr, key, 10))
        assert got == want, (['%08x' % g for g in got], ['%08x' % w for w in want])
    # all three at once, as arrays
    ctr = [np.array([k[0][i] for k in KAT], dtype=np.uint64) for i in range(4)]
    for n, (_, key, want) in enumerate(KAT):
        got = NR.philox4x32(ctr, key, 10)
        assert tuple(int(w[n]) for w in got) == want
    assert tuple(int(w) for w in NR.philox4x32(*KAT[2][:2], 7)) != KAT[2][2]


def test_counter_layout_and_box_muller():
    """element (b, c, y, x) depends on its own coordinates only: a crop / another batch size / fewer channels reproduce
    the same values; layer and both key words matter; |z| <= sqrt(-2 ln 2^-16)"""
    seed = (0x1234 << 32) | 0x89abcdef
    z = NR.normal((2, 20, 5, 70), seed, 91)
    assert z.shape == (2, 20, 5, 70) and np.isfinite(z).all()
    assert np.array_equal(z[:1, :9], NR.normal((1, 9, 5, 70), seed, 91))
    one = NR.philox4x32((np.uint64((1 * 5 + 3) * 70 + 69), np.uint64(2), np.uint64(91), np.uint64(0)), (0x89abcdef, 0x1234), 7)
    r = int(one[1])                                                # channel 19 = octet 2, element 3: word 1, the sine
    want = np.sqrt(-2 * np.log(((r >> 16) + 1) / 65536.0)) * np.sin(2 * np.pi * (r & 0xffff) / 65536.0)
    assert z[1, 19, 3, 69] == want
    for other in (NR.normal((2, 20, 5, 70), seed, 0), NR.normal((2, 20, 5, 70), seed ^ (1 << 40), 91),
                  NR.normal((2, 20, 5, 70), seed ^ 1, 91)):
        assert np.abs(other - z).max() > 1.0
    assert np.abs(z).max() <= 4.7096


def _corr(a, b):
    return abs(float((a * b).mean() / (a.std() * b.std())))


def test_five_rounds_fail_the_correlation_band_seven_pass():
    shape = (4, 64, 96, 128)                                       # the shape and band of test_philox_stream_statistics
    n = int(np.prod(shape))
    lim = 5 / (n / 2) ** 0.5
    z7, z5 = NR.normal(shape, 12345, 3, 7), NR.normal(shape, 12345, 3, 5)
    c7, c5 = _corr(z7[:, :-8], z7[:, 8:]), _corr(z5[:, :-8], z5[:, 8:])
    print('lag-8 channel correlation: 7 rounds %.2e, 5 rounds %.2e, band %.2e' % (c7, c5, lim))
    assert c7 < lim
    assert c5 > 4 * lim                                            # 20 sigma
    m1, m2 = z7.mean(), (z7 * z7).mean()
    assert abs(m1) < 4 / n ** 0.5 and abs(m2 - 1) < 6 / n ** 0.5
