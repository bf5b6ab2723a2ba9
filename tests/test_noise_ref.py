"""CPU tests of tests/noise_ref.py, the reference the GPU noise tests compare with: Philox known answers, the position
rules of the contract in include/comms_hip.h, the statistics of its normal values, and a symbol-level BPSK link against
the closed-form bit-error rate.  No GPU."""
import math

import numpy as np
import pytest

import noise_ref as nr

# Random123's known-answer set for philox4x32 10, first three lines: (counter, key, output)
KATS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_philox_known_answers():
    for ctr, key, want in KATS:
        got = tuple(int(x[0]) for x in nr.philox4x32_10(ctr, key))
        assert got == want, [hex(v) for v in got]


def test_word_stream_layout():
    # block b -> words 4b ... 4b+3; key = seed halves, counter = (b lo, b hi, stream lo, stream hi)
    w = nr.words(0, 0, 0, 4)
    assert tuple(int(v) for v in w) == KATS[0][2]
    # a block whose index needs the high counter word
    b = (1 << 40) + 5
    want = nr.philox4x32_10((b & nr.MASK32, b >> 32, 7, 9), (3, 4))
    got = nr.words((4 << 32) | 3, (9 << 32) | 7, 4 * b + 1, 3)
    assert [int(v) for v in got] == [int(want[i][0]) for i in (1, 2, 3)]
    # any window of the stream is the same words
    whole = nr.words(11, 3, 0, 1000)
    for p, n in ((0, 1), (1, 1), (3, 6), (5, 995), (998, 2)):
        assert np.array_equal(nr.words(11, 3, p, n), whole[p:p + n])


def test_position_rules_and_cut_invariance():
    rng = np.random.default_rng(1)
    seed, stream = 99, 5
    # bits: ceil(n / 32) words per draw; cuts at multiples of 32 give the uncut stream; LSB first
    s = nr.Source(seed, stream)
    a = s.bits(1000)
    assert s.pos == 32
    w = nr.words(seed, stream, 0, 32)
    assert all(a[i] == (int(w[i // 32]) >> (i % 32)) & 1 for i in range(1000))
    s = nr.Source(seed, stream)
    assert np.array_equal(np.concatenate([s.bits(64), s.bits(320), s.bits(616)]), a)
    s = nr.Source(seed, stream)
    assert np.array_equal(np.unpackbits(s.bits(1000, packed=True), bitorder="little")[:1000], a)
    s = nr.Source(seed, stream)
    assert s.bits(33).size == 33 and s.pos == 2
    # uniform and normal: n words, any cut
    for kind in ("uniform", "normal"):
        s = nr.Source(seed, stream, pos=3)
        whole = getattr(s, kind)(501)
        assert s.pos == 504
        s = nr.Source(seed, stream, pos=3)
        cuts = np.sort(rng.choice(np.arange(1, 501), 7, replace=False))
        parts = [getattr(s, kind)(n) for n in np.diff(np.concatenate([[0], cuts, [501]]))]
        if kind == "uniform":
            assert np.array_equal(np.concatenate([p[1] for p in parts]), whole[1])
        else:
            assert np.array_equal(np.concatenate(parts), whole)
    # a normal value at an odd word is the sine of the pair that started one word earlier
    z = nr.Source(seed, stream).normal(8)
    assert np.array_equal(nr.Source(seed, stream, pos=5).normal(3), z[5:8])
    # complex draws: the position first goes to an even word, then 2 words per sample
    s = nr.Source(seed, stream, pos=7)
    g = s.complex_normal(10)
    assert s.pos == 28
    zz = nr.Source(seed, stream, pos=8).normal(20)
    assert np.array_equal(g, zz[0::2] + 1j * zz[1::2])
    s = nr.Source(seed, stream, pos=8)
    assert np.array_equal(np.concatenate([s.complex_normal(3), s.complex_normal(1), s.complex_normal(6)]), g)
    # shard [a, b) of an AWGN stream that started at even p0: set_pos(p0 + 2a)
    x = rng.standard_normal(10) + 1j * rng.standard_normal(10)
    whole = nr.Source(seed, stream, pos=8).awgn(x, 0.5)
    assert np.array_equal(nr.Source(seed, stream, pos=8 + 2 * 4).awgn(x[4:], 0.5), whole[4:])
    # skip(n) equals drawing and discarding
    s1, s2 = nr.Source(seed, stream), nr.Source(seed, stream)
    s1.normal(77)
    s2.skip(77)
    assert s1.pos == s2.pos and np.array_equal(s1.normal(5), s2.normal(5))
    # the position wraps modulo 2^64: word 2^64 - 1 is followed by word 0
    s = nr.Source(1, 0, pos=(1 << 64) - 2)
    assert np.array_equal(s.normal(6), np.concatenate([nr.Source(1, 0, (1 << 64) - 2).normal(2), nr.Source(1, 0).normal(4)]))
    assert s.pos == 4 and nr.Source(1, 0, pos=(1 << 64) - 2).skip(5).pos == 3
    # different streams differ
    assert not np.array_equal(nr.words(seed, 0, 0, 8), nr.words(seed, 1, 0, 8))


def test_uniform_stays_in_range():
    f32 = np.float32
    one_up = np.nextafter(f32(1.0), f32(2.0))
    for lo, hi in ((0.0, 1.0), (-3.5, 2.25), (1.0, one_up), (1e-30, 3e38), (-3e38, 3e38)):
        exact, f = nr.Source(7, 1).uniform(1 << 16, lo, hi)
        assert f.dtype == np.float32
        assert np.all(f >= f32(lo)) and np.all(f < f32(hi)), (lo, hi)
        assert np.all(exact >= np.float64(f32(lo))) and np.all(exact < np.float64(f32(hi)))
    # u = 1 - 2^-24 at bounds one ulp apart rounds to hi, and is replaced by lo (the float below hi)
    _, f = nr.Source(7, 1).uniform(1 << 16, 1.0, one_up)
    assert set(np.unique(f)) == {f32(1.0)}


def _phi(x):
    import torch

    return (0.5 * torch.erfc(-torch.from_numpy(x) / math.sqrt(2.0))).numpy()


def test_normal_statistics_2p24():
    """Moments, correlations and the Kolmogorov-Smirnov distance of 2^24 values of (seed 12345, stream 7).  The standard
    errors are those of n independent standard normal values: mean 1/sqrt(n), variance sqrt(2/n), skewness sqrt(6/n), excess
    kurtosis sqrt(24/n), a correlation coefficient 1/sqrt(n).  Bounds: 4 standard errors; KS * sqrt(n) <= 1.63 (the 1 % point)."""
    n = 1 << 24
    z = nr.Source(12345, 7).normal(n)
    m, v = z.mean(), z.var()
    c = z - m
    skew = np.mean(c ** 3) / v ** 1.5
    kurt = np.mean(c ** 4) / v ** 2 - 3.0
    re_im = np.mean(z[0::2] * z[1::2])          # the cosine and the sine of one pair
    lag1 = np.mean(z[:-1] * z[1:])
    stats = {"mean": m * math.sqrt(n), "variance": (v - 1.0) / math.sqrt(2.0 / n), "skewness": skew / math.sqrt(6.0 / n),
             "excess kurtosis": kurt / math.sqrt(24.0 / n), "re/im correlation": re_im * math.sqrt(n / 2),
             "lag-1 correlation": lag1 * math.sqrt(n - 1)}
    zs = np.sort(z)
    cdf = _phi(zs)
    i = np.arange(1, n + 1, dtype=np.float64)
    ks = max(np.max(i / n - cdf), np.max(cdf - (i - 1) / n)) * math.sqrt(n)
    zmax = np.max(np.abs(z))
    print("standard errors:", {k: round(float(s), 3) for k, s in stats.items()}, "KS*sqrt(n) = %.3f" % ks, "max |z| = %.4f" % zmax)
    for name, s in stats.items():
        assert abs(s) <= 4.0, (name, s)
    assert ks <= 1.63, ks
    assert zmax <= math.sqrt(48.0 * math.log(2.0))  # the tail ends at 5.77 sigma


@pytest.mark.parametrize("ebn0_db", [0, 4, 7, 9])
def test_symbol_level_bpsk_matches_the_closed_form(ebn0_db):
    n = 1 << 23
    errors, n_bits, _ = nr.symbol_link_bpsk(n, ebn0_db, seed=2024, stream=ebn0_db)
    p = 0.5 * math.erfc(math.sqrt(10.0 ** (ebn0_db / 10.0)))
    z = (errors - n_bits * p) / math.sqrt(n_bits * p * (1.0 - p))
    print("Eb/N0 %d dB: %d errors, expected %.1f, z = %.2f" % (ebn0_db, errors, n_bits * p, z))
    assert abs(z) <= 4.0, (errors, n_bits * p, z)


def test_sample_level_link_without_noise_has_no_errors():
    rng = np.random.default_rng(3)
    sps, n_sym = 8, 4096
    t = (np.arange(65) - 32) / sps
    taps = np.sinc(t) * np.hanning(67)[1:-1]  # any Nyquist-like pulse will do here
    for k in (1, 2):
        bits = rng.integers(0, 2, n_sym * k)
        errors, n_cmp, d = nr.sample_link(bits, k, taps, sps, 4000.0, 0.0, np.zeros(n_sym * sps, np.complex128))
        assert errors == 0 and n_cmp == (n_sym - 8) * k and d.shape == (n_sym - 8, k)


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("sigma", nr.LINK_SIGMAS)
def test_link_noise_levels_keep_the_gpu_link_test_honest(k, sigma):
    """tests/test_gpu_noise.py asserts |E_gpu - E_ref| <= m, m the reference decisions within delta of the threshold.  That
    says something only while m is small: m <= 1e-3 of the symbols and m < E_ref / 4, checked here for the reference alone at
    the test's size, taps and noise levels (2^-17 and 1e-5 are the accuracy and parity tolerances the GPU test uses)."""
    import __graft_entry__ as g

    g.build()
    import comms_rs_amd as c

    n_sym = 1 << 18
    h = c.rrc_taps(nr.LINK_TAPS, float(nr.LINK_SPS), nr.LINK_BETA).real.astype(np.float64)  # host code: no GPU needed
    scale = nr.link_scale(h, k)
    bits = nr.Source(5, k).bits(n_sym * k)
    noise = nr.Source(6, 100 + k).complex_normal(n_sym * nr.LINK_SPS)
    wire = nr.tx_wire(bits, k, h, nr.LINK_SPS, scale)
    e_ref, n_cmp, d = nr.sample_link(bits, k, h, nr.LINK_SPS, scale, sigma, noise, wire=wire)
    rx_max = float(np.max(np.abs(wire))) / scale + sigma * max(np.max(np.abs(noise.real)), np.max(np.abs(noise.imag)))
    delta = nr.link_delta(h, sigma, noise, rx_max, 2.0 ** -17, 1e-5)
    m = int(np.count_nonzero(np.abs(d) < delta))
    print("k=%d sigma=%.2f: E_ref=%d of %d bits (%.2e), m=%d, delta=%.3e" % (k, sigma, e_ref, n_cmp, e_ref / n_cmp, m, delta))
    assert m <= 1e-3 * n_sym and m < e_ref / 4
    # and the error rate is the matched-filter bound's: Q(sqrt(sum h^2) / sigma) per bit, within 4 binomial deviations plus
    # the few percent the truncated RRC's inter-symbol interference adds
    p = 0.5 * math.erfc(math.sqrt(np.sum(h * h)) / sigma / math.sqrt(2.0))
    assert abs(e_ref - n_cmp * p) <= 4.0 * math.sqrt(n_cmp * p) + 0.1 * n_cmp * p
