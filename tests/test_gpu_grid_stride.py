"""The second-tier kernels past the point where their grid stops growing.

fir_exact_kernel<double2>, fir_exact_kernel<short2>, fmdemod_f64_kernel, the wire-format converters of iqformat.hip and estimator_kernel all launch
min(ceil(n / 256), 8 * kNumCU) workgroups of 256 lanes and walk the rest of the batch in grid-stride rounds.  Below T work
items there is one round and the `r * stride` / `i += stride` arithmetic never runs; the estimator's four-accumulator main
loop needs more than 3 T terms to run at all.  Every test here sits on or beyond T and compares EVERY output with the oracle:
bit for bit where the node promises the reference's bits (f64 and i16 FIR / pulse, the converters), at the existing bounds
where it promises rounding-level agreement (f64 FM demod 1e-12, estimators 1e-9).

The estimator bound of 1e-9 is only worth something if the oracle's sequential fold is itself far more accurate than that
on the inputs used: test_estimator_oracle_fold_is_accurate_on_these_inputs (CPU, no GPU needed) holds it to 1e-10 of an
extended-precision sum for every input and length the device test uses."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
from test_estimators import psk_stream, qam16_stream

# The grid cap: 8 * kNumCU workgroups (kNumCU = 256, csrc/common.hpp) of 256 lanes -- run_dev<V> (fir_exact.hip, both sample
# types), comms_fmdemod_f64_run_dev (fft_f64.hip), conv_grid (iqformat.hip), estimate (estimators.hip).
T = 8 * 256 * 256
SIZES = (T - 1, T, T + 1, 2 * T + 3, 3 * T + 1)   # one round to the brim, one lane into the second, three and four rounds
HEAD = 1077                                        # a short first call: the seam to the long call is no multiple of 256


@pytest.fixture(scope="module")
def c():
    import comms_rs_amd as c

    assert c.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested (no CPU fallback)"
    return c


def ok(status):
    assert status == 0, "comms_status_t %d" % status


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def rand_c128(rng, n, scale=1.0):
    return (scale * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex128)


def rand_i16(rng, n):
    return rng.integers(-32768, 32768, (n, 2), dtype=np.int16)   # full range: nearly every product wraps


def on_device(run_dev, x, n_out, out_dtype, out_cols=None):
    """run_dev(in_ptr, out_ptr, stream) on torch copies of x; returns the output as numpy."""
    import torch

    xd = torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")
    yd = torch.empty((n_out,) if out_cols is None else (n_out, out_cols), dtype=out_dtype, device="cuda:0")
    run_dev(xd.data_ptr(), yd.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return yd.cpu().numpy()


# ------------------------------------------------------------------ f64 FIR and pulse: the reference's bits
@pytest.mark.gpu
@pytest.mark.parametrize("n,n_taps", [(T - 1, 7), (T, 31), (T + 1, 63), (2 * T + 3, 15), (3 * T + 1, 33),
                                      (T + 1, 2050)])   # 2050 taps: two passes over the LDS tap window AND two rounds
def test_batch_fir_f64_past_the_grid_cap(c, n, n_taps):
    """A short call, then n samples in one call (host form and device form, a node each), then the state: all of it the
    oracle's bits.  The long call starts from a non-zero history and every round r > 0 re-stages the taps."""
    import torch

    rng = np.random.default_rng(n % 1000 + n_taps)
    taps = rand_c128(rng, n_taps, 0.3)
    x = rand_c128(rng, HEAD + n)
    ost = oracle.default_state(taps)
    want = [oracle.batch_fir(x[:HEAD], taps, ost), oracle.batch_fir(x[HEAD:], taps, ost)]
    host, dev = c.BatchFirNodeF64(taps), c.BatchFirNodeF64(taps)
    for k, (a, b) in enumerate(((0, HEAD), (HEAD, HEAD + n))):
        assert np.array_equal(bits(host.run(x[a:b])), bits(want[k])), ("host", k)
        got = on_device(lambda i, o, s: dev.run_dev(i, b - a, o, s), x[a:b], b - a, torch.complex128)
        assert np.array_equal(bits(got), bits(want[k])), ("dev", k)
    assert np.array_equal(bits(host.state(n_taps)), bits(ost))
    assert np.array_equal(bits(dev.state(n_taps)), bits(ost))


# n_out = n_sym * sps must land on the sizes: T - 1 = 2^19 - 1 is prime (sps 1 only), T + 1 = 3 * 174763,
# 2 T + 3 = 7 * 149797, 3 T + 1 = 5 * 314573 -- 3, 5 and 7 do not divide T, so i / sps and i % sps differ from round to round
PULSE_CASES = [(T - 1, 1, 7), (T, 4, 63), (T + 1, 3, 40), (2 * T + 3, 7, 20), (3 * T + 1, 5, 31)]


@pytest.mark.gpu
@pytest.mark.parametrize("n_out,sps,n_taps", PULSE_CASES + [(T + 1, 3, 2050)])
def test_pulse_f64_past_the_grid_cap(c, n_out, sps, n_taps):
    import torch

    assert n_out % sps == 0
    n_sym = n_out // sps
    rng = np.random.default_rng(n_out % 1000 + sps)
    taps = rand_c128(rng, n_taps, 0.2)
    sym = rand_c128(rng, 333 + n_sym + 50)
    ost = oracle.default_state(taps)
    cuts = ((0, 333), (333, 333 + n_sym), (333 + n_sym, sym.size))   # the last call shows the state the long one left
    host, dev = c.PulseNodeF64(taps, sps), c.PulseNodeF64(taps, sps)
    for a, b in cuts:
        want = oracle.pulse(sym[a:b], taps, sps, ost)
        assert want.size == (b - a) * sps
        assert np.array_equal(bits(host.run(sym[a:b])), bits(want)), ("host", a, b)
        got = on_device(lambda i, o, s: dev.run_dev(i, b - a, o, s), sym[a:b], (b - a) * sps, torch.complex128)
        assert np.array_equal(bits(got), bits(want)), ("dev", a, b)


# ------------------------------------------------------------------ i16 FIR and pulse: wrapping arithmetic, the same bits
@pytest.mark.gpu
@pytest.mark.parametrize("n,n_taps", [(T - 1, 7), (T, 31), (T + 1, 63), (2 * T + 3, 15), (3 * T + 1, 33),
                                      (T + 1, 4100)])   # 4100 taps: two passes over the LDS tap window AND two rounds
def test_batch_fir_i16_past_the_grid_cap(c, n, n_taps):
    import torch

    rng = np.random.default_rng(n % 1000 + n_taps + 1)
    taps = rand_i16(rng, n_taps)
    x = rand_i16(rng, HEAD + n)
    ost = np.zeros_like(taps)
    want = [oracle.batch_fir(x[:HEAD], taps, ost), oracle.batch_fir(x[HEAD:], taps, ost)]
    host, dev = c.BatchFirNodeI16(taps), c.BatchFirNodeI16(taps)
    for k, (a, b) in enumerate(((0, HEAD), (HEAD, HEAD + n))):
        assert np.array_equal(host.run(x[a:b]), want[k]), ("host", k)
        got = on_device(lambda i, o, s: dev.run_dev(i, b - a, o, s), x[a:b], b - a, torch.int16, 2)
        assert np.array_equal(got, want[k]), ("dev", k)
    assert np.array_equal(host.state(n_taps), ost)
    assert np.array_equal(dev.state(n_taps), ost)


@pytest.mark.gpu
@pytest.mark.parametrize("n_out,sps,n_taps", PULSE_CASES + [(T + 1, 3, 4100)])
def test_pulse_i16_past_the_grid_cap(c, n_out, sps, n_taps):
    import torch

    assert n_out % sps == 0
    n_sym = n_out // sps
    rng = np.random.default_rng(n_out % 1000 + sps + 1)
    taps = rand_i16(rng, n_taps)
    sym = rand_i16(rng, 333 + n_sym + 50)
    ost = np.zeros_like(taps)
    host, dev = c.PulseNodeI16(taps, sps), c.PulseNodeI16(taps, sps)
    for a, b in ((0, 333), (333, 333 + n_sym), (333 + n_sym, sym.shape[0])):
        want = oracle.pulse(sym[a:b], taps, sps, ost)
        assert want.shape == ((b - a) * sps, 2)
        assert np.array_equal(host.run(sym[a:b]), want), ("host", a, b)
        got = on_device(lambda i, o, s: dev.run_dev(i, b - a, o, s), sym[a:b], (b - a) * sps, torch.int16, 2)
        assert np.array_equal(got, want), ("dev", a, b)


# ------------------------------------------------------------------ f64 FM demod
@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_fmdemod_f64_past_the_grid_cap(c, n):
    """Every output against the oracle, in[i - 1] across the round seams included; prev afterwards."""
    import torch

    rng = np.random.default_rng(n % 1000)
    t = np.arange(HEAD + n)
    x = np.exp(1j * (0.3 * t + 2.0 * np.sin(t / 300.0))) * (1 + 0.05 * rng.standard_normal(t.size))
    ofm = oracle.FM(np.complex128)
    host, dev = c.FMDemodNodeF64(), c.FMDemodNodeF64()
    for a, b in ((0, HEAD), (HEAD, HEAD + n)):
        want = ofm.demod(x[a:b])
        for got in (host.run(x[a:b]), on_device(lambda i, o, s: dev.run_dev(i, b - a, o, s), x[a:b], b - a, torch.float64)):
            assert got.dtype == np.float64 and got.shape == want.shape
            d = np.abs((got - want + np.pi) % (2 * np.pi) - np.pi)
            assert np.max(d) <= 1e-12, (a, b, int(np.argmax(d)))
    assert host.prev == x[-1] and dev.prev == x[-1]


# ------------------------------------------------------------------ f64 mixer
@pytest.mark.gpu
def test_mixer_f64_samples_do_not_depend_on_the_batch_they_arrive_in(c):
    """Four grid sweeps in one call against the same stream in ragged calls (one of them a single sample): the same bits.  A
    rotor stepped from sweep to sweep instead of evaluated per sample fails this in the last bits of the later sweeps."""
    n = 3 * T + 1
    x = rand_c128(np.random.default_rng(6), n)
    one = c.MixerNode(0.123, 0.4).run(x)
    node = c.MixerNode(0.123, 0.4)
    cuts = (0, HEAD, HEAD + 1, T + 1, 2 * T + 3, n)
    parts = np.concatenate([node.run(x[a:b]) for a, b in zip(cuts[:-1], cuts[1:])])
    assert one.dtype == np.complex128 and np.array_equal(bits(one), bits(parts))
    want = oracle.Mixer(0.4, 0.123).mix(x)
    assert np.all(np.abs(one - want) <= 1e-9 * np.abs(x) + 1e-30)   # the bound of test_mixer_f64_vs_oracle


# ------------------------------------------------------------------ wire-format converters
def c32_with_edges(rng, n):
    """Samples whose 8192-fold covers the i16 range and beyond (saturation both ways), with NaN and +-inf sprinkled in."""
    x = (rng.uniform(-6, 6, n) + 1j * rng.uniform(-6, 6, n)).astype(np.complex64)
    f = x.view(np.float32)
    at = rng.integers(0, f.size, 3 * 64)
    f[at[:64]] = np.nan
    f[at[64:128]] = np.inf
    f[at[128:]] = -np.inf
    for k, v in enumerate((np.nan, np.inf, -np.inf, 3.99, -4.0001)):   # and in the lanes either side of each round seam
        f[[p for p in (2 * T - 2 - k, 2 * T + k, 4 * T - 1 - k, 4 * T + 1 + k) if p < f.size]] = v
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_wire_converters_past_the_grid_cap(c, n):
    import torch

    rng = np.random.default_rng(n % 1000 + 3)
    lib = c.lib()
    i16 = rand_i16(rng, n)
    u8 = rng.integers(0, 256, (n, 2), dtype=np.uint8)
    x = c32_with_edges(rng, n)
    for scale in (1.0, 1.0 / 8192):
        want = oracle.iq_i16_to_c32(i16, scale)
        assert np.array_equal(c.iq_i16_to_c32(i16, scale), want), scale
        got = on_device(lambda i, o, st: ok(lib.comms_iq_i16_to_c32_dev(i, n, scale, o, 0, st)), i16, n, torch.complex64)
        assert np.array_equal(got, want), scale
    want = oracle.iq_u8_to_c32(u8)
    assert np.array_equal(c.iq_u8_to_c32(u8), want)
    assert np.array_equal(on_device(lambda i, o, st: ok(lib.comms_iq_u8_to_c32_dev(i, n, o, 0, st)), u8, n, torch.complex64), want)
    want = oracle.iq_c32_to_i16(x, 8192.0)
    assert want.min() == -32768 and want.max() == 32767
    assert np.array_equal(c.iq_c32_to_i16(x, 8192.0), want)
    got = on_device(lambda i, o, st: ok(lib.comms_iq_c32_to_i16_dev(i, n, 8192.0, o, 0, st)), x, n, torch.int16, 2)
    assert np.array_equal(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2 * T + 3, 4 * T + 6])   # two samples per lane: the cap sits at 2 T samples; odd (a lone tail) and even
def test_real_casts_past_the_grid_cap(c, n):
    import torch

    rng = np.random.default_rng(n % 1000 + 4)
    lib = c.lib()
    r = rng.standard_normal(n).astype(np.float32)
    r[[0, 1, 2 * T - 1, 2 * T, 2 * T + 1, n - 1]] = [-0.0, np.inf, 1.5, -2.5, 3.5, -7.0]
    got = on_device(lambda i, o, st: ok(lib.comms_iq_real_to_c32_dev(i, n, o, 0, st)), r, n, torch.complex64)
    want = np.zeros(n, np.complex64)
    want.real = r
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    z = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    got = on_device(lambda i, o, st: ok(lib.comms_iq_c32_re_dev(i, n, o, 0, st)), z, n, torch.float32)
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(z.real).view(np.uint32))


# ------------------------------------------------------------------ estimators
# count > 3 * stride is what enters estimator_kernel's unrolled loop; the frequency kind has count = n - 1, so 3 T + 1 and
# 3 T + 2 straddle its first entry
EST_N = (3 * T, 3 * T + 1, 3 * T + 2, 4 * T, 4 * T + 5, (1 << 24) + 3)
EST_NMAX = max(EST_N)
PSK_TRUTH, FREQ_TRUTH = 0.123456, 0.123456789
KINDS = [("freq", 0)] + [("psk", m) for m in (1, 2, 3, 4, 8)] + [("qam", 4)]


def long_freq_stream(rng, truth, n):
    """test_estimators.freq_stream at length: 4-PSK, x4 zero-stuffed, 16-tap RRC (beta 0.75), shifted by `truth` rad / sample."""
    n_sym = -(-n // 4)
    up = np.zeros(4 * n_sym, np.complex128)
    up[::4] = np.exp(2j * np.pi * rng.integers(0, 4, n_sym) / 4)
    taps = oracle.rrc_taps(16, 4.0, 0.75, dtype=np.complex128)
    data = oracle.batch_fir(up, taps, oracle.default_state(taps))[:n]
    return data * np.exp(1j * truth * np.arange(n))


@functools.lru_cache(maxsize=1)
def noise_input():
    rng = np.random.default_rng(2024)
    return rng.standard_normal(EST_NMAX) + 1j * rng.standard_normal(EST_NMAX)


@functools.lru_cache(maxsize=1)
def est_input(kind, m, which):
    """EST_NMAX samples; the tests use its prefixes.  which = "known": the reference tests' constructions, whose truth is
    known; "noise": complex normal noise (a sum that cancels down to ~sqrt(n) of its terms)."""
    if which == "noise":
        return noise_input()
    rng = np.random.default_rng(100 + m)
    if kind == "freq":
        return long_freq_stream(rng, FREQ_TRUTH, EST_NMAX)
    return psk_stream(rng, m, EST_NMAX, PSK_TRUTH) if kind == "psk" else qam16_stream(rng, EST_NMAX, PSK_TRUTH)


def oracle_estimate(kind, m, x):
    if kind == "freq":
        return oracle.frequency_offset_estimate(x)
    return oracle.psk_phase_estimate(x, m) if kind == "psk" else oracle.qam_phase_estimate(x)


def extended_estimates(kind, m, x, lengths):
    """The same estimates with the f64 terms summed in np.longdouble (numpy's pairwise sum, accumulator type only: no
    extended-precision copy of the stream): one per prefix length.  The terms are formed in f64 as the oracle forms them, up
    to the order of the multiplications of x^m -- rounding of ~1e-16 per term, which averages out over a sum."""
    if kind == "freq":
        t = x[1:] * np.conj(x[:-1])
    else:
        t = x.copy()
        for _ in range(m - 1):
            t *= x
        if kind == "qam":
            t = -t
    div = 1 if kind == "freq" else m
    out, re, im, done = [], np.longdouble(0), np.longdouble(0), 0
    for n in sorted(lengths):                      # each prefix = the one before it plus the stretch between them
        cnt = max(n - 1, 0) if kind == "freq" else n
        re += np.sum(t.real[done:cnt], dtype=np.longdouble)
        im += np.sum(t.imag[done:cnt], dtype=np.longdouble)
        done = cnt
        out.append(float(np.arctan2(im, re) / div))
    return out


# The condition the issue sets: at most 1e-10.  Largest value observed over every (kind, input, length) below: 7.21e-11
# (psk m = 3, known truth: 2^24 equal terms, where a sequential fold is at its worst); noise inputs stay below 2e-13.
ORACLE_FOLD_BOUND = 1e-10


@pytest.mark.parametrize("which", ["known", "noise"])
@pytest.mark.parametrize("kind,m", KINDS)
def test_estimator_oracle_fold_is_accurate_on_these_inputs(kind, m, which):
    """No GPU.  The condition under the 1e-9 of the device test: the oracle's sequential f64 fold is within 1e-10 of the
    extended-precision sum on every input and length used there, and the known-truth inputs meet the reference's own test
    bounds (1e-6 for PSK, 0.01 for the frequency and QAM estimates)."""
    x = est_input(kind, m, which)
    ext = extended_estimates(kind, m, x, EST_N)
    worst = 0.0
    for n, e in zip(EST_N, ext):
        o = oracle_estimate(kind, m, x[:n])
        worst = max(worst, abs(o - e))
        if which == "known":
            truth, tol = (FREQ_TRUTH, 0.01) if kind == "freq" else (PSK_TRUTH, 1e-6 if kind == "psk" else 0.01)
            assert abs(o - truth) < tol, (kind, m, n, o)
    print("oracle fold vs extended precision: %s m=%d %s: %.3e" % (kind, m, which, worst))
    assert worst <= ORACLE_FOLD_BOUND, (kind, m, which, worst)


def device_estimates(c, kind, m, x, xd):
    """(host entry, device entry) of one estimator on the same samples (x on the host, xd the torch copy)."""
    import torch

    lib, out, s = c.lib(), C.c_double(), torch.cuda.current_stream().cuda_stream
    if kind == "freq":
        host = c.frequency_offset_estimate(x)
        ok(lib.comms_frequency_offset_estimate_dev(xd.data_ptr(), x.size, C.byref(out), 0, s))
    elif kind == "psk":
        host = c.psk_phase_estimate(x, m)
        ok(lib.comms_psk_phase_estimate_dev(xd.data_ptr(), x.size, m, C.byref(out), 0, s))
    else:
        host = c.qam_phase_estimate(x)
        ok(lib.comms_qam_phase_estimate_dev(xd.data_ptr(), x.size, C.byref(out), 0, s))
    return host, out.value


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["known", "noise"])
@pytest.mark.parametrize("kind,m", KINDS)
def test_estimators_past_the_unrolled_loop_threshold(c, kind, m, which):
    import torch

    x = est_input(kind, m, which)
    xd = torch.from_numpy(x).to("cuda:0")
    assert xd.data_ptr() % 16 == 0
    for n in EST_N + (T + 1, 65537, 65536, 1000):   # descending at the end: short calls after long ones on one partials buffer
        want = oracle_estimate(kind, m, x[:n])
        host, dev = device_estimates(c, kind, m, x[:n], xd[:n])
        assert host == dev, (n, host, dev)             # same kernel, same grid, same fixed-order fold of the partials
        # parallel tree vs sequential fold: rounding-level differences only (the oracle itself is within 1e-10 of the
        # extended-precision sum on these inputs: ORACLE_FOLD_BOUND)
        assert abs(host - want) < 1e-9, (n, host, want)
        if which == "known" and n >= 3 * T:
            truth, tol = (FREQ_TRUTH, 0.01) if kind == "freq" else (PSK_TRUTH, 1e-6 if kind == "psk" else 0.01)
            assert abs(host - truth) < tol, (n, host)


@pytest.mark.gpu
def test_estimator_edges_and_stale_partials(c):
    """The empty sum, the one-sample frequency estimate (no pair), a misaligned device pointer; and a long call followed by
    short ones on the same thread: the long call leaves 2048 partials in the thread's buffer, the short ones must read
    back only their own."""
    import torch

    lib, out, s = c.lib(), C.c_double(), torch.cuda.current_stream().cuda_stream
    x = est_input("freq", 0, "noise")[:4 * T + 5]
    xd = torch.from_numpy(x).to("cuda:0")
    empty = np.zeros(0, np.complex128)
    for n in (4 * T + 5, 0, 1, 2, 255, 257, 4 * T + 5, 1, 0):
        for kind, m in KINDS:
            xs = x[:n] if n else empty
            want = oracle_estimate(kind, m, xs)
            host, dev = device_estimates(c, kind, m, xs, xd[:n])
            assert host == dev and abs(host - want) < 1e-9, (n, kind, m, host, dev, want)
            if n == 0 or (n == 1 and kind == "freq"):
                assert host == want == 0.0        # arg(0 + 0i) = atan2(0, 0) = 0
    # Complex<f64> samples are read as 16-byte words: a pointer half a sample off is refused
    assert lib.comms_frequency_offset_estimate_dev(xd.data_ptr() + 8, 100, C.byref(out), 0, s) == c.COMMS_ERR_ARG
    assert lib.comms_psk_phase_estimate_dev(xd.data_ptr() + 8, 100, 4, C.byref(out), 0, s) == c.COMMS_ERR_ARG
    assert lib.comms_qam_phase_estimate_dev(xd.data_ptr() + 8, 100, C.byref(out), 0, s) == c.COMMS_ERR_ARG
