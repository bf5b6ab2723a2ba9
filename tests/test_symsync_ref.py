"""CPU check of tests/symsync_ref.py, the float64 reference the GPU symbol-synchroniser tests compare with.
Part 1: against the oracle's nodes in series -- oracle.upsample(x, L) -> oracle.batch_fir(.., norotate=True) over the
concatenated calls -> [mu::L S] -> oracle.Mixer -- within the project's f32 FIR bound, in two calls with the state carried.
Part 2: the relation between TimingEstimator::push and the node's tau that include/comms_hip.h states
(comms_symsync_set_timing), pinned over a sweep of fractional delays with the oracle's estimator, and the end-to-end
conditions of tests/test_gpu_symsync.py on the reference alone.
Also what of comms_symsync_* needs no device: the length helpers and the argument checks that come before the device."""
import ctypes as C

import numpy as np
import pytest

import oracle
import rx_ref
import symsync_ref as sr
from symsync_ref import SymSyncRef

TOL = 1e-5  # tests/test_gpu_parity.py: the f32 FIR bound is TOL * sum|taps| * max|x|
CASES = [(1, 4, 33), (32, 4, 1025), (32, 2, 513), (7, 3, 50), (8, 1, 64), (16, 4, 5)]


def mus(L, S):
    return sorted({0, 1 % (S * L), L - 1, L % (S * L), S * L - 1})


def rand_c(rng, n):
    return (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(np.complex64)


# ------------------------------------------------------------------ part 1: the oracle's composition
@pytest.mark.parametrize("L,S,N", CASES)
def test_symsync_ref_matches_the_oracle_composition(L, S, N):
    rng = np.random.default_rng(1000 * L + 10 * S + N)
    taps = rng.uniform(-1, 1, N).astype(np.float32)
    ct = taps.astype(np.complex64)
    calls = (S * 37, S * 23)
    xs = [rand_c(rng, n) for n in calls]
    # the filter at L times the rate over the concatenated calls: one state, as a stream
    state = oracle.default_state(ct)
    fine = [oracle.batch_fir(oracle.upsample(x, L), ct, state, norotate=True) for x in xs]
    bound = TOL * float(np.sum(np.abs(taps))) * max(float(np.max(np.abs(x))) for x in xs)
    for mu in mus(L, S):
        for dphase, phase in ((0.0, 0.0), (0.37, 1.1)):
            ref = SymSyncRef(taps, L, S)
            ref.mu = mu
            ref.set_rotation(dphase, phase)
            mix = oracle.Mixer(phase, dphase)
            for x, f in zip(xs, fine):
                want = f[mu::L * S]
                assert want.size == x.size // S
                if dphase or phase:
                    want = mix.mix(want)
                got = ref.run(x)
                assert got.shape == want.shape
                err = float(np.max(np.abs(got - want.astype(np.complex128))))
                assert err <= bound, (L, S, N, mu, dphase, err, bound)
            # the history is raw samples, whatever mu: the last Q inputs, newest first
            seen = np.concatenate([np.zeros(ref.Q, np.complex64)] + xs)
            assert np.array_equal(ref.state(), seen[::-1][: ref.Q])
            assert ref.Q == sr.state_len(N, L) == (N - 1) // L


def test_empty_phases_are_exact_zeros_and_cuts_are_neutral():
    rng = np.random.default_rng(5)
    taps = rng.uniform(-1, 1, 5).astype(np.float32)
    x = rand_c(rng, 4 * 40)
    for mu in range(4 * 16):
        ref = SymSyncRef(taps, 16, 4)
        ref.mu = mu
        y = ref.run(x)
        assert np.all(y == 0.0) if mu % 16 >= 5 else np.all(y[1:] != 0.0)
    taps = rng.uniform(-1, 1, 50).astype(np.float32)
    whole = SymSyncRef(taps, 7, 3)
    cut = SymSyncRef(taps, 7, 3)
    whole.mu = cut.mu = 11
    x = rand_c(rng, 3 * 50)
    parts = np.concatenate([cut.run(x[:3]), cut.run(x[3:3 * 9]), cut.run(x[3 * 9:])])
    assert np.array_equal(parts, whole.run(x))   # the same products in the same order


def test_timing_reduction_and_decisions():
    assert sr.mu_of(0.37, 32, 4) == 12 and sr.mu_of(-0.01, 32, 4) == 0 and sr.mu_of(-0.02, 32, 4) == 127
    assert sr.mu_of(4.0, 32, 4) == 0 and sr.mu_of(3.99, 32, 4) == 0 and sr.mu_of(0.5 / 32, 32, 4) == 1
    ref = SymSyncRef(np.ones(1, np.float32), 1, 1)
    ref.set_output(2)
    y = np.array([1 + 1j, -1 + 1j, 1 - 1j, -1 - 1j, 0.5 + 2j], np.complex64)
    assert np.array_equal(ref.run(y), rx_ref.sym_to_bits(y, 2))


# ------------------------------------------------------------------ part 2: what to feed set_timing
def qpsk(n_sym, seed):
    v = np.random.default_rng(seed).integers(0, 4, n_sym)
    return v, rx_ref.QPSK_DEF[v].astype(np.complex128)


SWEEPS = [  # L, S, taps of the transmit pulse per S, taps of the node's prototype per S (both odd), beta, estimator d, step of dd
    (32, 4, 33, 33, 0.35, 8, 1),
    (32, 4, 35, 33, 0.35, 8, 7),
    (32, 4, 33, 35, 0.35, 4, 7),
    (16, 2, 21, 23, 0.5, 8, 3),
    (8, 8, 65, 49, 0.25, 8, 5),
]


@pytest.mark.parametrize("L,S,NP,NN,beta,d_est,step", SWEEPS)
def test_estimate_is_the_peak_position_and_tau_follows(L, S, NP, NN, beta, d_est, step):
    """e = c mod S to ESTIMATE_ACCURACY, c the position of the symbol peaks in the call; so tau = e + (N - 1) / (2 L) puts the
    node's sample within ESTIMATE_ACCURACY + 1 / (2 L) of the symbol centre c + (N - 1) / (2 L)."""
    _, sym = qpsk(2048, 1)
    N = (NN - 1) * L + 1
    worst = 0.0
    for dd in range(0, L * S, step):
        x = sr.fractional_delay(sym, NP, S, L, beta, dd, oracle.rrc_taps, oracle.pulse)
        e = oracle.timing_push(x, S, d_est, beta)
        assert -S / 2 - 1e-9 <= e <= S / 2 + 1e-9
        c = sr.peak_position(NP, L, dd)
        worst = max(worst, abs((e - c + S / 2) % S - S / 2))
        tau = sr.tau_from_estimate(e, N, L, S)
        centre = (c + (N - 1) / (2.0 * L)) % S
        assert abs((tau - centre + S / 2) % S - S / 2) <= sr.ESTIMATE_ACCURACY
        mu = sr.mu_of(tau, L, S)
        assert abs((mu / L - centre + S / 2) % S - S / 2) <= sr.ESTIMATE_ACCURACY + 0.5 / L
    print("L=%d S=%d: max |e - c| = %.5f input samples" % (L, S, worst))
    assert worst <= sr.ESTIMATE_ACCURACY


def end_to_end_ref(dd, half_symbol_off, step=0, L=32, S=4, NP=33, beta=0.35, n_sym=4096, seed=7):
    """The pipeline of test_gpu_symsync's end-to-end test on the reference, its mu moved by `step` steps of 1 / L: (bit
    errors, decisions within the f32 bound of a decision line, bits compared)."""
    v, sym = qpsk(n_sym, seed)
    x = sr.fractional_delay(sym, NP, S, L, beta, dd, oracle.rrc_taps, oracle.pulse)
    N = (NP - 1) * L + 1
    h = oracle.rrc_taps(N, float(L * S), beta, np.complex128).real.astype(np.float32)
    e = oracle.timing_push(x, S, 8, beta)
    tau = sr.tau_from_estimate(e, N, L, S) + (S / 2.0 if half_symbol_off else 0.0)
    ref = SymSyncRef(h, L, S)
    ref.set_timing(tau)
    ref.mu = (ref.mu + step) % (S * L)
    y = ref.run_c(x.astype(np.complex64))
    return count_errors(y, v, NP, h, x)


def half_symbol_margin(y_of_mu, mu, v, NP, h, x, L=32, S=4):
    """The bit errors a receiver half a symbol off must at least show.  The relation's measured accuracy (ESTIMATE_ACCURACY =
    0.003 input samples = 0.1 step at L = 32) on top of the rounding to a step puts its instant within ONE step of 1 / L of
    mu: the margin is the fewest errors of the reference over mu - 1, mu, mu + 1, less the decisions that f32 sums could flip
    against the reference (those within the f32 FIR bound of a decision line).  y_of_mu(mu) -> the reference's outputs."""
    worst = None
    for step in (-1, 0, 1):
        errs, flippable, _ = count_errors(y_of_mu((mu + step) % (S * L)), v, NP, h, x, L, S)
        worst = errs - flippable if worst is None else min(worst, errs - flippable)
    return worst


def count_errors(y, v, NP, h, x, L=32, S=4):
    """Transient symbols dropped (the two filters' spans), whole-symbol lag by trying -2 .. 2 around the filters' delay:
    (fewest bit errors, the decisions a perturbation of the f32 FIR bound could flip, bits compared)."""
    skip = NP
    delay = int(round(((NP - 1) / 2.0 + (h.size - 1) / (2.0 * L)) / S))   # pulse + matched filter, in symbols
    got = rx_ref.decide(np.asarray(y).astype(np.complex64), rx_ref.QPSK_DEF)
    bound = TOL * float(np.sum(np.abs(h))) * float(np.max(np.abs(x)))
    k = np.arange(skip, got.size - skip)
    near = (np.abs(y.real) <= bound) | (np.abs(y.imag) <= bound)
    best = None
    for lag in range(-2, 3):
        diff = got[k] ^ v[k - delay - lag]
        errs = int(np.sum((diff & 1) + (diff >> 1)))
        if best is None or errs < best[0]:
            best = (errs, 2 * int(np.sum(near[k])), 2 * k.size)
    return best


@pytest.mark.parametrize("dd", [0, 5, 16, 27])
def test_end_to_end_conditions_hold_on_the_reference(dd):
    errs, flippable, n_bits = end_to_end_ref(dd, False)
    assert errs == 0 and flippable == 0 and n_bits > 8000, (errs, flippable, n_bits)
    # half a symbol off, every neighbouring pair of unlike bits is decided by the rest of the intersymbol interference: about
    # a quarter of the bits are wrong.  The margin the GPU test asserts is the fewest errors over the three steps the
    # estimator's accuracy allows (half_symbol_margin); here: it is far from the 0 errors of the receiver on time
    per_step = [end_to_end_ref(dd, True, step) for step in (-1, 0, 1)]
    margin = min(errs - flippable for errs, flippable, _ in per_step)
    print("dd=%d: half a symbol off, (errors, flippable, bits) at steps -1, 0, 1: %s -> margin %d" % (dd, per_step, margin))
    assert margin > 0


# ------------------------------------------------------------------ the library without a device
@pytest.fixture(scope="module")
def c():
    import __graft_entry__ as g

    g.build()
    import comms_rs_amd as c

    return c


def test_length_helpers(c):
    from comms_rs_amd import _lib

    lib = _lib.lib()
    m = C.c_size_t(12345)
    for L, S, N in CASES + [(256, 4, 4096), (1, 1, 1), (4, 256, 4096), (0, 0, 7)]:
        for n in (0, 1, 5, 17, 40, 4097, 20011, 1 << 26):
            assert lib.comms_symsync_out_len(n, S, C.byref(m)) == 0 and m.value == sr.out_len(n, S), (S, n)
        assert lib.comms_symsync_state_len(N, L, C.byref(m)) == 0 and m.value == sr.state_len(N, L), (L, N)
    assert lib.comms_symsync_out_len(6, 3, None) == 1
    assert lib.comms_symsync_state_len(6, 3, None) == 1
    assert lib.comms_symsync_state_len(0, 3, C.byref(m)) == 1


def test_arguments_are_checked_before_the_device(c):
    from comms_rs_amd import _lib

    lib = _lib.lib()
    t = np.ones(4096, np.float32)
    p = t.ctypes.data_as(C.c_void_p)
    h = C.c_void_p()
    assert lib.comms_symsync_create(p, 0, 32, 4, 0, C.byref(h)) == 1 and not h       # n_taps == 0
    assert lib.comms_symsync_create(None, 4, 32, 4, 0, C.byref(h)) == 1 and not h    # NULL taps
    assert lib.comms_symsync_create(p, 4, 32, 4, 0, None) == 1                       # NULL out
    assert lib.comms_symsync_create(p, 4, 257, 4, 0, C.byref(h)) == 1 and not h      # L > 256
    assert lib.comms_symsync_create(p, 4, 32, 257, 0, C.byref(h)) == 1 and not h     # S > 256
    assert lib.comms_symsync_create(p, 2049, 2, 4, 0, C.byref(h)) == 1 and not h     # ceil(N / L) > 1024
    with pytest.raises(c.CommsError) as e:
        c.SymbolSyncNode(np.zeros(0, np.float32), 32, 4)
    assert e.value.code == 1
    assert lib.comms_symsync_destroy(None) == 0
    for call in (lambda: lib.comms_symsync_set_timer(None, None), lambda: lib.comms_symsync_run_dev(None, None, 0, None, None),
                 lambda: lib.comms_symsync_run(None, None, 0, None), lambda: lib.comms_symsync_get_state(None, None, 0),
                 lambda: lib.comms_symsync_set_state(None, None, 0), lambda: lib.comms_symsync_get_kernel(None, 8, None, 0),
                 lambda: lib.comms_symsync_set_timing(None, 0.0), lambda: lib.comms_symsync_get_timing(None, None),
                 lambda: lib.comms_symsync_set_rotation(None, 0.0, 0.0), lambda: lib.comms_symsync_get_phase(None, None),
                 lambda: lib.comms_symsync_set_output_format(None, 0, 0, None)):
        assert call() == 1


def test_symbol_synchroniser_has_no_cpu_fallback(c):
    if c.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(c.CommsError) as e:
        c.SymbolSyncNode(np.ones(1025, np.float32), 32, 4)
    assert e.value.code == 2
