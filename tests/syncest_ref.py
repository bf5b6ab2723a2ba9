"""Reference material of the Complex<f32> synchronisation estimators (comms_syncest_*, comms_*_phase_estimate_c32), shared
by tests/test_syncest_ref.py (CPU) and tests/test_gpu_syncest.py:

  ref_sums    TimingEstimator::push and frequency_offset_estimate restated in numpy, f64 throughout, returning the complex
              sums the two take arg of and the sums of |terms| (the oracle returns angles only); the CPU test pins its angles
              to the oracle's.
  model_sums  the ARITHMETIC of syncest_kernel (include/comms_hip.h): rotor table of 2 n values computed in f64 and rounded
              to f32, qin / q(t) filter / din in f32, every product qout * dout and the sums in f64.  Its distance from the
              oracle is what the f32 filter costs; the GPU tolerance is four times the largest distance measured.
  CASES       every input the GPU test runs, so that the CPU test measures the model on exactly those.
"""
import functools

import numpy as np

import oracle
import rx_ref
import symsync_ref

TILE = 2048        # samples per tile of syncest_kernel (the GPU test checks it against comms_syncest_get_kernel)
GRID_CAP = 8 * 256  # no persistent grid of the library exceeds eight workgroups on each of 256 CUs (resident_workgroups)
N_BIG = (GRID_CAP + 1) * TILE + 5   # every workgroup walks at least two tiles, whatever the grid

# Largest distance of model_sums from the oracle over CASES, measured by tests/test_syncest_ref.py (which asserts that they
# still hold): the timing estimate in samples (circular, mod n), and the timing sum relative to the sum of |terms|.
MODEL_TIMING_DISTANCE = 1.9e-7   # measured 1.896e-7: (n, d) = (8, 63) at len = n d + 1, a sum of ONE product; long blocks: < 7e-8
MODEL_SUM_DISTANCE = 2.02e-7     # measured 2.017e-7, the same case
# The GPU tolerances: four times those (the kernel's summation order within the f32 filter differs from the model's).
TIMING_TOL = 4 * MODEL_TIMING_DISTANCE
TIMING_SUM_TOL = 4 * MODEL_SUM_DISTANCE
# An input whose model distance exceeds this has a sum too incoherent to test an angle on: it is replaced, not tolerated.
MAX_MODEL_DISTANCE = 1e-5
# Angle inputs keep |sum| / sum|terms| of the reference above this.
MIN_COHERENCE = 0.05
# Frequency and phase estimates: the bound tests/test_estimators.py holds the f64 entries to (the arithmetic after the
# widening load is the same).
ANGLE_TOL = 1e-9
# freq_sum against the f64 restatement, relative to the sum of |terms|: a sum error below ANGLE_TOL * MIN_COHERENCE cannot move
# the angle of a tested input by more than ANGLE_TOL.  (Each term is exact to 2^-53; the orders of summation differ by
# ~1e-14 of the sum of |terms| at the longest input.)
FREQ_SUM_TOL = ANGLE_TOL * MIN_COHERENCE


def circ(a, b, period):
    """|a - b| modulo `period`: an estimate near +-period/2 may land on either side."""
    return abs((a - b + period / 2.0) % period - period / 2.0)


def timing_of(s, n):
    """-n arg(s) / (2 pi), TimingEstimator::push's last line."""
    return -n * np.arctan2(s.imag, s.real) / (2.0 * np.pi)


# ------------------------------------------------------------------ the two restatements
def ref_sums(x, n, d, alpha):
    """f64: (timing_sum, freq_sum, sum|timing terms|, sum|freq terms|) of X = x as complex128."""
    X = np.asarray(x).astype(np.complex128)
    nd = n * d
    i = np.arange(X.size, dtype=np.float64)
    r = np.exp(1j * (-np.pi * i / n))
    qin, din = np.conj(X) * r, X * r
    taps = oracle.qfilt_taps(2 * nd + 1, alpha, n)
    if X.size > nd:
        qout = np.convolve(qin, taps)[: X.size]
        terms = qout[nd:] * din[: X.size - nd]
        ts, ta = complex(np.sum(terms)), float(np.sum(np.abs(terms)))
    else:
        ts, ta = 0j, 0.0
    ft = X[1:] * np.conj(X[:-1])
    return ts, complex(np.sum(ft)), ta, float(np.sum(np.abs(ft)))


def model_sums(x, n, d, alpha):
    """syncest_kernel's arithmetic: (timing_sum, freq_sum)."""
    x = np.ascontiguousarray(x, dtype=np.complex64)
    nd, f32 = n * d, np.float32
    th = (-np.pi * np.arange(2 * n, dtype=np.float64)) / n
    rr_t, ri_t = np.cos(th).astype(f32), np.sin(th).astype(f32)        # the rotor table, f64 rounded to f32
    m = np.arange(x.size) % (2 * n)
    rr, ri = rr_t[m], ri_t[m]
    xr, xi = x.real.astype(f32), x.imag.astype(f32)
    qr, qi = xr * rr + xi * ri, xr * ri - xi * rr                       # conj(x) r, f32, unfused
    dr, di = xr * rr - xi * ri, xr * ri + xi * rr                       # x r
    taps = oracle.qfilt_taps(2 * nd + 1, alpha, n).astype(f32)
    if x.size > nd:
        or_, oi = np.zeros(x.size, f32), np.zeros(x.size, f32)
        for k in range(min(taps.size, x.size)):                         # k ascending from +0, f32 (the kernel fuses each step)
            if taps[k] != 0:
                or_[k:] += taps[k] * qr[: x.size - k]
                oi[k:] += taps[k] * qi[: x.size - k]
        qo = or_[nd:].astype(np.float64) + 1j * oi[nd:].astype(np.float64)
        do = dr[: x.size - nd].astype(np.float64) + 1j * di[: x.size - nd].astype(np.float64)
        ts = complex(np.sum(qo * do))
    else:
        ts = 0j
    X = x.astype(np.complex128)
    return ts, complex(np.sum(X[1:] * np.conj(X[:-1])))


# ------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def signal(n, length, seed=0, drop=None):
    """QPSK at n samples per symbol shaped by an RRC pulse (8 symbols, beta 0.5), a little noise, as Complex<f32>; the first
    `drop` samples removed (default 1 where n > 1: the symbol peaks do not sit on multiples of n)."""
    drop = (1 if n > 1 else 0) if drop is None else drop
    rng = np.random.default_rng(1000 * n + seed)
    n_sym = (length + drop) // n + 1
    up = np.zeros(n_sym * n, np.complex128)
    up[::n] = np.exp(1j * (np.pi / 2 * rng.integers(0, 4, n_sym) + np.pi / 4))
    taps = oracle.rrc_taps(8 * n + 1, float(n), 0.5, np.complex128)
    y = oracle.batch_fir(up, taps, oracle.default_state(taps))[drop: drop + length]
    y = y + 0.01 * (rng.standard_normal(length) + 1j * rng.standard_normal(length))
    out = y.astype(np.complex64)
    out.setflags(write=False)
    return out


def with_impulse(x, at):
    y = x.copy()
    y[at] += np.complex64(5.0 + 2.5j)
    return y


ND = [(1, 1), (2, 5), (4, 4), (8, 8), (8, 63)]   # the last: 1009 taps, the long-filter end


def lengths(n, d):
    return [0, 1, 2, n * d, n * d + 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5]


@functools.lru_cache(maxsize=None)
def cases():
    """(name, n, d, alpha, x): every block the GPU test estimates."""
    out = []
    for n, d in ND:
        for ln in lengths(n, d):
            out.append(("len%d" % ln, n, d, 0.25, signal(n, ln)))
    for alpha in (0.0, 1.0):                                  # 0.25 is in the grid above
        for ln in (TILE + 1, 3 * TILE + 5):
            out.append(("alpha%g-len%d" % (alpha, ln), 4, 4, alpha, signal(4, ln)))
    out.append(("past-the-grid", 4, 4, 0.25, signal(4, N_BIG)))
    out.append(("offset-pointer", 4, 4, 0.25, signal(4, TILE + 2)[1:]))        # the GPU test passes pointer + 8 bytes
    for n, d in ((4, 4), (8, 63)):
        out.append(("impulse-at-0", n, d, 0.25, with_impulse(signal(n, 2 * TILE), 0)))
        out.append(("impulse-at-tile-edge", n, d, 0.25, with_impulse(signal(n, 2 * TILE), TILE - 1)))
    return out


@functools.lru_cache(maxsize=None)
def reference(idx):
    """Oracle values and f64 sums of case idx, computed once: dict(timing, freq, ts, fs, ta, fa)."""
    _, n, d, alpha, x = cases()[idx]
    X = x.astype(np.complex128)
    ts, fs, ta, fa = ref_sums(x, n, d, alpha)
    return dict(timing=oracle.timing_push(X, n, d, alpha), freq=oracle.frequency_offset_estimate(X), ts=ts, fs=fs, ta=ta, fa=fa)


# ------------------------------------------------------------------ the loop the estimators exist for
LOOP_L, LOOP_S, LOOP_NP, LOOP_BETA, LOOP_D, LOOP_NSYM = 32, 4, 33, 0.35, 8, 2048
LOOP_PHASE = 0.3                     # constant carrier phase of the received stream
LOOP_DD = (0, 5, 27, 64)             # fractional delays in steps of 1 / L; 64 puts the estimate at +-S / 2
# psk_phase_estimate measures the rotation of a constellation ON the axes (exp(2 pi i k / M)); digital.rs's QPSK table sits at
# odd multiples of pi / 4, which is part of what the estimate returns and must stay in the symbols
QPSK_OFFSET = np.pi / 4


@functools.lru_cache(maxsize=None)
def loop_signal(dd):
    """(values, x as Complex<f32>, prototype h): QPSK of known values, RRC pulse, delayed by dd / L samples, rotated by
    LOOP_PHASE; no frequency offset, no noise."""
    v = np.random.default_rng(77).integers(0, 4, LOOP_NSYM)
    sym = rx_ref.QPSK_DEF[v].astype(np.complex128)
    x = symsync_ref.fractional_delay(sym, LOOP_NP, LOOP_S, LOOP_L, LOOP_BETA, dd, oracle.rrc_taps, oracle.pulse)
    x = (x * np.exp(1j * LOOP_PHASE)).astype(np.complex64)
    N = (LOOP_NP - 1) * LOOP_L + 1
    h = oracle.rrc_taps(N, float(LOOP_L * LOOP_S), LOOP_BETA, np.complex128).real.astype(np.float32)
    return v, x, h


def loop_rotations(phase_estimate):
    """The four rotations to try: the estimate taken out (the mixer's sign is exp(+i phase)), the constellation's own pi / 4
    left in, and the quarter turns the 4th power cannot tell apart."""
    return [(-(phase_estimate - QPSK_OFFSET) + k * np.pi / 2) % (2 * np.pi) for k in range(4)]


def loop_bit_errors(values, v, h, bit_errors=None):
    """Bit errors of decided symbol values against the transmitted ones: transients dropped, best whole-symbol lag of -2 .. 2
    around the filters' delay (the alignment of test_symsync_ref.count_errors).  bit_errors(a, b, n_bits) counts (default:
    numpy)."""
    skip = LOOP_NP
    delay = int(round(((LOOP_NP - 1) / 2.0 + (h.size - 1) / (2.0 * LOOP_L)) / LOOP_S))
    k = np.arange(skip, values.size - skip)
    best = None
    for lag in range(-2, 3):
        a, b = rx_ref.pack(values[k], 2), rx_ref.pack(v[k - delay - lag], 2)
        if bit_errors is None:
            errs = int(np.sum(np.unpackbits(a ^ b)))
        else:
            errs = bit_errors(a, b, 2 * k.size)
        best = errs if best is None else min(best, errs)
    return best, 2 * k.size
