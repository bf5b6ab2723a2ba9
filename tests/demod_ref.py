"""Reference material of the f64 timing estimator and the NCO (csrc/demod.hip: comms_timing_*, comms_nco_*), shared by
tests/test_demod_ref.py (CPU), tests/test_gpu_demod_seams.py, tests/test_estimators.py and the demod family of
tests/grid_children.py.

NCO.  Phase errors, dphase and the start phase are integers in units of 2^-30 rad, so the phase of every sample is an exact
int64 cumulative sum; nco_exact() reduces it modulo 2 pi and takes cos / sin in np.longdouble.  The device is held to these
values at NCO_TOL; the oracle's Nco (a sequentially rounded f64 phase with a single wrap by fl(2 pi)) is held to them at
ORACLE_NCO_TOL on every input the GPU tests use (tests/test_demod_ref.py).

Timing estimator.  FILTERS are (n, d) pairs whose 2 n d + 1 taps meet every seam of timing_kernel's passes of TE_QMAX taps;
blocks are shaped QPSK under white noise of equal power, and sparse blocks of a few complex impulses on the tile edges and
the filter's and the passes' offsets from them.  Every block keeps |sum| / sum |terms| of syncest_ref.ref_sums at or above
syncest_ref.MIN_COHERENCE (an input that does not is replaced: the next seed), so that an angle can be tested on it."""
import functools

import numpy as np

import oracle
import syncest_ref as sr

TILE = 2048                                  # TE_TILE = NCO_TILE: samples per tile of timing_kernel and of the three NCO kernels
GRID = 8 * 256                               # the NCO's persistent grid (slots); the timing estimator's is 4 * 256
SWEEP = 8192                                 # tile sums nco_scan_kernel takes per sweep

# ------------------------------------------------------------------ NCO
UNIT_BITS = 30
UNIT = 2.0 ** -UNIT_BITS                     # rad
# 2 pi to the precision of np.longdouble: fl(2 pi) plus the rest
TWO_PI = np.longdouble(6.283185307179586) + np.longdouble(2.4492935982947064e-16)
NCO_TOL = 1e-9                               # the project's bound on an NCO output (tests/test_estimators.py)
# The oracle against the exact values.  Its phase is an f64 that every addition rounds and every wrap moves by 2 pi - fl(2 pi) =
# 2.4e-16; on the inputs here it stays within a few tens of rad (ulp / 2 <= 3.6e-15) and the roundings add up like a random walk.
# Measured: 1.1e-12 on the small shapes and the cut streams, 2.0e-11 past the grid, 8.1e-11 on the 2^24 + 777 block -- its
# 3.3e5 wraps times 2.4e-16, a sum that is the same on every run.  A tenth of the device's bound: the two references are
# interchangeable at NCO_TOL, and a restatement that is wrong (an index, a sign, the order of increment and output) is wrong by ~1.
ORACLE_NCO_TOL = 1e-10
RATIO_TOL = 1e-12                            # out[i] conj(out[i-1]) against exp(i (dphase + perr[i])), and | |out[i]| - 1 |: a few f64 roundings each
SMALL_ERR = 1 << 23                          # |perr| < 2^-7 rad = 0.0078: the loop-filter scale of tests/test_estimators.py
LARGE_ERR = 50 << UNIT_BITS                  # |perr| < 50 rad: several whole turns, nco_turns' rint(hi) != 0
KINDS = ("small", "large")
SMALL_N = (1, 2, 3, 511, 512, 513, 2047, 2048, 2049, 4095, 4097)
N_CUT = 3 * TILE + 5
N_BIG = (GRID + 3) * TILE + 5                # every workgroup of the sum and apply kernels takes a second tile, three a third
N_LONG = (1 << 24) + 777                     # 8193 tiles: a second sweep of the scan (tests/test_estimators.py)

D_POS = int(round(0.1234567 / UNIT))
D_NEG = -int(round(0.3 / UNIT))              # wrapped to [0, 2 pi) by Nco::new: one rounding of dphase + fl(2 pi), ~7e-16 a sample
P_NEAR_TURN = int(np.floor(2 * np.pi / UNIT))  # the last start phase below 2 pi on the grid
P_QUARTER = int(round(np.pi / 4 / UNIT))


def rad(k):
    """Grid integers as f64 radians (exact: |k| < 2^53)."""
    return np.asarray(k, dtype=np.int64).astype(np.float64) * UNIT


def nco_errors(kind, n, seed):
    """n phase errors as int64 grid integers.  "small": uniform below SMALL_ERR.  "large": uniform below LARGE_ERR.  "bounded":
    large steps b[i] - b[i-1] of a bounded sequence plus small ones, |perr| < 50 rad: the phase stays near its drift, which is
    what lets the ORACLE follow a block of millions of samples (its f64 phase would otherwise wander to 1e5 rad and lose 1e-9)."""
    rng = np.random.default_rng(seed)
    if kind == "small":
        e = rng.integers(-SMALL_ERR + 1, SMALL_ERR, n, dtype=np.int64)
    elif kind == "large":
        e = rng.integers(-LARGE_ERR + 1, LARGE_ERR, n, dtype=np.int64)
    else:
        assert kind == "bounded"
        b = rng.integers(-(LARGE_ERR // 2) + SMALL_ERR, LARGE_ERR // 2 - SMALL_ERR, n, dtype=np.int64)
        e = np.diff(b, prepend=0) + rng.integers(-SMALL_ERR + 1, SMALL_ERR, n, dtype=np.int64)
    e.setflags(write=False)
    return e


def nco_phases(p0, d, e):
    """The exact phase of every sample in grid units (int64): p0 + sum_{j <= i} (d + e[j])."""
    return p0 + np.cumsum(d + np.asarray(e, dtype=np.int64))


def rotor_exact(k):
    """exp(i k 2^-30) for int64 k: reduced modulo 2 pi and evaluated in np.longdouble, rounded to complex128."""
    ph = np.fmod(np.asarray(k, dtype=np.int64).astype(np.longdouble) * np.longdouble(UNIT), TWO_PI)
    return np.cos(ph).astype(np.float64) + 1j * np.sin(ph).astype(np.float64)


def nco_exact(p0, d, e, idx=None):
    """(outputs, phase after the block in grid units); idx: the outputs at those indices only."""
    k = nco_phases(p0, d, e)
    return rotor_exact(k if idx is None else k[idx]), int(k[-1]) if k.size else p0


def seam_indices(n, n_random=4000, seed=1):
    """Every tile seam +- 1, both ends, and n_random random indices."""
    seams = TILE * np.arange(1, (n + TILE - 1) // TILE, dtype=np.int64)
    idx = np.concatenate([[0, 1, n - 2, n - 1], seams - 1, seams, seams + 1, np.random.default_rng(seed).integers(0, n, n_random)])
    return np.unique(idx[(idx >= 0) & (idx < n)])


@functools.lru_cache(maxsize=None)
def small_cases():
    """(name, dphase, phase0, errors) in grid integers: every SMALL_N, both error ranges, dphase of either sign, and a start
    phase one grid step below 2 pi."""
    out = []
    for kind in KINDS:
        for i, n in enumerate(SMALL_N):
            out.append(("%s-n%d-pos" % (kind, n), D_POS, P_NEAR_TURN, nco_errors(kind, n, 100 + i)))
            out.append(("%s-n%d-neg" % (kind, n), D_NEG, P_QUARTER, nco_errors(kind, n, 200 + i)))
    return out


# where the cut stream is cut: calls end at these indices (and at N_CUT)
CUTS = {"at-1": (1,), "odd": (777,), "2047": (2047,), "2048": (2048,), "2049": (2049,),
        "single-samples-across-an-edge": (2 * TILE - 2, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 2 * TILE + 2),
        "every-seam": (TILE - 1, TILE, TILE + 1, 2 * TILE, 3 * TILE, 3 * TILE + 4)}


@functools.lru_cache(maxsize=None)
def cut_stream(kind):
    """(dphase, phase0, errors) of the stream that is run uncut and cut: a negative dphase on the large errors."""
    return (D_POS, P_NEAR_TURN, nco_errors(kind, N_CUT, 300)) if kind == "small" else (D_NEG, P_QUARTER, nco_errors(kind, N_CUT, 301))


@functools.lru_cache(maxsize=None)
def big_stream():
    """Past the grid: N_BIG errors, large steps and small ones."""
    return D_POS, P_QUARTER, nco_errors("bounded", N_BIG, 400)


@functools.lru_cache(maxsize=None)
def long_stream():
    """Past one sweep of the scan: N_LONG small errors."""
    return D_POS, 1 << (UNIT_BITS - 1), nco_errors("small", N_LONG, 500)


def oracle_nco(p0, d, e, cuts=()):
    """The oracle's Nco over the same stream, call by call: (outputs, its phase)."""
    nco = oracle.Nco(float(rad(d)), float(rad(p0)))
    x = rad(e)
    edges = [0] + list(cuts) + [x.size]
    return np.concatenate([nco.push(x[a:b]) for a, b in zip(edges[:-1], edges[1:])]), nco.phase.value


# ------------------------------------------------------------------ timing estimator
TE_QMAX = 1020                               # taps one pass of timing_kernel stages
ALPHA = 0.35
#          taps   passes
FILTERS = ((4, 0),      # 1      one
           (1, 1),      # 3
           (5, 1),      # 11
           (3, 2),      # 13 -> 24
           (509, 1),    # 1019 -> 1020: exactly one full pass
           (1, 509),    # the same taps at n = 1
           (10, 51),    # 1021: 1020 + 12
           (1, 1020),   # 2041: 1020 + 1020 + 12
           (3, 340),    # the same at n = 3
           (2, 650))    # 2601: 1020 + 1020 + 564
# The existing tests hold n = 10 to 1e-9 samples: an angle of 2 pi 1e-9 / 10 rad of the sum.  Every case here is held to that angle.
ANGLE_TOL = 2 * np.pi * 1e-9 / 10
KINDS_T = ("qpsk", "sparse")


def angle_error(got, want, n):
    """The distance of two estimates as an angle of the sum they are taken from (rad)."""
    return sr.circ(got, want, n) * 2 * np.pi / n


def pass_lengths(n, d):
    """comms_timing_push_dev's passes: the taps padded to a multiple of 12, in launches of at most TE_QMAX."""
    nq12 = (2 * n * d + 1 + 11) // 12 * 12
    return [min(TE_QMAX, nq12 - k) for k in range(0, nq12, TE_QMAX)]


def block_lengths(n, d):
    nd = n * d
    return sorted({nd, nd + 1, TILE - 1, TILE, TILE + 1, TILE + nd, 2 * TILE + nd + 1})


def _qpsk(n, d, length, seed):
    """QPSK at n samples per symbol under an RRC pulse (8 symbols, beta 0.5), unit power, plus white noise of unit power."""
    rng = np.random.default_rng(seed)
    n_sym = (length + 1) // n + 10
    up = np.zeros(n_sym * n, np.complex128)
    up[::n] = np.exp(1j * (np.pi / 2 * rng.integers(0, 4, n_sym) + np.pi / 4))
    taps = oracle.rrc_taps(8 * n + 1, float(n), 0.5, np.complex128)
    drop = 4 * n + (1 if n > 1 else 0)       # past the pulse's rise; the symbol peaks off the multiples of n
    y = oracle.batch_fir(up, taps, oracle.default_state(taps))[drop: drop + length]
    y = y / np.sqrt(np.mean(np.abs(y) ** 2))
    return y + np.sqrt(0.5) * (rng.standard_normal(length) + 1j * rng.standard_normal(length))


def sparse_positions(n, d, length):
    """Where a sparse block may have an impulse: the block's ends, the tile edges - 1, + 0, + 1, and those moved by the delay
    n d and by the first samples of the later passes (k_lo = 1020, 2040), either way."""
    nd = n * d
    edges = [0, length - 1] + [TILE * k + e for k in range(0, length // TILE + 2) for e in (-1, 0, 1)]
    offs = [0, nd, -nd] + [s * k for k in range(TE_QMAX, 2 * nd + 1, TE_QMAX) for s in (1, -1)]
    return sorted({p + o for p in edges for o in offs if 0 <= p + o < length})


def _sparse(n, d, length, seed):
    """Four to eight complex impulses (fewer where the block has fewer positions), all on sparse_positions and one of them at
    0 (with len = n d + 1 the single product is q[n d] d[0]).  A block that holds a tile edge T takes T - 1, T, T + 1, one of
    T +- n d and one of T +- k_lo per later pass; a shorter block a few of its positions at random."""
    rng = np.random.default_rng(seed)
    nd = n * d
    edges = [t for t in range(TILE, length + 2, TILE) if t - 1 < length]
    if edges:
        t = int(rng.choice(edges))
        near = [t - 1, t, t + 1] + [t + o if t + o < length else t - o for o in [nd] + list(range(TE_QMAX, 2 * nd + 1, TE_QMAX))]
        chosen = sorted({0} | {p for p in near if 0 <= p < length})
        rest = [p for p in sparse_positions(n, d, length) if p not in chosen]
        chosen += rng.choice(rest, min(len(rest), max(0, 4 - len(chosen))), replace=False).tolist()
    else:
        others = [p for p in sparse_positions(n, d, length) if p != 0]
        k = min(len(others), int(rng.integers(3, 8)))
        chosen = [0] + (rng.choice(others, k, replace=False).tolist() if k else [])
    x = np.zeros(length, np.complex128)
    for p in chosen:
        x[p] = (1.0 + rng.uniform()) * np.exp(2j * np.pi * rng.uniform())
    return x


def coherence(x, n, d, alpha=ALPHA):
    """|sum| / sum |terms| of the timing sum; None where the block forms no product."""
    ts, _, ta, _ = sr.ref_sums(x, n, d, alpha)
    return abs(ts) / ta if ta > 0 else None


@functools.lru_cache(maxsize=None)
def timing_block(kind, n, d, length, margin=2.0):
    """The block of (kind, n, d, length): the first seed whose coherence is at least margin * MIN_COHERENCE (any seed where
    the block is too short to form a product)."""
    make = _qpsk if kind == "qpsk" else _sparse
    for seed in range(64):
        x = make(n, d, length, 7919 * seed + 100 * n + d + length) if length else np.zeros(0, np.complex128)
        c = coherence(x, n, d) if length > n * d else None
        if length <= n * d or (c is not None and c >= margin * sr.MIN_COHERENCE):
            x.setflags(write=False)
            return x
    raise AssertionError("no coherent %s block for n=%d d=%d len=%d" % (kind, n, d, length))


@functools.lru_cache(maxsize=None)
def timing_cases():
    """(kind, n, d, length) of every block tests/test_gpu_demod_seams.py estimates."""
    return [(kind, n, d, ln) for n, d in FILTERS for ln in block_lengths(n, d) for kind in KINDS_T]


@functools.lru_cache(maxsize=None)
def timing_reference(kind, n, d, length):
    """The oracle's estimate of that block, computed once."""
    return oracle.timing_push(timing_block(kind, n, d, length), n, d, ALPHA)
