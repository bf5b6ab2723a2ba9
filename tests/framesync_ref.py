"""Reference material of the frame synchroniser (comms_framesync_*), shared by tests/test_framesync_ref.py (CPU) and
tests/test_gpu_framesync.py:

  ref_detect    the definition of include/comms_hip.h in f64, whole stream at once, the k >= 0 rule and a flush included.
  model_detect  the ARITHMETIC of framesync_kernel: f32, j ascending from +0, one FMA per real product (an FMA is emulated as
                the f64 sum of the exact product, rounded to f32), the metric with every operation rounded on its own.
  WORDS, cases  every word and every block the GPU test runs, so that the CPU test measures the model on exactly those.
  dense_*       streams on which every position is a detection, and the positions whose model metric serves as the threshold
                (tests/test_gpu_dense_metrics.py compares the kernel with model_detect bit for bit).
"""
import functools

import numpy as np

import oracle
import rx_ref
from ofdmsync_ref import fma32
import symsync_ref
import syncest_ref

TILE = 2048          # decided positions per tile of framesync_kernel (the GPU test checks it against comms_framesync_get_kernel)
GRID_CAP = 8 * 256   # no persistent grid of the library exceeds eight workgroups on each of 256 CUs (resident_workgroups)
N_BIG = (GRID_CAP + 1) * TILE + 5   # every workgroup walks at least two tiles, whatever the grid

# Largest distance of model_detect from ref_detect over cases(), measured by tests/test_framesync_ref.py (which asserts
# that they still hold): the metric (absolute; it lies in [0, 1]) and the correlation relative to sqrt(Ep e) -- the energy, relative to itself, shares that figure.
MODEL_METRIC_DISTANCE = 1.4e-6   # measured 1.382e-6: "w512-B" (512 taps: about sqrt(P) ulps of a metric near 1); 13 ... 63 taps: below 4.2e-7
MODEL_CORR_DISTANCE = 7.6e-7     # measured 7.571e-7: "w512-A", its energy (a chain of 1024 f32 additions)
# The same over EVERY position of the dense streams (dense_stream: thousands of positions each, where cases() has a few
# detections).  The metric stays inside MODEL_METRIC_DISTANCE (9.70e-7, qpsk512); the sums do not: no GPU tolerance rests on
# this one (the dense GPU tests compare bits), it records how far the chosen order lies from the definition.
DENSE_CORR_DISTANCE = 1.29e-6    # measured 1.282e-6: qpsk512, the energy; its correlation 4.58e-7; 2 ... 63 taps: below 4.6e-7
# The GPU tolerances: four times those (the kernel may fuse where the model does not).
METRIC_TOL = 4 * MODEL_METRIC_DISTANCE
CORR_TOL = 4 * MODEL_CORR_DISTANCE
# Every f64 metric of every case keeps this distance from the threshold, and every detection beats the metrics of its guard
# window by it (exact ties of identical windows excepted): at least eight times MODEL_METRIC_DISTANCE, so that no rounding
# within METRIC_TOL on either side of a comparison can flip a decision.  A case that violates it is replaced, not tolerated.
DECISION_MARGIN = 2.0e-5
SIGMA = 0.05         # noise per real component, relative to the symbol amplitude A of the stream


# ------------------------------------------------------------------ the two statements of the contract
def _pad(y, P, G, dtype):
    """y with the zeros the definition puts around it: P + G - 1 in front (y[i] = 0 for i < 0: positions -(G + P - 1) ... are
    the neighbours of position 0), P + G behind (the flush)."""
    y = np.asarray(y).astype(dtype)
    return np.concatenate([np.zeros(P + G - 1, dtype), y, np.zeros(P + G, dtype)])


def _decide(m, k0, thr, G, n_pos):
    """Positions 0 <= k < n_pos that the rule selects; m[i] is the metric of position k0 + i (k0 = -G)."""
    with np.errstate(invalid="ignore"):
        cand = np.nonzero(m[G: G + n_pos] >= thr)[0]
    out = []
    for k in cand:
        i = k + G
        if G == 0 or (np.all(m[i] > m[i - G: i]) and np.all(m[i] >= m[i + 1: i + G + 1])):
            out.append(k)
    return np.array(out, np.int64)


def ref_detect(y, p, thr, G):
    """f64: (index, c, m, e) arrays of the detections of the whole stream y, flushed; and the metrics of positions
    -G ... len(y) + G - 1 for the margin checks, as the fifth value."""
    p = np.asarray(p).astype(np.complex128)
    P, T = p.size, len(y)
    yp = _pad(y, P, G, np.complex128)                       # position k at yp[k + P + G - 1]
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.correlate(yp, p, "valid")                    # c[i] = sum_j yp[i + j] conj(p[j]): position i - (P + G - 1)
        e = np.correlate(yp.real ** 2 + yp.imag ** 2, np.ones(P), "valid")
        Ep = float(np.float32(np.sum(p.real ** 2 + p.imag ** 2)))
        m = np.where(e == 0.0, 0.0, (c.real ** 2 + c.imag ** 2) / (Ep * np.where(e == 0.0, 1.0, e)))
    lo = P - 1                                              # index of position -G
    m, c, e = m[lo: lo + T + 2 * G], c[lo: lo + T + 2 * G], e[lo: lo + T + 2 * G]
    idx = _decide(m, -G, thr, G, T)
    return idx, c[idx + G], m[idx + G], e[idx + G], m


def _fma(a, b, acc):
    return fma32(a, b, acc)      # one rounding, as the hardware's: the f64 sum of the exact product, rounded to f32, tie-corrected


def model_sums(y, p, G):
    """framesync_kernel's arithmetic at the positions -G ... len(y) + G - 1: (cr, ci, e, m) as float32."""
    f32 = np.float32
    p = np.asarray(p).astype(np.complex64)
    P, T = p.size, len(y)
    yp = _pad(np.asarray(y, np.complex64), P, G, np.complex64)
    n = T + 2 * G
    yr, yi = yp.real.astype(f32)[P - 1:], yp.imag.astype(f32)[P - 1:]      # element i + j: tap j of position i - G
    cr, ci, e = np.zeros(n, f32), np.zeros(n, f32), np.zeros(n, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(P):
            ar, ai = yr[j: j + n], yi[j: j + n]
            pr, pi = np.full(n, p[j].real, f32), np.full(n, p[j].imag, f32)
            cr = _fma(ar, pr, cr)
            ci = _fma(ai, pr, ci)
            cr = _fma(ai, pi, cr)
            ci = _fma(-ar, pi, ci)
            e = _fma(ar, ar, e)
            e = _fma(ai, ai, e)
        Ep = f32(np.sum(p.real.astype(np.float64) ** 2 + p.imag.astype(np.float64) ** 2))
        num = (cr * cr) + (ci * ci)
        den = Ep * e
        m = np.where(e == 0, f32(0), num / np.where(e == 0, f32(1), den)).astype(f32)
    return cr, ci, e, m


def model_detect(y, p, thr, G, sums=None):
    """framesync_kernel's arithmetic: (index, c as complex64 parts in complex128, m, e, all metrics) as ref_detect; `sums` are
    model_sums(y, p, G) where the caller holds them."""
    cr, ci, e, m = model_sums(y, p, G) if sums is None else sums
    idx = _decide(m, -G, np.float32(thr), G, len(y))
    c = cr.astype(np.float64) + 1j * ci.astype(np.float64)
    return idx, c[idx + G], m[idx + G].astype(np.float64), e[idx + G].astype(np.float64), m


def ref_detect_cut(y, p, thr, G, cuts):
    """The streaming statement: the stream cut at `cuts`, each call deciding exactly its n new positions k <= T - P - G from the
    H = P + 2 G - 1 symbols kept, and a flush.  Returns the indices in the order found."""
    P = len(p)
    H = P + 2 * G - 1
    hist = np.zeros(H, np.complex128)
    T, out = 0, []
    y = np.asarray(y).astype(np.complex128)
    pieces = np.split(y, cuts) + [np.zeros(P + G, np.complex128)]
    for piece in pieces:
        n = piece.size
        if not n:
            continue
        ext = np.concatenate([hist, piece])              # symbol T - H + i at ext[i]
        k_first = T - (P + G) + 1                        # its window starts at ext[G]
        pp = np.asarray(p).astype(np.complex128)
        with np.errstate(invalid="ignore"):
            c = np.correlate(ext, pp, "valid")           # ext index i: position T - H + i = k_first - G + i
            e = np.correlate(ext.real ** 2 + ext.imag ** 2, np.ones(P), "valid")
            Ep = float(np.float32(np.sum(pp.real ** 2 + pp.imag ** 2)))
            m = np.where(e == 0.0, 0.0, (c.real ** 2 + c.imag ** 2) / (Ep * np.where(e == 0.0, 1.0, e)))
        assert m.size == n + 2 * G
        for q in _decide(m, -G, thr, G, n):
            if k_first + q >= 0:
                out.append(k_first + q)
        hist = ext[n:]
        T += n
    return np.array(out, np.int64)


# ------------------------------------------------------------------ words
def _msequence63():
    """63 bits of the m-sequence of x^6 + x + 1 from the oracle's PRNS (8-bit register, feedback from the two oldest of its
    six youngest bits; the first eight outputs are the register's initial content)."""
    bits, _ = oracle.prns_u8(0x30, 0x01, 8 + 63)
    return bits[8:].astype(np.int64)


@functools.lru_cache(maxsize=None)
def words():
    barker = np.array([1, 1, 1, 1, 1, -1, -1, 1, 1, -1, 1, -1, 1], np.complex64)
    mseq = (1 - 2 * _msequence63()).astype(np.complex64)
    q32 = rx_ref.QPSK_DEF[np.random.default_rng(32).integers(0, 4, 32)]
    q512 = rx_ref.QPSK_DEF[np.random.default_rng(512).integers(0, 4, 512)]
    out = {"barker13": barker, "mseq63": mseq, "qpsk32": q32, "p2": np.array([1, -1], np.complex64), "qpsk512": q512}
    for w in out.values():
        w.setflags(write=False)
    return out


# name -> (threshold, guard).  A payload of random QPSK against a BPSK word of P symbols has metrics near the exponential law of
# mean 1 / P: short words need the higher threshold.
SETUP = {"barker13": (0.8, 12), "mseq63": (0.5, 62), "qpsk32": (0.5, 31), "p2": (0.8, 0), "qpsk512": (0.5, 511)}


# ------------------------------------------------------------------ streams
def stream(word, positions, length, A, theta, seed, noise=True):
    """Seeded QPSK payload with the word planted at `positions`, plus noise of SIGMA per component, times A exp(i theta):
    the noise is relative to the amplitude, so that the three amplitudes are the same stream at the same signal-to-noise
    ratio (the metric does not depend on A).  Complex<f32>."""
    rng = np.random.default_rng(seed)
    s = rx_ref.QPSK_DEF[rng.integers(0, 4, length)].astype(np.complex128)
    for k in positions:
        s[k: k + len(word)] = word
    if noise:
        s = s + SIGMA * (rng.standard_normal(length) + 1j * rng.standard_normal(length))
    out = (s * (A * np.exp(1j * theta))).astype(np.complex64)
    out.setflags(write=False)
    return out


def _zeros_with(word, positions, length):
    s = np.zeros(length, np.complex64)
    for k in positions:
        s[k: k + len(word)] = word
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def cases():
    """(name, word name, threshold, guard, y, ties): every block the GPU test runs whole (run + flush); `ties` marks the cases
    whose equal metrics are exact ties of identical windows."""
    W = words()
    out = []
    for wi, (wn, w) in enumerate(W.items()):
        thr, G = SETUP[wn]
        P = w.size
        tag = {"barker13": "w13", "mseq63": "w63", "qpsk32": "w32", "p2": "w2", "qpsk512": "w512"}[wn]
        # the planted positions 0, 1, TILE - P, TILE - 1, TILE, TILE + 1 over three streams, one per amplitude
        out.append((tag + "-A", wn, thr, G, stream(w, [0, TILE - P, TILE], TILE + 2 * P + G + 37, 1.0, 0.7, 10 * wi + 1), False))
        # ... and, since position k of a single call is decided as the kernel's position k + P + G - 1, the last position of
        # its first tile and the first of its second
        edge = TILE - (P + G) + 1
        out.append((tag + "-B", wn, thr, G, stream(w, [1] + ([edge - 1] if G else []) + [TILE - 1], TILE + 2 * P + G + 11, 1e-3, 2.1,
                                                   10 * wi + 2), False))
        out.append((tag + "-C", wn, thr, G, stream(w, [edge, TILE + 1], TILE + 2 * P + G + 5, 1e3, -1.3, 10 * wi + 3), False))
    b = W["barker13"]
    G = 20
    out.append(("two-apart-G+1", "barker13", 0.8, G, stream(b, [100, 100 + G + 1], 300, 1.0, 0.4, 101), False))
    out.append(("two-apart-G", "barker13", 0.8, G, stream(b, [100, 100 + G], 300, 1.0, 0.4, 102), False))
    out.append(("largest-guard", "barker13", 0.8, 512, stream(b, [100, 613, 1400], 2100, 1.0, 0.4, 106), False))   # 613 - 100 = G + 1
    out.append(("tie-repeat", "barker13", 0.8, 16, _zeros_with(b, [50, 63, 76, 200, 213], 300), True))
    out.append(("all-zero", "barker13", 0.8, 12, _zeros_with(b, [], 257), True))
    const = np.full(300, 0.5 - 0.25j, np.complex64)
    const.setflags(write=False)
    out.append(("constant", "barker13", 0.8, 12, const, True))
    out.append(("constant-p2", "p2", 0.8, 0, const, True))
    nan = stream(b, [100, 295, 400], 500, 1.0, 0.9, 103).copy()
    nan[300] = np.complex64(complex(np.nan, 1.0))
    nan.setflags(write=False)
    out.append(("one-nan", "barker13", 0.8, 12, nan, False))
    out.append(("shorter-than-word", "barker13", 0.8, 12, stream(b, [], 5, 1.0, 0.0, 104), False))
    # past the grid: noise alone except a word in the first, a middle and the last tile
    rng = np.random.default_rng(105)
    big = (SIGMA * (rng.standard_normal(N_BIG) + 1j * rng.standard_normal(N_BIG))).astype(np.complex64)
    # (twenty more along the way: more detections in one call than come back with the count)
    for k in [7, (GRID_CAP // 2) * TILE + TILE - 5, N_BIG - 20] + [100003 + 200003 * i for i in range(20)]:
        big[k: k + 13] = (b * np.exp(0.3j)).astype(np.complex64) + big[k: k + 13]
    big.setflags(write=False)
    out.append(("past-the-grid", "barker13", 0.8, 12, big, False))
    return out


@functools.lru_cache(maxsize=None)
def reference(idx):
    """ref_detect of case idx, computed once: dict(index, c, m, e, metrics)."""
    _, wn, thr, G, y, _ = cases()[idx]
    k, c, m, e, mm = ref_detect(y, words()[wn], thr, G)
    for a in (k, c, m, e, mm):
        a.setflags(write=False)
    return dict(index=k, c=c, m=m, e=e, metrics=mm)


def case(name):
    return [i for i, cs in enumerate(cases()) if cs[0] == name][0]


# ------------------------------------------------------------------ dense streams (tests/test_gpu_dense_metrics.py)
# With G = 0 the peak rule is "m >= thr": under a tiny threshold every position is a detection, and the metric of the kernel's
# register-window path decides at every position what the scalar loop then reports.
DENSE_N = 2 * TILE + 77        # positions whose whole word lies in the stream: two tiles and a ragged third
DENSE_THR = 1e-30
DENSE_WORDS = ("p2", "barker13", "qpsk32", "mseq63", "qpsk512")
DENSE_FAR_WORDS = ("p2", "barker13", "qpsk512")                      # run again at positions past 2^32
PASS = 2048                    # metrics per pass of a workgroup (256 lanes of eight): FS_PASS
LATE_GUARD = 8                 # the least guard whose second, partial pass holds all eight lane columns as decided positions


@functools.lru_cache(maxsize=None)
def dense_stream(wn):
    """DENSE_N + P - 1 symbols of stream(): a QPSK payload with noise everywhere, the word planted twice."""
    P = words()[wn].size
    return stream(words()[wn], [300, TILE + 900], DENSE_N + P - 1, 1.0, 0.7, 900 + P)


@functools.lru_cache(maxsize=None)
def dense_sums(wn, G=0):
    out = model_sums(dense_stream(wn), words()[wn], G)
    for a in out:
        a.setflags(write=False)
    return out


def dense_detect(wn, thr, G=0):
    """model_detect of the dense stream: (index, c, m, e, all metrics)."""
    return model_detect(dense_stream(wn), words()[wn], thr, G, sums=dense_sums(wn, G))


def first_pass_picks(wn):
    """{column: k} at G = 0: metric index r of a single call's tile is position k = r - (P - 1) (mod TILE), its lane column r mod
    8.  Per column a position with the whole word in the stream and a model metric between the 20th and the 80th percentile:
    the first such at or behind column * DENSE_N / 8, so that the eight lie in different lanes and tiles."""
    P = words()[wn].size
    m = dense_sums(wn)[3][:DENSE_N]
    lo, hi = np.percentile(m, [20, 80])
    k = np.flatnonzero((m >= lo) & (m <= hi))
    return {col: int(k[((k + P - 1) % 8 == col) & (k >= col * DENSE_N // 8)][0]) for col in range(8)}


def late_pass_picks(wn):
    """{column: (k, n1)} at G = LATE_GUARD: metric PASS + column of a tile is computed by the second, partial pass, and is decided
    position r = PASS + column - G.  A peak k of the model lands there in the second of two calls when the first one takes
    n1 = k - r + P + G - 1 symbols (the second call's first decided position is n1 - (P + G) + 1).  The peaks are the model's
    under DENSE_THR with metrics between the 20th and 80th percentile of all peaks, eight of them spread over that range."""
    P, G = words()[wn].size, LATE_GUARD
    T = dense_stream(wn).size
    idx, _, m, _, _ = dense_detect(wn, DENSE_THR, G)
    lo, hi = np.percentile(m, [20, 80])
    ok = (m >= lo) & (m <= hi) & (idx >= PASS + 7 - G - P - G + 1) & (idx <= T - P - G)
    idx = idx[ok][np.argsort(m[ok], kind="stable")]
    out = {}
    for col in range(8):
        k = int(idx[col * idx.size // 8])
        out[col] = (k, k - (PASS + col - G) + P + G - 1)
    return out


# ------------------------------------------------------------------ the loop the node exists for
LOOP_WORD, LOOP_THR, LOOP_FRONT, LOOP_NPAY = "qpsk32", 0.5, 40, syncest_ref.LOOP_NSYM
LOOP_QUARTERS = (0, 1, 2, 3)


@functools.lru_cache(maxsize=None)
def loop_signal(dd, quarter):
    """(payload values, x as Complex<f32>, prototype h): LOOP_FRONT random symbols, the word, then LOOP_NPAY QPSK symbols of
    known values; RRC pulse, delayed by dd / L samples, rotated by LOOP_PHASE plus `quarter` quarter turns -- the rotation the
    4th-power estimate cannot see.  syncest_ref.loop_signal with a word in front."""
    sr = syncest_ref
    rng = np.random.default_rng(78)
    front = rx_ref.QPSK_DEF[rng.integers(0, 4, LOOP_FRONT)]
    v = rng.integers(0, 4, LOOP_NPAY)
    tail = rx_ref.QPSK_DEF[rng.integers(0, 4, 2 * sr.LOOP_NP)]       # keeps the last payload symbols clear of the stream's end
    sym = np.concatenate([front, words()[LOOP_WORD], rx_ref.QPSK_DEF[v], tail]).astype(np.complex128)
    x = symsync_ref.fractional_delay(sym, sr.LOOP_NP, sr.LOOP_S, sr.LOOP_L, sr.LOOP_BETA, dd, oracle.rrc_taps, oracle.pulse)
    x = (x * np.exp(1j * (sr.LOOP_PHASE + quarter * np.pi / 2))).astype(np.complex64)
    N = (sr.LOOP_NP - 1) * sr.LOOP_L + 1
    h = oracle.rrc_taps(N, float(sr.LOOP_L * sr.LOOP_S), sr.LOOP_BETA, np.complex128).real.astype(np.float32)
    return v, x, h
