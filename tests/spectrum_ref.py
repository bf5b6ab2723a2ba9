"""The definition of the spectrum estimator (include/comms_hip.h, "spectrum estimator") in numpy float64, the case table of the
GPU tests and their bounds: test infrastructure, no GPU.  Nothing here comes from a kernel's output.

  segments_before(T, N, H)   S(T), the segments completed before stream position T
  out_len(T, n, N, H, K)     rows of a call on [T, T + n)
  ref_rows(x, w, H, K, ...)  the rows of a whole stream from position 0: np.fft.fft of the windowed segments, |.|^2, the sum
                             of K segments, times scale -- in float64, so the order of the sums does not matter here
  row_bound / bin_bound      what an f32 implementation of the contract may differ by (derived below)
"""
import math

import numpy as np

SIZES = (64, 128, 256, 512, 1024)
CHUNK = 32                     # COMMS_SPECTRUM_CHUNK
AVGS = (1, 3, 32, 33, 65, 97)  # one chunk; the chunk boundary; two chunks and one segment; three chunks and one segment
FFT_BOUND = 1e-5               # the project's f32 transform bound (ofdm_ref.FFT_BOUND, tests/test_gpu_fft_lengths.py)


def hops(n_fft):
    """No overlap, half, an odd hop below half (an odd sample offset for every second segment), a hop that skips samples; and
    at the smallest size the densest overlap."""
    return (n_fft, n_fft // 2, 3 * n_fft // 8 + 1, n_fft + 5) + ((1,) if n_fft == 64 else ())


def cases():
    """(n_fft, hop) of the accuracy test; each runs every K of AVGS."""
    return [(n, h) for n in SIZES for h in hops(n)]


def n_samples(n_fft, hop, avg):
    """Three (K >= 65) or four rows' worth of samples and a ragged tail that ends inside a row, a chunk and a segment."""
    rows = 3 if avg >= 65 else 4
    segs = rows * avg + avg // 2
    return n_fft + (segs - 1) * hop + hop // 3 + 7


def segments_before(T, n_fft, hop):
    return (T - n_fft) // hop + 1 if T >= n_fft else 0


def out_len(T, n, n_fft, hop, avg):
    return segments_before(T + n, n_fft, hop) // avg - segments_before(T, n_fft, hop) // avg


def brute_out_len(T, n, n_fft, hop, avg):
    """The same by enumeration: the segments with T < s H + N <= T + n, and the rows whose last segment is among them."""
    rows, s = 0, 0
    while s * hop + n_fft <= T + n:
        if s * hop + n_fft > T and s % avg == avg - 1:
            rows += 1
        s += 1
    return rows


def window(kind, n):
    """The periodic windows of comms_window_taps, float64."""
    a = {"rect": (1.0, 0.0, 0.0), "hann": (0.5, 0.5, 0.0), "hamming": (0.54, 0.46, 0.0), "blackman": (0.42, 0.5, 0.08)}[kind]
    t = 2.0 * np.pi * np.arange(n) / n
    return a[0] - a[1] * np.cos(t) + a[2] * np.cos(2.0 * t)


def segment_powers(x, w, hop):
    """|FFT(w x[s H : s H + N])|^2 for every whole segment of x: (segments, N) float64."""
    n_fft = len(w)
    x = np.asarray(x, np.complex128)
    n_seg = segments_before(len(x), n_fft, hop)
    idx = np.arange(n_seg)[:, None] * hop + np.arange(n_fft)[None, :]
    X = np.fft.fft(x[idx] * np.asarray(w, np.float64)[None, :], axis=1)
    return X.real ** 2 + X.imag ** 2


def ref_rows(x, w, hop, avg, scale, order="natural"):
    p = segment_powers(x, w, hop)
    rows = p.shape[0] // avg
    out = scale * p[: rows * avg].reshape(rows, avg, len(w)).sum(axis=1)
    return np.fft.fftshift(out, axes=1) if order == "centred" else out


def psd_scale(w, avg):
    return float(1.0 / (avg * np.sum(np.asarray(w, np.float64) ** 2)))


def signal(n, seed):
    """Seeded complex noise of unit variance plus two tones, one on a bin centre of every size and one between bins."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * math.sqrt(0.5)
    x += 3.0 * np.exp(2j * np.pi * (5.0 / 64.0) * t) + 0.5 * np.exp(2j * np.pi * (-0.2371) * t + 0.3j)
    return x.astype(np.complex64)


# ---- bounds ------------------------------------------------------------------------------------------------------------------
# Let B = FFT_BOUND: the f32 transform returns X + d with ||d|| <= B ||X|| (2-norm over the bins).  Then per bin
#   | |X + d|^2 - |X|^2 | <= 2 |X| |d| + |d|^2 <= 2 B sqrt(P_k sum P) + B^2 sum P       (|d_k| <= ||d|| <= B sqrt(sum P))
# and over a row, by Cauchy-Schwarz, sum_k 2 |X_k| |d_k| <= 2 ||X|| ||d||: at most (2 B + B^2) sum P.  A row is a sum of such
# terms over its segments and sqrt(P_k,s sum P_s) summed over s is at most sqrt(P_k sum P) of the row (Cauchy-Schwarz again).
# The f32 steps around the transform are sums and products of non-negative terms, so their relative errors (2^-24 each) add
# and never cancel: a value passes at most 32 additions of its chunk sum, ceil(K / 32) of its row sum, and three more steps
# (the window multiply, whose error the square doubles, the power and the scale, to first order):
#   e = (32 + ceil(K / 32) + 3) 2^-24
def eps_sum(avg):
    return (CHUNK + -(-avg // CHUNK) + 3) * 2.0 ** -24


def row_bound(P, avg):
    """Bound of sum_k |got - P| per row; P the reference rows (rows, N)."""
    return (2 * FFT_BOUND + FFT_BOUND ** 2 + eps_sum(avg)) * P.sum(axis=1)


def bin_bound(P, avg):
    """Bound of |got_k - P_k|, (rows, N)."""
    tot = P.sum(axis=1, keepdims=True)
    return 2 * FFT_BOUND * np.sqrt(P * tot) + FFT_BOUND ** 2 * tot + eps_sum(avg) * P


def check_rows(got, P, avg, what=""):
    """Prints the worst figure of either bound as a share of the bound, then asserts both."""
    got = np.asarray(got, np.float64)
    assert got.shape == P.shape, (what, got.shape, P.shape)
    if not P.size:
        return
    err = np.abs(got - P)
    row_share = float(np.max(err.sum(axis=1) / row_bound(P, avg)))
    bin_share = float(np.max(err / bin_bound(P, avg)))
    print("%s rows=%d row error / bound = %.3f, bin error / bound = %.3f" % (what, P.shape[0], row_share, bin_share))
    assert row_share <= 1.0, (what, "row", row_share)
    assert bin_share <= 1.0, (what, "bin", bin_share)
