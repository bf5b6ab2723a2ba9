"""The definition of the OFDM modulator and demodulator (include/comms_hip.h, "OFDM modulator and demodulator") in numpy
complex128, an f32 model of the kernels' arithmetic, and the formats, inputs and case tables that tests/test_ofdm_ref.py
(no GPU) and tests/test_gpu_ofdm.py share.  Nothing here touches the library."""
import numpy as np

NULL, DATA, PILOT = 0, 1, 2

# ---------------------------------------------------------------- carrier maps (bin 0 = DC, bin N - k = frequency -k)


def map_80211a():
    """52 used carriers of 64 as in 802.11a: -26 ... 26 without DC, pilots at -21, -7, 7, 21."""
    kind = np.zeros(64, np.uint8)
    for f in range(-26, 27):
        if f:
            kind[f % 64] = PILOT if abs(f) in (7, 21) else DATA
    return kind


def map_all_data(n):
    return np.full(n, DATA, np.uint8)


def map_single(n, k=5):
    kind = np.zeros(n, np.uint8)
    kind[k] = DATA
    return kind


def map_generic(n):
    """DC and the outer eighth on each side null, a pilot every 16th frequency, data elsewhere."""
    kind = np.zeros(n, np.uint8)
    edge = n // 2 - n // 8
    for f in range(-edge, edge + 1):
        if f:
            kind[f % n] = PILOT if f % 16 == 8 else DATA
    return kind


def unit_points(n, seed):
    """n points of modulus 1 with random phases (complex64): non-zero training and pilot values."""
    return np.exp(2j * np.pi * np.random.default_rng(seed).random(n)).astype(np.complex64)


class Format:
    """One handle's arguments; everything the definition needs."""

    def __init__(self, n_fft, n_cp, kind, n_syms, n_train=0, polarity=None, cpe=False, tx_scale=None, seed=1):
        self.n_fft, self.n_cp, self.n_syms, self.n_train, self.cpe = n_fft, n_cp, n_syms, n_train, cpe
        self.kind = np.asarray(kind, np.uint8)
        self.data_bins = np.flatnonzero(self.kind == DATA)
        self.pilot_bins = np.flatnonzero(self.kind == PILOT)
        self.pilots = unit_points(self.pilot_bins.size, seed + 100)
        self.polarity = None if polarity is None else np.asarray(polarity, np.float32)
        self.train = unit_points(n_fft, seed + 200)   # given on every bin, null bins included
        self.tx_scale = np.float32(1.0 / np.sqrt(n_fft)) if tx_scale is None else np.float32(tx_scale)

    D = property(lambda self: self.data_bins.size)
    data_syms = property(lambda self: self.n_syms * self.D)
    sym_len = property(lambda self: self.n_fft + self.n_cp)
    frame_samples = property(lambda self: (self.n_train + self.n_syms) * self.sym_len)

    def pol(self, s):
        return 1.0 if self.polarity is None else float(self.polarity[s % self.polarity.size])

    def but(self, **kw):
        """The same format with some attributes replaced."""
        f = Format.__new__(Format)
        f.__dict__.update(self.__dict__)
        f.__dict__.update(kw)
        return f

    def node_args(self):
        """Positional and keyword arguments of OfdmModNode / OfdmDemodNode."""
        return (self.n_fft, self.n_cp, self.kind), dict(pilots=self.pilots if self.pilots.size else None, polarity=self.polarity,
                                                       train=self.train if self.n_train else None, n_train=self.n_train,
                                                       n_syms=self.n_syms, cpe=self.cpe, tx_scale=float(self.tx_scale))


POLARITY = (1.0, -1.0, 1.0, 1.0, -1.0)
# The formats of the issue: the smallest at which the kernels can go wrong.  Symbols per wave are 1024 / N, per workgroup round
# 4096 / N: S = 3 at N = 64 is ragged against both, S = 9 at N = 512 makes a second, ragged round (and two blocks per frame).
FORMATS = {
    "n64_11a": Format(64, 16, map_80211a(), 3, 2, POLARITY, seed=1),
    "n64_all": Format(64, 16, map_all_data(64), 3, 2, seed=2),
    "n64_single": Format(64, 16, map_single(64), 3, 2, seed=3),
    "n128_cp9": Format(128, 9, map_generic(128), 5, 2, POLARITY, seed=4),
    "n256_cp0": Format(256, 0, map_all_data(256), 4, 0, seed=5),
    "n256_cpN": Format(256, 256, map_generic(256), 4, 2, POLARITY, seed=6),
    "n512_cp36": Format(512, 36, map_generic(512), 9, 2, POLARITY, seed=7),
    "n1024_cp72": Format(1024, 72, map_generic(1024), 2, 2, POLARITY, seed=8),
}
CHANNEL_FORMATS = tuple(k for k, f in FORMATS.items() if f.n_train == 2 and f.n_cp >= 2)   # check 3: the prefix covers the channel
CPE_FORMATS = tuple(k for k in CHANNEL_FORMATS if FORMATS[k].pilot_bins.size)               # check 4
FRAME_COUNTS = (1, 5)

# ---------------------------------------------------------------- the definition, complex128


def dft_direct(x, sign):
    """O(N^2): X_k = sum_n x[n] e^{sign 2 pi i k n / N} along the last axis."""
    n = x.shape[-1]
    k = np.arange(n)
    return np.asarray(x, np.complex128) @ np.exp(sign * 2j * np.pi * np.outer(k, k) / n)


def freq_values(f, syms):
    """X[frame, symbol, bin] of every transmitted symbol, training first."""
    syms = np.asarray(syms, np.complex128).reshape(-1, f.n_syms, f.D)
    X = np.zeros((syms.shape[0], f.n_train + f.n_syms, f.n_fft), np.complex128)
    X[:, : f.n_train, :] = f.train.astype(np.complex128)
    X[:, f.n_train:, f.data_bins] = syms
    for s in range(f.n_syms):
        X[:, f.n_train + s, f.pilot_bins] = f.pilots.astype(np.complex128) * f.pol(s)
    return X


def ref_mod(f, syms):
    """(n_frames, frame_samples) complex128."""
    X = freq_values(f, syms)
    x = np.fft.ifft(X, axis=-1) * f.n_fft * float(f.tx_scale)
    out = np.concatenate([x[..., f.n_fft - f.n_cp:], x], axis=-1)
    return out.reshape(X.shape[0], -1)


def ref_spectra(f, rx):
    """Y[frame, symbol, bin] behind prefix removal."""
    y = np.asarray(rx, np.complex128).reshape(-1, f.n_train + f.n_syms, f.sym_len)[..., f.n_cp:]
    return np.fft.fft(y, axis=-1)


def ref_demod(f, rx):
    """(n_frames, data_syms) complex128."""
    Y = ref_spectra(f, rx)
    used = f.kind != NULL
    Z = np.zeros_like(Y[:, f.n_train:, :])
    if f.n_train:
        H = Y[:, : f.n_train, used].sum(axis=1) / f.n_train / f.train[used].astype(np.complex128)
        Z[..., used] = Y[:, f.n_train:, used] / H[:, None, :]
    else:
        Z[..., used] = Y[:, :, used] / (f.n_fft * float(f.tx_scale))
    out = Z[..., f.data_bins]
    if f.cpe:
        for s in range(f.n_syms):
            c = (Z[:, s, f.pilot_bins] * np.conj(f.pilots.astype(np.complex128) * f.pol(s))).sum(axis=-1)
            ok = np.isfinite(c) & (np.abs(c) > 0)
            out[:, s, :] *= np.where(ok, np.conj(c) / np.where(ok, np.abs(c), 1.0), 1.0)[:, None]
    return out.reshape(Y.shape[0], -1)

# ---------------------------------------------------------------- the f32 model of the kernels' arithmetic


def fft_f32(x, sign):
    """Radix-2 decimation-in-time transform along the last axis with every operation in f32 and twiddles from an f64 table
    rounded once: log2 N rounded stages, where the kernels make two or three."""
    x = np.asarray(x, np.complex64)
    n = x.shape[-1]
    bits = n.bit_length() - 1
    rev = np.array([int(format(i, "0%db" % bits)[::-1], 2) for i in range(n)])
    a = x[..., rev]
    w = np.exp(sign * 2j * np.pi * np.arange(n // 2) / n).astype(np.complex64)
    h = 1
    while h < n:
        a = a.reshape(x.shape[:-1] + (n // (2 * h), 2, h))
        lo, hi = a[..., 0, :], (a[..., 1, :] * w[:: n // (2 * h)]).astype(np.complex64)
        a = np.stack([lo + hi, lo - hi], axis=-2).astype(np.complex64).reshape(x.shape)
        h *= 2
    return a


def model_demod(f, rx):
    """ref_demod with f32 arithmetic throughout (complex64): the transform above, the training sum in symbol order, one
    division per bin, the pilot sum in bin order."""
    y = np.asarray(rx, np.complex64).reshape(-1, f.n_train + f.n_syms, f.sym_len)[..., f.n_cp:]
    Y = fft_f32(y, -1)
    used = f.kind != NULL
    Z = np.zeros_like(Y[:, f.n_train:, :])
    if f.n_train:
        acc = np.zeros_like(Y[:, 0, :])
        for t in range(f.n_train):
            acc = (acc + Y[:, t, :]).astype(np.complex64)
        tt = (np.float64(f.n_train) * f.train.astype(np.complex128)).astype(np.complex64)
        inv = (tt[used] / acc[:, used]).astype(np.complex64)
        Z[..., used] = (Y[:, f.n_train:, used] * inv[:, None, :]).astype(np.complex64)
    else:
        Z[..., used] = (Y[:, :, used] * np.float32(1.0 / (f.n_fft * np.float64(f.tx_scale)))).astype(np.complex64)
    out = Z[..., f.data_bins].copy()
    if f.cpe:
        for s in range(f.n_syms):
            c = np.zeros(Y.shape[0], np.complex64)
            for p, v in zip(f.pilot_bins, f.pilots):
                c = (c + Z[:, s, p] * np.conj(v)).astype(np.complex64)
            c = (c * np.float32(f.pol(s))).astype(np.complex64)
            mag = np.abs(c).astype(np.float32)
            ok = np.isfinite(mag) & (mag > 0)
            r = np.where(ok, c / np.where(ok, mag, np.float32(1)), np.complex64(1)).astype(np.complex64)
            out[:, s, :] = (out[:, s, :] * np.conj(r)[:, None]).astype(np.complex64)
    return out.reshape(Y.shape[0], -1)

# ---------------------------------------------------------------- inputs


def data_values(f, n_frames, seed=0):
    """Unit-power complex Gaussian data-carrier values, complex64 (n_frames, data_syms)."""
    rng = np.random.default_rng(1000 + seed + f.n_fft + f.n_cp)
    z = (rng.standard_normal((n_frames, f.data_syms)) + 1j * rng.standard_normal((n_frames, f.data_syms))) / np.sqrt(2)
    return z.astype(np.complex64)


def samples(f, n_frames, seed=0):
    """Unit-power complex Gaussian received samples, complex64 (n_frames, frame_samples): the T = 0 demodulator's input."""
    rng = np.random.default_rng(2000 + seed + f.n_fft + f.n_cp)
    z = (rng.standard_normal((n_frames, f.frame_samples)) + 1j * rng.standard_normal((n_frames, f.frame_samples))) / np.sqrt(2)
    return z.astype(np.complex64)


# The channel of checks 3 to 5: three taps, |H_k| >= 1 - 0.4 - 0.2 = 0.4 on every bin of every N by the triangle inequality.
H_TAPS = np.array([1.0, 0.4 * np.exp(0.7j), 0.2 * np.exp(-1.9j)])
H_FLOOR = 0.4


def frame_rotation(i):
    return np.exp(1j * (0.9 + 2.1 * i))


def symbol_thetas(f):
    """A different rotation |theta_s| <= 1 rad for every symbol of a frame, training symbols included (theirs is 0: the
    estimate is the channel's; the data symbols then carry theta_s on top of it)."""
    th = np.zeros(f.n_train + f.n_syms)
    th[f.n_train:] = np.linspace(-1.0, 1.0, f.n_syms) if f.n_syms > 1 else 0.7
    return th


def through_channel(f, tx, thetas=None):
    """Every frame convolved with H_TAPS (the tail beyond the frame is dropped, the start sees silence), rotated by
    frame_rotation(frame), and with `thetas` every symbol s rotated by e^{i theta_s} on top.  complex64."""
    tx = np.asarray(tx, np.complex128)
    rx = np.stack([np.convolve(fr, H_TAPS)[: fr.size] * frame_rotation(i) for i, fr in enumerate(tx)])
    if thetas is not None:
        rx = (rx.reshape(tx.shape[0], -1, f.sym_len) * np.exp(1j * np.asarray(thetas))[None, :, None]).reshape(tx.shape)
    return rx.astype(np.complex64)


def channel_case(name, n_frames, cpe=False, rotate=False):
    """(format, transmitted data values, received samples) of checks 3 (cpe, rotate = False) and 4."""
    f = FORMATS[name].but(cpe=cpe)
    z = data_values(f, n_frames)
    return f, z, through_channel(f, ref_mod(f, z), symbol_thetas(f) if rotate else None)


def symbol_errors(got, want, per_symbol):
    """||got - want||_2 / ||want||_2 per (frame, symbol) of `per_symbol` values each; float64 (n_frames, symbols)."""
    w = np.asarray(want, np.complex128)
    w = w.reshape(w.shape[0], -1, per_symbol)
    g = np.asarray(got, np.complex128).reshape(w.shape)
    return np.linalg.norm(g - w, axis=2) / np.linalg.norm(w, axis=2)


def worst(err):
    """(value, frame, symbol) of the largest entry, for a message that names it."""
    i = np.unravel_index(int(np.argmax(err)), err.shape)
    return float(err[i]), int(i[0]), int(i[1])


# The project's f32 transform bound (tests/test_gpu_fft_lengths.py): checks 1 and 2
FFT_BOUND = 1e-5
# Checks 3 and 4: four times the worst per-symbol distance of model_demod from ref_demod over CHANNEL_FORMATS x FRAME_COUNTS, with
# and without the pilot phase correction (tests/test_ofdm_ref.py measures it and holds this constant to it).  Measured worst:
# 2.65e-7 (n64_11a, 5 frames, correction on, symbols rotated).  The factor covers the kernels' different summation order; nothing here comes from a kernel.
CHANNEL_MODEL_WORST = 2.66e-7
CHANNEL_BOUND = 4 * CHANNEL_MODEL_WORST

# ---------------------------------------------------------------- the link of check 5 (16-QAM)
LINK_FORMAT = "n64_11a"
LINK_FRAMES = 5

# ---------------------------------------------------------------- the block rule (the capped-grid cases are tests/grid_cases.py's)
def block_rule(n_fft, per_frame, n_frames, max_grid):
    """ofdm.hip's ofdm_block: (symbols per block, blocks per frame)."""
    rnd = 4096 // n_fft
    rounds = -(-per_frame // rnd)
    want = -(-max_grid // n_frames) if 0 < n_frames < max_grid else 1
    want = min(want, rounds)
    blk = -(-rounds // want) * rnd
    return blk, -(-per_frame // blk)
