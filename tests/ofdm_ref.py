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


def round_of(n_fft):
    """Symbols ofdm_demod_kernel transforms at once: four waves of 1024 / N."""
    return 4096 // n_fft


def _training_formats():
    """T = 1, 3, ROUND - 1, ROUND, ROUND + 1, 2 ROUND + 1 at every N (without duplicates), on the smallest S of that N: one slot,
    a few, a round less one, a full round, a second round of one slot and a third.  n256_cp0 (prefix 0, no pilots) at ROUND + 1."""
    out = {}
    for base, s in (("n64_11a", 3), ("n128_cp9", 3), ("n256_cpN", 3), ("n512_cp36", 9), ("n1024_cp72", 2)):
        rnd = round_of(FORMATS[base].n_fft)
        for t in sorted({1, 3, rnd - 1, rnd, rnd + 1, 2 * rnd + 1}):
            out["%s_t%d" % (base, t)] = FORMATS[base].but(n_syms=s, n_train=t)
    out["n256_cp0_t17"] = FORMATS["n256_cp0"].but(n_syms=3, n_train=17)
    return out


# The training sum (tests/test_ofdm_ref.py, "sensitivity"): FORMATS has T = 2 everywhere and through_channel() gives both
# training symbols of a frame the same samples, so no case above can tell which symbols the demodulator adds.  These can:
# training_case() makes every received training symbol of a frame different from every other.
TRAINING_FORMATS = _training_formats()
TRAINING_CPE_FORMATS = tuple(k for k, f in TRAINING_FORMATS.items() if f.n_fft >= 512)   # also with the correction on, symbols rotated
LONG_TRAINING_FORMATS = tuple(k for k, f in TRAINING_FORMATS.items() if f.n_train >= round_of(f.n_fft))   # the modulator's

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


def training_gains(n_train):
    """g_t = 1 + 0.3 e^{2.4 i t}: 0.7 <= |g_t| <= 1.3 and no two of a frame alike (2.4 t is no multiple of 2 pi)."""
    return 1.0 + 0.3 * np.exp(2.4j * np.arange(n_train))


TRAINING_NOISE = 10.0 ** (-30.0 / 20.0)   # the training symbols' noise, relative to their rms


def training_case(name, n_frames, cpe=False, rotate=False, seed=0):
    """(format, transmitted data values, received samples) behind the channel of channel_case, with training symbol t of every
    frame multiplied by training_gains()[t] and seeded complex noise 30 dB below the training symbols added to them: the
    received training symbols of a frame all differ.  Data symbols keep gain 1 and no noise; `seed` gives other frames."""
    f = TRAINING_FORMATS[name].but(cpe=cpe)
    z = data_values(f, n_frames, seed)
    rx = through_channel(f, ref_mod(f, z), symbol_thetas(f) if rotate else None).astype(np.complex128)
    tr = rx.reshape(n_frames, -1, f.sym_len)[:, : f.n_train, :]     # (a view: rx is contiguous)
    rms = np.sqrt(np.mean(np.abs(tr) ** 2))
    rng = np.random.default_rng(3000 + seed + f.n_fft + f.n_cp + f.n_train)
    noise = (rng.standard_normal(tr.shape) + 1j * rng.standard_normal(tr.shape)) / np.sqrt(2)
    tr[...] = tr * training_gains(f.n_train)[None, :, None] + TRAINING_NOISE * rms * noise
    return f, z, rx.astype(np.complex64)


def training_cases():
    """[(name, cpe, rotate)] of the table: every format plain, N = 512 and 1024 also corrected and rotated as check 4 is."""
    return [(k, False, False) for k in TRAINING_FORMATS] + [(k, True, True) for k in TRAINING_CPE_FORMATS]


def training_mutants(f):
    """[(label, slot, source)]: the wrong training sums a kernel could make.  Slot t (a) left out, (b) read from symbol t + 1,
    (c) read from symbol t + 1024 / N, the same slot of the next wave's exchange buffer; both modulo T.  T = 1 has (a) alone."""
    spw, T = 1024 // f.n_fft, f.n_train
    out = [("omit", t, None) for t in range(T)]
    out += [("next", t, (t + 1) % T) for t in range(T) if T > 1]
    out += [("wave", t, (t + spw) % T) for t in range(T) if T > 1]
    return out


def mutant_samples(f, rx, slot, source):
    """`rx` with training symbol `slot` of every frame replaced by symbol `source` (None: by zeros, which leaves it out of the
    sum while the sum is still divided by T): the definition of a mutant is ref_demod of these samples."""
    out = np.array(rx, np.complex64).reshape(rx.shape[0], -1, f.sym_len)
    out[:, slot, :] = 0 if source is None else out[:, source, :]
    return out.reshape(rx.shape)


# Degenerate frames (the contract's "left as it is when |c| is 0 or not finite", and a training sum of zero): frame
# DEGENERATE_FRAME of DEGENERATE_FRAMES is made degenerate, data symbol DEGENERATE_SYMBOL where it is one symbol's.
DEGENERATE_FORMAT, DEGENERATE_FRAMES, DEGENERATE_FRAME, DEGENERATE_SYMBOL = "n64_11a_t3", 5, 2, 1
DEGENERATE_KINDS = ("zero_symbol", "inf_sample", "zero_training")


def degenerate_case(kind):
    """(format, received samples) of training_case(DEGENERATE_FORMAT, correction on, symbols rotated) with one frame changed:
    zero_symbol    every sample of one data symbol is 0: the pilot sum c is 0, the symbol stays unrotated, its values are 0;
    inf_sample     one sample of one data symbol is +Inf: every bin of it, and c, is NaN or infinite, the rotation is skipped;
    zero_training  every training sample is 0: the sum is 0 on every bin, Y / 0 is NaN or infinite in that frame."""
    f, _, rx = training_case(DEGENERATE_FORMAT, DEGENERATE_FRAMES, cpe=True, rotate=True)
    sym = rx.reshape(DEGENERATE_FRAMES, -1, f.sym_len)     # (a view)
    if kind == "zero_symbol":
        sym[DEGENERATE_FRAME, f.n_train + DEGENERATE_SYMBOL, :] = 0
    elif kind == "inf_sample":
        sym[DEGENERATE_FRAME, f.n_train + DEGENERATE_SYMBOL, f.n_cp + 5] = np.inf
    elif kind == "zero_training":
        sym[DEGENERATE_FRAME, : f.n_train, :] = 0
    else:
        raise ValueError(kind)
    return f, rx


def nonfinite(z):
    """Per complex value: a part is NaN or infinite.  Whether a part is NaN or infinite depends on the order of the transform's
    additions (Inf - Inf against Inf + x), so the definition and a kernel are compared by this mask, position by position."""
    z = np.asarray(z)
    return ~(np.isfinite(z.real) & np.isfinite(z.imag))


def check_degenerate(f, kind, got, want, bound):
    """The comparison of a degenerate call with ref_demod's `want`, shared by the CPU and the GPU test: NaN or infinite values at
    the same positions, the degenerate symbol or frame as the contract says, and everything else within `bound` per symbol."""
    n = DEGENERATE_FRAMES
    g = np.asarray(got).reshape(n, f.n_syms, f.D)
    w = np.asarray(want).reshape(n, f.n_syms, f.D)
    bad = np.zeros((n, f.n_syms), bool)
    if kind == "zero_training":
        bad[DEGENERATE_FRAME, :] = True
    else:
        bad[DEGENERATE_FRAME, DEGENERATE_SYMBOL] = True
    assert np.array_equal(nonfinite(g), nonfinite(w)), kind
    if kind == "zero_symbol":
        assert not nonfinite(g).any() and not g[bad].any() and not w[bad].any(), kind      # exactly zero, unrotated
    else:
        assert np.array_equal(nonfinite(g), np.broadcast_to(bad[:, :, None], g.shape)), kind
    err = symbol_errors(g[~bad].reshape(1, -1), w[~bad].reshape(1, -1), f.D)
    assert err.max() <= bound, (kind, worst(err))
    return float(err.max())


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
# The training-sum cases: the same measurement over training_cases() x FRAME_COUNTS (tests/test_ofdm_ref.py holds it likewise).
# Measured worst: 2.706e-7 (n1024_cp72_t4, 5 frames, correction on, symbols rotated); n64_11a_t129, 129 f32 additions into
# the sum, gives 2.69e-7: the sum's rounding errors average out in H, and the transform's error dominates at every T.
TRAINING_MODEL_WORST = 2.71e-7
TRAINING_BOUND = 4 * TRAINING_MODEL_WORST
# Every mutant of training_mutants() moves ref_demod's output by at least this many bounds in some symbol (the issue's factor;
# tests/test_ofdm_ref.py prints what each case achieves)
TRAINING_SENSITIVITY = 10.0

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
