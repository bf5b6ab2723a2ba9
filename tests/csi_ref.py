"""The definitions of the OFDM demodulator's channel-state record and of the weighted soft demapper (include/comms_hip.h,
"Channel state" and "Weighted LLRs") in numpy, an f32 model of the kernel's channel-state arithmetic, and the cases, weights and
the coded link that tests/test_csi_ref.py (no GPU) and tests/test_gpu_csi.py share.  Built on tests/ofdm_ref.py and
tests/symmap_ref.py, which stay as they are; nothing here touches the library."""
import functools

import numpy as np

import ofdm_ref as r
import symmap_ref as sr

f32 = np.float32

# ---------------------------------------------------------------- the channel-state record


def ref_csi(f, rx):
    """g[frame, d] = |H_k(d)|^2, H_k = (1 / T) sum_t Y_{t,k} / train[k], data carriers in increasing bin order: float64
    (n_frames, D), from complex128 spectra."""
    Y = r.ref_spectra(f, rx)[:, : f.n_train, :]
    H = Y.sum(axis=1) / f.n_train / f.train.astype(np.complex128)
    return np.abs(H[:, f.data_bins]) ** 2


def model_csi(f, rx):
    """ref_csi with the kernel's arithmetic in f32: ofdm_ref.fft_f32, the training sum in symbol order, den = |sum|^2, and the
    division by tt2_k = |T train[k]|^2, formed in f64 from the f32-rounded T train[k] and rounded once."""
    y = np.asarray(rx, np.complex64).reshape(-1, f.n_train + f.n_syms, f.sym_len)[:, : f.n_train, f.n_cp:]
    Y = r.fft_f32(y, -1)
    acc = np.zeros_like(Y[:, 0, :])
    for t in range(f.n_train):
        acc = (acc + Y[:, t, :]).astype(np.complex64)
    with np.errstate(all="ignore"):
        den = ((acc.real * acc.real).astype(f32) + (acc.imag * acc.imag).astype(f32)).astype(f32)
        tt = (np.float64(f.n_train) * f.train.astype(np.complex128)).astype(np.complex64)
        tt2 = (tt.real.astype(np.float64) ** 2 + tt.imag.astype(np.float64) ** 2).astype(f32)
        return (den / tt2).astype(f32)[:, f.data_bins]


CSI_MUTANTS = ("no_train", "no_T", "by_bin")


def mutant_csi(f, rx, kind):
    """The wrong records a kernel could write: no_train leaves |train[k]|^2 out of the divisor, no_T leaves T^2 out of it (the
    definition itself at T = 1), by_bin writes |H_k|^2 of bin d where data carrier d's belongs."""
    Y = r.ref_spectra(f, rx)[:, : f.n_train, :].sum(axis=1)
    tr = f.train.astype(np.complex128)
    if kind == "no_train":
        return np.abs(Y[:, f.data_bins] / f.n_train) ** 2
    if kind == "no_T":
        return np.abs(Y[:, f.data_bins] / tr[f.data_bins]) ** 2
    if kind == "by_bin":
        return np.abs(Y[:, : f.D] / f.n_train / tr[: f.D]) ** 2
    raise ValueError(kind)


def csi_errors(got, want):
    """||got - want||_2 / ||want||_2 per frame."""
    w = np.asarray(want, np.float64)
    return np.linalg.norm(np.asarray(got, np.float64) - w, axis=1) / np.linalg.norm(w, axis=1)


# ---------------------------------------------------------------- the cases
# ofdm_ref's formats have unit-modulus training values, and channel_case() gives both training symbols of a frame the same
# samples: no such case sees a missing |train[k]|^2, a missing 1 / T^2 or a record indexed by bin.  The scaled cases do:
# training values of amplitude 0.5 ... 2 per bin, T = 1, 3 and ROUND + 1 symbols that all differ (ofdm_ref.training_case's
# gains and noise), at N = 64 and N = 1024.
T_FORMATS = tuple("%s_t%d" % (base, t) for base in ("n64_11a", "n1024_cp72")
                  for t in (1, 3, r.round_of(r.FORMATS[base].n_fft) + 1))


def scaled_format(name):
    f = r.TRAINING_FORMATS[name]
    amp = np.random.default_rng(4000 + f.n_fft + f.n_train).uniform(0.5, 2.0, f.n_fft)
    return f.but(train=(f.train.astype(np.complex128) * amp).astype(np.complex64))


def scaled_case(name, n_frames, cpe=False):
    """ofdm_ref.training_case(name, n_frames, cpe, rotate=cpe) on scaled_format(name): (format, received samples)."""
    f = scaled_format(name).but(cpe=cpe)
    z = r.data_values(f, n_frames)
    rx = r.through_channel(f, r.ref_mod(f, z), r.symbol_thetas(f) if cpe else None).astype(np.complex128)
    tr = rx.reshape(n_frames, -1, f.sym_len)[:, : f.n_train, :]     # (a view)
    rms = np.sqrt(np.mean(np.abs(tr) ** 2))
    rng = np.random.default_rng(3000 + f.n_fft + f.n_cp + f.n_train)
    noise = (rng.standard_normal(tr.shape) + 1j * rng.standard_normal(tr.shape)) / np.sqrt(2)
    tr[...] = tr * r.training_gains(f.n_train)[None, :, None] + r.TRAINING_NOISE * rms * noise
    return f, rx.astype(np.complex64)


def csi_cases():
    """[(kind, name, cpe)]: ofdm_ref.CHANNEL_FORMATS behind through_channel, the T = 1, 3, ROUND + 1 cases as they are and with
    scaled training values; each without the pilot phase correction and, where the format has pilots, with it (symbols rotated)."""
    out = []
    for kind, names in (("channel", r.CHANNEL_FORMATS), ("training", T_FORMATS), ("scaled", T_FORMATS)):
        for name in names:
            f = r.FORMATS[name] if kind == "channel" else r.TRAINING_FORMATS[name]
            out += [(kind, name, False)] + ([(kind, name, True)] if f.pilot_bins.size else [])
    return out


@functools.lru_cache(maxsize=None)
def csi_case(kind, name, cpe, n_frames):
    """(format, received samples, ref_csi of them), computed once and shared read-only."""
    if kind == "channel":
        f, _, rx = r.channel_case(name, n_frames, cpe, cpe)
    elif kind == "training":
        f, _, rx = r.training_case(name, n_frames, cpe, cpe)
    else:
        f, rx = scaled_case(name, n_frames, cpe)
    want = ref_csi(f, rx)
    rx.setflags(write=False)
    want.setflags(write=False)
    return f, rx, want


# Four times the worst per-frame distance of model_csi from ref_csi over csi_cases() x ofdm_ref.FRAME_COUNTS
# (tests/test_csi_ref.py measures it and holds this constant to it).  The factor covers the kernel's different summation order;
# nothing here comes from a kernel.  g is a squared magnitude: about twice the transform's relative error.
CSI_MODEL_WORST = 2.63e-7
CSI_BOUND = 4 * CSI_MODEL_WORST
CSI_SENSITIVITY = 10.0     # every mutant is at least this many bounds off in every scaled case (no_T: in those with T > 1)

# ---------------------------------------------------------------- the weighted demapper


def ref_weighted_llr(z, weights, table, F, scale=1.0):
    """z (frames * F,) complex64, weights (frames, P) f32 -> (frames, F m) float32: L_b = fl(c fl(D1_b - D0_b)), c = fl(s w),
    w = weights[frame, j mod P]; every LLR of a symbol whose weight is not finite and > 0 is +0.0.  The distances and minima
    are symmap_ref's brute force."""
    c = np.asarray(table, np.complex64)
    m = c.size.bit_length() - 1
    w = np.asarray(weights, f32)
    frames, P = w.shape
    wj = w[:, np.arange(F) % P].ravel()
    diff = sr.ref_llr(z, c, 1.0)                                     # fl(1 * fl(D1 - D0)) = fl(D1 - D0)
    with np.errstate(all="ignore"):
        cw = (f32(scale) * wj).astype(f32)
        out = (cw[:, None] * diff).astype(f32)
        ok = np.isfinite(wj) & (wj > 0)
    out[~ok, :] = f32(0.0)
    return out.reshape(frames, F * m)


WEIGHT_SHAPES = ((1, 1), (63, 1), (65, 7), (100, 48), (129, 129))    # (F, P)
WEIGHT_FRAMES = (1, 5)
WEIGHT_TABLES = ("bpsk", "qpsk", "8psk", "16qam", "64qam", "256qam")  # m = 1, 2, 3, 4, 6, 8: QAM tables and 8-PSK
PLANTED = np.array([0.0, -1.0, np.nan, np.inf, 1e-40, np.finfo(np.float32).max, -np.inf, -0.0], f32)


def weights_for(F, P, n_frames, seed):
    """(n_frames, P) float32 drawn log-uniformly from [0.01, 100], with PLANTED written at the weights of the symbols around
    every frame seam (flat symbol indices f F - 1, f F) and wave seam (64 i - 1, 64 i), as far as they exist."""
    rng = np.random.default_rng(seed)
    w = np.exp(rng.uniform(np.log(0.01), np.log(100.0), (n_frames, P))).astype(f32)
    spots = sorted({s for f in range(n_frames + 1) for s in (f * F - 1, f * F)} | {s for i in range(1, n_frames * F // 64 + 1) for s in (64 * i - 1, 64 * i)})
    k = 0
    for s in spots:
        if 0 <= s < n_frames * F:
            w[s // F, (s % F) % P] = PLANTED[k % PLANTED.size]
            k += 1
    return w


# ---------------------------------------------------------------- the coded link
# K = 7 rate-1/2 terminated code -> block interleaver -> QPSK or 16-QAM -> OFDM at n64_11a, through the two-tap channel
# [1, 0.95 e^{i phi}] whose null sits on data carrier LINK_NULL_BIN, with seeded noise on the received samples.  The receiver
# decodes twice: LLRs weighted by the channel state, and unweighted.
LINK_FRAMES = 16
LINK_FORMAT = "n64_11a"
LINK_NULL_BIN = 10
LINK_TAPS = np.array([1.0, 0.95 * np.exp(1j * (np.pi + 2 * np.pi * LINK_NULL_BIN / 64))])
LINK_COLS = 12                                   # interleaver columns: neighbouring coded bits land 12 carriers apart or more
# m -> (noise per component of a received sample, seed): chosen on the CPU with the references (tests/test_csi_ref.py
# asserts the two conditions of the link for them)
LINK_NOISE = {2: (0.4, 12), 4: (0.12, 12)}
LINK_MARGIN = 1.25


def link_format(m):
    import viterbi_ref as vr

    f = r.FORMATS[LINK_FORMAT]
    E = m * f.data_syms                            # transmitted bits = coded bits: nothing is punctured
    T = E // 2 - 6
    assert 2 * vr.n_steps(T, 7, True) == E
    return dict(f=f, m=m, T=T, N=E, E=E, F=f.data_syms, table=sr.qam_table(m))


def link_transmit(m):
    """(payload bits (frames, T), transmitted bits (frames, E), frames of samples complex128) on the references."""
    import ratematch_ref as rr
    import viterbi_ref as vr

    L = link_format(m)
    payload = np.random.default_rng(500 + m).integers(0, 2, (LINK_FRAMES, L["T"]), dtype=np.uint8)
    src, _ = rr.build_map(L["N"], None, LINK_COLS)
    sent = rr.ref_tx(vr.ref_encode(payload, 7, vr.GENS[(7, 2)]), src)
    sym = sr.ref_map(sent, m, L["table"])
    return payload, sent, r.ref_mod(L["f"], sym)


def link_channel(m, tx, amplitude=1.0):
    """Every frame through LINK_TAPS (the tail beyond the frame dropped), plus the seeded noise times `amplitude`: complex64."""
    sigma, seed = LINK_NOISE[m]
    tx = np.asarray(tx, np.complex128)
    rx = np.stack([np.convolve(fr, LINK_TAPS)[: fr.size] for fr in tx])
    rng = np.random.default_rng(seed)
    noise = rng.standard_normal(rx.shape) + 1j * rng.standard_normal(rx.shape)
    return (rx + amplitude * sigma * noise).astype(np.complex64)


def link_scales(m):
    """(llr_scale, the unweighted run's llr_scale, qscale).  A data carrier's value is Y_k / H_k with H_k the estimate in the
    spectrum's units (g = |H_k|^2, about N |h_k|^2 at tx_scale 1 / sqrt(N)), and Y_k carries the noise of N samples: sigma_Y^2 =
    N sigma^2 per component, llr_scale = 1 / (2 sigma_Y^2).  The unweighted run takes the mean weight of the true channel into its
    scale.  qscale keeps the strongest carrier (|h| = 1.95) off the clamp at the table's outermost decision distance."""
    sigma, _ = LINK_NOISE[m]
    n = r.FORMATS[LINK_FORMAT].n_fft
    s = 1.0 / (2.0 * n * sigma ** 2)
    g_mean, g_max = n * (1 + 0.95 ** 2), n * 1.95 ** 2
    reach = 4.0 * (1 if m == 2 else 3)              # |D1 - D0| of a point one unit beyond the outermost level
    return s, s * g_mean, 127.0 / (s * g_max * reach)


def link_receive(m, rx, weighted):
    """The receive side on the references: (decoded bits (frames, T), LLR records f32, channel state)."""
    import ratematch_ref as rr
    import viterbi_ref as vr

    L = link_format(m)
    s, s_flat, qscale = link_scales(m)
    with np.errstate(all="ignore"):
        z = r.ref_demod(L["f"], rx).astype(np.complex64)
        g = ref_csi(L["f"], rx).astype(f32)
    if weighted:
        llr = ref_weighted_llr(z.ravel(), g, L["table"], L["F"], s)
    else:
        llr = sr.ref_llr_records(z.ravel(), L["table"], L["F"], s_flat)
    src, _ = rr.build_map(L["N"], None, LINK_COLS)
    words = rr.ref_rx(llr.view(np.uint32), src, L["N"])
    decoded, _ = vr.ref_decode(vr.ref_quantise(words.view(f32), qscale), 7, vr.GENS[(7, 2)], L["T"])
    return decoded, llr, g


def frames_wrong(decoded, payload):
    return int(np.count_nonzero((np.asarray(decoded)[:, : payload.shape[1]] != payload).any(axis=1)))
