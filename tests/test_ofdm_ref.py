"""tests/ofdm_ref.py held to the contract of include/comms_hip.h ("OFDM modulator and demodulator") without a GPU: the
definition against a direct DFT, the properties the contract states, the f32 model's distance from the definition (which
fixes the bound the GPU tests use) and the rules of the case tables."""
import numpy as np
import pytest

import grid_cases as gc
import ofdm_ref as r


def test_reference_equals_direct_dft_at_64():
    f = r.FORMATS["n64_11a"]
    z = r.data_values(f, 2)
    X = r.freq_values(f, z)
    x = r.dft_direct(X, +1) * float(f.tx_scale)
    want = np.concatenate([x[..., 64 - f.n_cp:], x], axis=-1).reshape(2, -1)
    assert np.abs(r.ref_mod(f, z) - want).max() <= 1e-12
    rx = r.samples(f.but(n_train=0), 2)
    Y = r.dft_direct(rx.reshape(2, -1, f.sym_len)[..., f.n_cp:], -1)
    assert np.abs(r.ref_spectra(f.but(n_train=0), rx) - Y).max() <= 1e-11
    assert np.abs(r.fft_f32(rx.reshape(2, -1, f.sym_len)[..., f.n_cp:], -1) - Y).max() <= 1e-4


@pytest.mark.parametrize("name,cpe", [(n, c) for n in sorted(r.FORMATS) for c in (False, True) if not c or r.FORMATS[n].pilot_bins.size])
def test_mod_demod_identity(name, cpe):
    f = r.FORMATS[name].but(cpe=cpe)
    z = r.data_values(f, 3)
    tx = r.ref_mod(f, z)
    assert tx.shape == (3, f.frame_samples) and z.shape == (3, f.data_syms)
    assert np.abs(r.ref_demod(f, tx) - z).max() <= 1e-12


@pytest.mark.parametrize("name", sorted(r.FORMATS))
def test_prefix_is_the_symbols_tail(name):
    f = r.FORMATS[name]
    sym = r.ref_mod(f, r.data_values(f, 2)).reshape(2, -1, f.sym_len)
    assert np.array_equal(sym[..., : f.n_cp], sym[..., f.sym_len - f.n_cp:])


def test_nulls_pilots_and_polarity_land_where_the_contract_says():
    f = r.FORMATS["n64_11a"]
    assert f.D == 48 and f.pilot_bins.tolist() == [7, 21, 43, 57] and f.kind[0] == r.NULL and not f.kind[27:38].any()
    z = r.data_values(f, 2)
    X = r.ref_spectra(f, r.ref_mod(f, z)) / (64 * float(f.tx_scale))
    assert np.abs(X[:, f.n_train:, f.kind == r.NULL]).max() <= 1e-12                     # null bins stay out of data symbols
    assert np.abs(X[:, : f.n_train, :] - f.train).max() <= 1e-12                          # a training symbol is train[k] on every bin
    assert np.abs(X[:, f.n_train:, f.data_bins].reshape(2, -1) - z).max() <= 1e-12        # increasing bin order, symbol-major
    for s in range(f.n_syms):
        assert np.abs(X[:, f.n_train + s, f.pilot_bins] - f.pilots * r.POLARITY[s % 5]).max() <= 1e-12
    g = f.but(polarity=None)
    X = r.ref_spectra(g, r.ref_mod(g, z)) / (64 * float(g.tx_scale))
    assert np.abs(X[:, g.n_train + 1, g.pilot_bins] - g.pilots).max() <= 1e-12            # no polarity: 1


def test_channel_floor_and_ls_estimate():
    for n in (64, 128, 256, 512, 1024):
        assert np.abs(np.fft.fft(r.H_TAPS, n)).min() >= r.H_FLOOR
    f, z, rx = r.channel_case("n64_11a", 3)
    Y = r.ref_spectra(f, rx)
    used = f.kind != r.NULL
    H = Y[:, : f.n_train, used].sum(axis=1) / f.n_train / f.train[used] / (64 * float(f.tx_scale))
    for i in range(3):   # the estimate is the channel times the frame's rotation (up to the complex64 rounding of rx)
        assert np.abs(H[i] - np.fft.fft(r.H_TAPS, 64)[used] * r.frame_rotation(i)).max() <= 1e-6
    assert r.symbol_errors(r.ref_demod(f, rx), z, f.D).max() <= 1e-6


def test_cpe_undoes_a_per_symbol_rotation():
    f, z, rx = r.channel_case("n64_11a", 2, cpe=True, rotate=True)
    th = r.symbol_thetas(f)
    assert np.abs(th).max() <= 1.0 and len(set(th[f.n_train:])) == f.n_syms and not th[: f.n_train].any()
    assert r.symbol_errors(r.ref_demod(f, rx), z, f.D).max() <= 1e-6
    off = r.ref_demod(f.but(cpe=False), rx).reshape(2, f.n_syms, f.D)       # flag off: the rotation stays
    want = z.reshape(2, f.n_syms, f.D) * np.exp(1j * th[f.n_train:])[None, :, None]
    assert np.abs(off - want).max() <= 1e-5 and np.abs(off - z.reshape(off.shape)).max() > 0.1


def test_model_distance_fixes_the_channel_bound():
    """The bound of the GPU tests' checks 3 and 4 is four times the f32 model's worst distance from the definition on those
    tests' own inputs: measured here, compared with the constant ofdm_ref.py stores."""
    seen = 0.0
    for cpe, rotate in ((False, False), (True, True), (True, False)):
        for name in (r.CPE_FORMATS if cpe else r.CHANNEL_FORMATS):
            for n_frames in r.FRAME_COUNTS:
                f, _, rx = r.channel_case(name, n_frames, cpe, rotate)
                err, frame, sym = r.worst(r.symbol_errors(r.model_demod(f, rx), r.ref_demod(f, rx), f.D))
                print("%-12s frames %d cpe %d rotate %d: model %.3e (frame %d symbol %d)" % (name, n_frames, cpe, rotate, err, frame, sym))
                seen = max(seen, err)
    assert 0.5 * r.CHANNEL_MODEL_WORST <= seen <= r.CHANNEL_MODEL_WORST, seen
    assert r.CHANNEL_BOUND == 4 * r.CHANNEL_MODEL_WORST <= r.FFT_BOUND


def test_training_table_covers_the_issue():
    fs = r.TRAINING_FORMATS
    for n, base, s in ((64, "n64_11a", 3), (128, "n128_cp9", 3), (256, "n256_cpN", 3), (512, "n512_cp36", 9), (1024, "n1024_cp72", 2)):
        rnd = r.round_of(n)
        assert rnd == 4 * (1024 // n)
        want = sorted({1, 3, rnd - 1, rnd, rnd + 1, 2 * rnd + 1})
        assert [f.n_train for k, f in fs.items() if k.startswith(base + "_t")] == want
        for t in want:
            f = fs["%s_t%d" % (base, t)]
            assert (f.n_fft, f.n_cp, f.n_syms, f.D) == (n, r.FORMATS[base].n_cp, s, r.FORMATS[base].D)
    assert max(f.n_train + f.n_syms for f in fs.values()) == 132 and fs["n64_11a_t129"].sym_len == 80      # the largest frame
    assert {f.n_cp for f in fs.values()} >= {9, 0, 256}                                                      # odd, none, N
    assert fs["n256_cp0_t17"].n_cp == 0 and not fs["n256_cp0_t17"].pilot_bins.size
    assert set(r.TRAINING_CPE_FORMATS) == {k for k, f in fs.items() if f.n_fft in (512, 1024)} and len(r.TRAINING_CPE_FORMATS) == 11
    assert all(fs[k].pilot_bins.size for k in r.TRAINING_CPE_FORMATS)
    assert len(r.training_cases()) == len(fs) + 11 == 41
    # the modulator's: T of at least a round, so that a block can hold training symbols only
    assert set(r.LONG_TRAINING_FORMATS) == {k for k, f in fs.items() if f.n_train >= r.round_of(f.n_fft)} and len(r.LONG_TRAINING_FORMATS) == 16
    assert np.abs(r.training_gains(129)).min() >= 0.7
    g = r.training_gains(129)
    assert np.abs(g[:, None] - g[None, :])[~np.eye(129, dtype=bool)].min() > 1e-3


def test_received_training_symbols_differ_and_the_definition_holds():
    """training_case() changes the channel the training symbols see and nothing else: the data symbols are channel_case's,
    every pair of training spectra of a frame differs, and H stays the mean of the received training spectra over train."""
    for name, cpe, rotate in r.training_cases():
        f, z, rx = r.training_case(name, 2, cpe, rotate)
        plain = r.through_channel(f, r.ref_mod(f, z), r.symbol_thetas(f) if rotate else None)
        sym, base = rx.reshape(2, -1, f.sym_len), plain.reshape(2, -1, f.sym_len)
        assert sym[:, f.n_train:].tobytes() == base[:, f.n_train:].tobytes()
        Y = r.ref_spectra(f, rx)[:, : f.n_train]
        scale = np.linalg.norm(Y, axis=2).min()
        for a in range(f.n_train):
            for b in range(a):
                assert np.linalg.norm(Y[:, a] - Y[:, b], axis=1).min() >= 0.01 * scale, (name, a, b)
        noise = sym[:, : f.n_train] - base[:, : f.n_train] * r.training_gains(f.n_train)[None, :, None]
        ratio = np.sqrt(np.mean(np.abs(noise) ** 2) / np.mean(np.abs(base[:, : f.n_train].astype(np.complex128)) ** 2))
        assert 0.8 * r.TRAINING_NOISE <= ratio <= 1.25 * r.TRAINING_NOISE, (name, ratio)      # about 30 dB below them
        other = r.training_case(name, 2, cpe, rotate, seed=1)[2]
        assert other.shape == rx.shape and (other != rx).any(axis=1).all()                     # `seed`: other frames


def _model_worst(cases, case_of):
    seen, where = 0.0, None
    for name, cpe, rotate in cases:
        for n_frames in r.FRAME_COUNTS:
            f, _, rx = case_of(name, n_frames, cpe, rotate)
            err, frame, sym = r.worst(r.symbol_errors(r.model_demod(f, rx), r.ref_demod(f, rx), f.D))
            print("%-16s frames %d cpe %d rotate %d: model %.3e (frame %d symbol %d)" % (name, n_frames, cpe, rotate, err, frame, sym))
            if err > seen:
                seen, where = err, (name, n_frames, cpe, rotate)
    return seen, where


def test_model_distance_fixes_the_training_bound():
    """TRAINING_BOUND is measured as CHANNEL_BOUND is: four times the f32 model's worst distance from the definition over the
    training-sum cases, every frame count, the corrected and rotated runs included."""
    seen, where = _model_worst(r.training_cases(), r.training_case)
    print("worst %.4e at %s" % (seen, where))
    assert 0.5 * r.TRAINING_MODEL_WORST <= seen <= r.TRAINING_MODEL_WORST, (seen, where)
    assert r.TRAINING_BOUND == 4 * r.TRAINING_MODEL_WORST <= r.FFT_BOUND


def test_every_training_slot_shows_in_the_output():
    """The condition the training-sum cases exist for.  A demodulator that leaves slot t out of the sum, reads slot t + 1 for it,
    or reads the same slot of the next wave's buffer is, by definition, ref_demod of mutant_samples(); each of them moves some
    symbol of every case by at least TRAINING_SENSITIVITY bounds, so no such kernel passes the comparison within TRAINING_BOUND
    (the f32 model with the same mutation is within the model's distance of the mutant definition, a quarter of a bound)."""
    lowest, where = np.inf, None
    for name, cpe, rotate in r.training_cases():
        for n_frames in r.FRAME_COUNTS:
            f, _, rx = r.training_case(name, n_frames, cpe, rotate)
            want = r.ref_demod(f, rx)
            muts = r.training_mutants(f)
            assert len(muts) == (3 * f.n_train if f.n_train > 1 else 1)
            assert all(src != t for _, t, src in muts)                       # no mutant is the identity
            low = np.inf
            for label, t, src in muts:
                with np.errstate(all="ignore"):      # T = 1 with its only symbol left out divides by zero: nothing is finite
                    moved = r.symbol_errors(r.ref_demod(f, r.mutant_samples(f, rx, t, src)), want, f.D)
                assert np.isfinite(moved).all() if f.n_train > 1 else not np.isfinite(moved).any()
                moved = float(moved.max()) if f.n_train > 1 else np.inf
                low = min(low, moved)
                if moved < lowest:
                    lowest, where = moved, (name, n_frames, cpe, label, t)
                assert moved >= r.TRAINING_SENSITIVITY * r.TRAINING_BOUND, (name, n_frames, cpe, label, t, moved)
            print("%-16s frames %d cpe %d: %4d mutants, the least visible moves a symbol by %.3e = %.0f bounds" %
                  (name, n_frames, cpe, len(muts), low, low / r.TRAINING_BOUND))
    print("least %.3e = %.0f bounds at %s" % (lowest, lowest / r.TRAINING_BOUND, where))
    # and the model itself, mutated, misses the bound: one mutant of each kind in the case where they show least
    name, n_frames, cpe, _, _ = where
    f, _, rx = r.training_case(name, n_frames, cpe, cpe)
    want = r.ref_demod(f, rx)
    for label, t, src in r.training_mutants(f):
        if t == where[4]:
            assert r.symbol_errors(r.model_demod(f, r.mutant_samples(f, rx, t, src)), want, f.D).max() > r.TRAINING_BOUND, (label, t)


def test_the_two_symbol_formats_cannot_see_the_training_sum():
    """Why the cases above exist: behind through_channel() both training symbols of a T = 2 frame are the same samples, so a
    demodulator that reads one of them twice gives ref_demod's output exactly.  This also pins through_channel(): the bounds of
    checks 3 and 4 were measured on these inputs."""
    for cpe, rotate in ((False, False), (True, True)):
        for name in (r.CPE_FORMATS if cpe else r.CHANNEL_FORMATS):
            f, _, rx = r.channel_case(name, 2, cpe, rotate)
            Y = r.ref_spectra(f, rx)
            assert np.abs(Y[:, 0] - Y[:, 1]).max() == 0.0
            want = r.ref_demod(f, rx)
            for t in (0, 1):
                assert np.abs(r.ref_demod(f, r.mutant_samples(f, rx, t, 1 - t)) - want).max() == 0.0, (name, t)


@pytest.mark.parametrize("kind", r.DEGENERATE_KINDS)
def test_degenerate_frames_in_the_definition_and_the_model(kind):
    """include/comms_hip.h: a symbol whose pilot sum is 0 or not finite is left unrotated; a training sum of 0 on a used bin
    divides by zero, and that frame's values are NaN or infinite.  Either stays within its symbol or frame: here for the
    definition (against the undisturbed call) and for the f32 model (against the definition)."""
    f, rx = r.degenerate_case(kind)
    clean = r.training_case(r.DEGENERATE_FORMAT, r.DEGENERATE_FRAMES, cpe=True, rotate=True)[2]
    assert f.cpe and f.pilot_bins.size and (rx != clean).any(axis=1).tolist() == [i == r.DEGENERATE_FRAME for i in range(r.DEGENERATE_FRAMES)]
    with np.errstate(all="ignore"):
        want, model = r.ref_demod(f, rx), r.model_demod(f, rx)
    # the definition: the rest of the call is what it is without the disturbance, exactly
    w = want.reshape(r.DEGENERATE_FRAMES, f.n_syms, f.D)
    cw = r.ref_demod(f, clean).reshape(w.shape)
    others = np.arange(r.DEGENERATE_FRAMES) != r.DEGENERATE_FRAME
    assert np.array_equal(w[others], cw[others]) and np.abs(cw).min() > 0
    if kind != "zero_training":
        rest = np.arange(f.n_syms) != r.DEGENERATE_SYMBOL
        assert np.array_equal(w[r.DEGENERATE_FRAME][rest], cw[r.DEGENERATE_FRAME][rest])
    err = r.check_degenerate(f, kind, model, want, r.TRAINING_BOUND / 4)
    print("%s: model within %.3e of the definition elsewhere" % (kind, err))


def test_link_margin_at_16qam():
    """Check 5's exact bits: a decision flips only if a value moves by half the level spacing (1 at the table's scale, levels
    +-1, +-3); CHANNEL_BOUND per symbol moves a value by at most bound * ||symbol||_2, far below that."""
    f = r.FORMATS[r.LINK_FORMAT]
    worst_norm = np.sqrt(f.D * 18.0)    # every value at a corner, |3 + 3i|^2 = 18
    assert r.CHANNEL_BOUND * worst_norm < 1e-3 < 1.0
    # and the definition itself returns the transmitted points to within the same order behind the channel
    levels = np.array([-3.0, -1.0, 1.0, 3.0])
    rng = np.random.default_rng(5)
    z = (rng.choice(levels, (r.LINK_FRAMES, f.data_syms)) + 1j * rng.choice(levels, (r.LINK_FRAMES, f.data_syms))).astype(np.complex64)
    rx = r.through_channel(f, r.ref_mod(f, z))
    assert np.abs(r.ref_demod(f, rx) - z).max() < 1e-4


def test_format_table_covers_the_issue():
    fs = r.FORMATS
    assert (fs["n64_11a"].n_cp, fs["n64_11a"].n_syms, fs["n64_11a"].n_train) == (16, 3, 2) and 3 % (1024 // 64)
    assert fs["n128_cp9"].n_cp % 2 == 1
    assert fs["n256_cp0"].n_cp == 0 and fs["n256_cpN"].n_cp == 256
    assert (fs["n512_cp36"].n_fft, fs["n512_cp36"].n_cp) == (512, 36)
    assert (fs["n1024_cp72"].n_fft, fs["n1024_cp72"].n_cp, fs["n1024_cp72"].n_syms) == (1024, 72, 2)
    assert fs["n64_all"].D == 64 and fs["n64_single"].D == 1 and not fs["n64_single"].pilot_bins.size
    assert {f.n_fft for f in fs.values()} == {64, 128, 256, 512, 1024}
    assert r.FRAME_COUNTS == (1, 5)
    assert "n64_11a" in r.CHANNEL_FORMATS and "n128_cp9" in r.CPE_FORMATS and "n1024_cp72" in r.CPE_FORMATS
    for f in list(fs.values()) + list(gc.OFDM_FORMATS.values()):
        assert f.frame_samples <= 1 << 24 and f.D >= 1


def test_block_rule():
    assert r.block_rule(64, 72, 13, 1) == (128, 1) and r.block_rule(64, 72, 13, 3) == (128, 1)    # frames >= grid: one block per frame
    assert r.block_rule(64, 200, 1, 1024) == (64, 4)      # few long frames: a block per round
    assert r.block_rule(64, 200, 1, 2) == (128, 2)        # no more blocks than workgroups to feed
    assert r.block_rule(512, 9, 5, 1024) == (8, 2)
    assert r.block_rule(1024, 2, 5, 1024) == (4, 1)
