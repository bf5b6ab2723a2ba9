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
