"""tests/csi_ref.py held to the contract of include/comms_hip.h ("Channel state", "Weighted LLRs") without a GPU: the f32
model's distance from the definition (which fixes the bound of tests/test_gpu_csi.py), what the scaled cases can see that
ofdm_ref's cannot, the weighted demapper's rule, and the two conditions of the coded link on the reference chain alone."""
import numpy as np
import pytest

import csi_ref as cr
import ofdm_ref as r
import symmap_ref as sr


def test_csi_is_the_channels_power_on_the_data_carriers():
    f, _, rx = r.channel_case("n64_11a", 3)
    g = cr.ref_csi(f, rx)
    amp = f.n_fft * float(f.tx_scale)
    want = np.abs(np.fft.fft(r.H_TAPS, 64)[f.data_bins] * amp) ** 2        # |frame_rotation| = 1
    assert g.shape == (3, f.D) and np.abs(g / want - 1).max() <= 1e-5
    assert f.data_bins[0] == 1 and f.D == 48                               # bin order, not bin index: bin 0 is null here


def test_model_distance_fixes_the_csi_bound():
    seen, where = 0.0, None
    for kind, name, cpe in cr.csi_cases():
        for n_frames in r.FRAME_COUNTS:
            f, rx, want = cr.csi_case(kind, name, cpe, n_frames)
            err = float(cr.csi_errors(cr.model_csi(f, rx), want).max())
            print("%-8s %-16s cpe %d frames %d: model %.3e" % (kind, name, cpe, n_frames, err))
            if err > seen:
                seen, where = err, (kind, name, cpe, n_frames)
    print("worst %.4e at %s" % (seen, where))
    assert 0.5 * cr.CSI_MODEL_WORST <= seen <= cr.CSI_MODEL_WORST, seen
    assert cr.CSI_BOUND == 4 * cr.CSI_MODEL_WORST <= r.FFT_BOUND


def test_case_table_covers_the_issue():
    cases = cr.csi_cases()
    assert {n for k, n, _ in cases if k == "channel"} == set(r.CHANNEL_FORMATS)
    assert cr.T_FORMATS == ("n64_11a_t1", "n64_11a_t3", "n64_11a_t65", "n1024_cp72_t1", "n1024_cp72_t3", "n1024_cp72_t5")
    for kind in ("training", "scaled"):
        assert [(n, c) for k, n, c in cases if k == kind] == [(n, c) for n in cr.T_FORMATS for c in (False, True)]
    for name in cr.T_FORMATS:
        f = cr.scaled_format(name)
        amp = np.abs(f.train.astype(np.complex128))
        assert 0.5 - 1e-6 <= amp.min() < 0.6 and 1.8 < amp.max() <= 2.0 + 1e-6, name
        assert not np.array_equal(f.data_bins, np.arange(f.D))


@pytest.mark.parametrize("name", cr.T_FORMATS)
def test_scaled_cases_see_what_the_unit_cases_cannot(name):
    """A record without |train[k]|^2, without 1 / T^2, or indexed by bin is at least 10 bounds off in every frame of every
    scaled case (without 1 / T^2: where T > 1; at T = 1 it is the definition); on unit training values with two equal
    training symbols the first of them is the definition itself."""
    for n_frames in r.FRAME_COUNTS:
        f, rx, want = cr.csi_case("scaled", name, False, n_frames)
        for kind in cr.CSI_MUTANTS:
            off = float(cr.csi_errors(cr.mutant_csi(f, rx, kind), want).min())
            print("%s frames %d %-8s: %.3e = %.0f bounds" % (name, n_frames, kind, off, off / cr.CSI_BOUND))
            if kind == "no_T" and f.n_train == 1:
                assert off == 0.0
            else:
                assert off >= cr.CSI_SENSITIVITY * cr.CSI_BOUND, (name, kind, off)
    f, _, rx = r.channel_case("n64_11a", 2)
    assert cr.csi_errors(cr.mutant_csi(f, rx, "no_train"), cr.ref_csi(f, rx)).max() <= 1e-6


def test_zero_training_gives_zero_csi_in_its_frame_only():
    f, rx = r.degenerate_case("zero_training")
    g, model = cr.ref_csi(f, rx), cr.model_csi(f, rx)
    bad = np.arange(r.DEGENERATE_FRAMES) == r.DEGENERATE_FRAME
    assert not g[bad].any() and not model[bad].any() and (g[~bad] > 0).all()
    assert cr.csi_errors(model[~bad], g[~bad]).max() <= cr.CSI_BOUND


@pytest.mark.parametrize("name", cr.WEIGHT_TABLES)
def test_weighted_rule(name):
    m, table, _, _ = sr.table_of(name)
    assert m in (1, 2, 3, 4, 6, 8)
    for (F, P) in cr.WEIGHT_SHAPES:
        for n_frames in cr.WEIGHT_FRAMES:
            z = sr.demap_input(table, n_frames * F, 7 + F)
            w = cr.weights_for(F, P, n_frames, 9 + F)
            got = cr.ref_weighted_llr(z, w, table, F, 0.75)
            ones = cr.ref_weighted_llr(z, np.ones((n_frames, P), np.float32), table, F, 0.75)
            assert sr.same_floats(ones, sr.ref_llr_records(z, table, F, 0.75))                 # all weights 1: the plain LLRs
            wj = w[:, np.arange(F) % P].ravel()
            ok = np.isfinite(wj) & (wj > 0)
            rec = got.reshape(-1, m)
            assert not rec[~ok].view(np.uint32).any()                                          # +0.0, NaN symbols included
            plain = sr.ref_llr(z, table, 1.0)
            with np.errstate(all="ignore"):
                want = ((np.float32(0.75) * wj).astype(np.float32)[:, None] * plain).astype(np.float32)
            assert sr.same_floats(rec[ok], want[ok])


def test_planted_weights_straddle_the_seams():
    for (F, P) in cr.WEIGHT_SHAPES:
        w = cr.weights_for(F, P, 5, 9 + F)
        wj = w[:, np.arange(F) % P].ravel()
        bad = ~(np.isfinite(wj) & (wj > 0))
        good = w[np.isfinite(w) & (w > 0)]
        assert good.min() >= 1e-41 and bad.any()
        if P == F > 64:                                # one weight per symbol: both sides of every seam hold a planted value
            planted = np.isin(wj.view(np.uint32), cr.PLANTED.view(np.uint32))
            for s in (F - 1, F, 63, 64, 2 * F - 1, 2 * F):
                assert planted[s], (F, s)


@pytest.mark.parametrize("m", sorted(cr.LINK_NOISE))
def test_link_conditions_on_the_reference_chain(m):
    """The noise level and seed of the link: with weights the reference chain decodes all 16 frames, also at 1.25 times the
    noise amplitude; without weights it gets at least 8 frames wrong.  A frame with zeroed training symbols is all erasures."""
    L = cr.link_format(m)
    f = L["f"]
    assert abs(np.fft.fft(cr.LINK_TAPS, 64)[cr.LINK_NULL_BIN]) <= 0.05 + 1e-9 and f.kind[cr.LINK_NULL_BIN] == r.DATA
    assert len(cr.LINK_TAPS) - 1 <= f.n_cp and cr.LINK_FRAMES == 16
    payload, sent, tx = cr.link_transmit(m)
    assert tx.shape == (16, f.frame_samples) and sent.shape == (16, m * f.data_syms)
    rx = cr.link_channel(m, tx)
    decoded, llr, g = cr.link_receive(m, rx, True)
    louder = cr.link_receive(m, cr.link_channel(m, tx, cr.LINK_MARGIN), True)[0]
    flat = cr.link_receive(m, rx, False)[0]
    s, _, qscale = cr.link_scales(m)
    print("m %d: weighted %d wrong, at %.2f x noise %d, unweighted %d of 16; largest |q| %.1f" %
          (m, cr.frames_wrong(decoded, payload), cr.LINK_MARGIN, cr.frames_wrong(louder, payload), cr.frames_wrong(flat, payload),
           float(np.abs(llr).max() * qscale)))
    assert cr.frames_wrong(decoded, payload) == 0 and cr.frames_wrong(louder, payload) == 0
    assert cr.frames_wrong(flat, payload) >= 8
    dead = rx.copy().reshape(16, -1, f.sym_len)
    dead[5, : f.n_train] = 0
    _, llr0, g0 = cr.link_receive(m, dead.reshape(rx.shape), True)
    assert not g0[5].any() and not llr0[5].view(np.uint32).any() and not np.isnan(llr0).any()
    assert llr0[np.arange(16) != 5].tobytes() == llr[np.arange(16) != 5].tobytes()
