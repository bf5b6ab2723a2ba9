"""CPU checks behind tests/test_gpu_deframe.py (no GPU needed).
Part 1: the numpy model of deframe_kernel's arithmetic against the f64 definition on every case the GPU test uses: the
measured distances are what the GPU tolerances (four times them) rest on.
Part 2: conditions on the INPUTS: every payload symbol keeps DECISION_MARGIN from the decision boundaries of its table -- no
symbol is excluded -- so that bits can be compared exactly; the model's bits are the definition's.
Part 3: the bookkeeping: the frames of a stream do not depend on the cuts, and the special cases emit where they should.
Part 4: the loop the node exists for, on the reference alone: timing estimate -> symbols -> detection -> ref_frames -> bits.
Part 5: what of comms_deframe_* needs no device."""
import ctypes as C

import numpy as np
import pytest

import deframe_ref as dr
import framesync_ref as fr
import oracle
import rx_ref
import symsync_ref
import syncest_ref as sr
from symsync_ref import SymSyncRef


# ------------------------------------------------------------------ parts 1 and 2
def test_model_distance_from_the_definition_on_every_gpu_input():
    """The figures in deframe_ref.py (MODEL_Z_DISTANCE, MODEL_LLR_DISTANCE) are the largest seen here."""
    worst_z = worst_l = 0.0
    for idx, cs in enumerate(dr.cases()):
        ref, left = dr.reference(idx)
        got, left_m = dr.model_frames(cs, cs.y, dr.calls(idx))
        assert left == left_m == 0, cs.name
        z, zm = dr.joined(ref, "z"), dr.joined(got, "z")
        assert z.shape == zm.shape and z.shape[0] >= 1, cs.name
        assert np.array_equal(dr.joined(ref, "index"), dr.joined(got, "index"))
        fin = np.isfinite(z)
        assert np.array_equal(fin, np.isfinite(zm)) and np.count_nonzero(~fin) == (0 if cs.nan_at is None else 1), cs.name
        dz = float(np.max(np.abs(zm[fin] - z[fin]) / np.abs(z[fin])))
        c = dr.table_of(cs).astype(np.complex128)
        dmax = np.max(np.abs(z[..., None] - c) ** 2, axis=-1)                    # frames x F: the largest d_i of each symbol
        llr, lm = dr.joined(ref, "llr"), dr.joined(got, "llr")
        s = float(np.float32(cs.scale))
        rel = np.abs(lm - llr).reshape(z.shape + (cs.K,)) / (s * dmax)[..., None]
        assert np.array_equal(np.isnan(llr), np.isnan(lm)), cs.name
        dl = float(np.nanmax(rel))
        print("%-16s F=%4d K=%d frames=%3d: z off by %.3e of |z|, LLR by %.3e of s max d" % (cs.name, cs.F, cs.K, z.shape[0], dz, dl))
        worst_z, worst_l = max(worst_z, dz), max(worst_l, dl)
    print("largest: z %.4e, LLR %.4e" % (worst_z, worst_l))
    assert worst_z <= dr.MODEL_Z_DISTANCE and worst_l <= dr.MODEL_LLR_DISTANCE
    assert dr.Z_TOL == 4 * dr.MODEL_Z_DISTANCE and dr.LLR_TOL == 4 * dr.MODEL_LLR_DISTANCE
    assert dr.DECISION_MARGIN > 8 * dr.MODEL_Z_DISTANCE


def test_every_symbol_has_its_margin_and_the_model_decides_alike():
    for idx, cs in enumerate(dr.cases()):
        ref, _ = dr.reference(idx)
        got, _ = dr.model_frames(cs, cs.y, dr.calls(idx))
        z = dr.joined(ref, "z").ravel()
        fin = np.isfinite(z)
        assert np.count_nonzero(~fin) == (0 if cs.nan_at is None else 1)         # no symbol is excluded but the NaN itself
        margin = dr.boundary_margin(z[fin], dr.table_of(cs))
        assert float(np.min(margin)) >= dr.DECISION_MARGIN, (cs.name, float(np.min(margin)))
        assert np.array_equal(dr.joined(ref, "values"), dr.joined(got, "values")), cs.name
        if cs.nan_at is not None:
            assert dr.joined(ref, "values").ravel()[~fin][0] == 0                # a NaN symbol: index 0
        # the sign of an LLR is the decided bit, on every value of the definition and of the model
        for per_call in (ref, got):
            v, llr = dr.joined(per_call, "values"), dr.joined(per_call, "llr").reshape(-1, cs.F, cs.K)
            bits = (v[..., None] >> np.arange(cs.K)) & 1
            assert not np.any((llr > 0) & (bits == 1)) and not np.any((llr < 0) & (bits == 0)), cs.name


def test_default_qpsk_llrs_are_four_s_z():
    idx = dr.case("amp1-norm")
    cs = dr.cases()[idx]
    ref, _ = dr.reference(idx)
    z, llr = dr.joined(ref, "z"), dr.joined(ref, "llr").reshape(-1, cs.F, 2)
    s = float(np.float32(cs.scale))
    assert np.allclose(llr[..., 0], 4 * s * z.real, rtol=1e-12, atol=1e-12) and np.allclose(llr[..., 1], 4 * s * z.imag, rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------ part 3
def test_frames_do_not_depend_on_the_cuts():
    rng = np.random.default_rng(9)
    for name in ("F17-K2", "straddle", "overlap", "adjacent", "one-nan", "300-frames"):
        idx = dr.case(name)
        cs = dr.cases()[idx]
        dets = dr.detections(idx)
        want, left = dr.ref_frames(cs, cs.y, dr.plan(cs.y, dets, []))
        assert left == 0
        for cuts in ([1], [cs.y.size - 1], sorted(rng.integers(0, cs.y.size + 1, 7).tolist()), list(range(1, cs.y.size, 37))):
            got, left = dr.ref_frames(cs, cs.y, dr.plan(cs.y, dets, cuts))
            assert left == 0, (name, cuts)
            for key in ("index", "z", "values", "llr"):
                assert np.array_equal(dr.joined(got, key), dr.joined(want, key), equal_nan=(key in ("z", "llr"))), (name, cuts, key)


def test_the_special_cases_emit_where_they_should():
    per_call = {cs.name: [r["index"].size for r in dr.reference(i)[0]] for i, cs in enumerate(dr.cases())}
    k = 40
    idx = dr.case("lookback-edge")
    cs = dr.cases()[idx]
    (n0, d0), (n1, d1) = dr.calls(idx)
    assert d0.size == 0 and d1.size == 1 and int(d1["index"][0]) + cs.offset == n0 - cs.lookback   # exactly lookback before the call
    assert per_call["lookback-edge"] == [0, 1]
    assert per_call["straddle"] == [0, 1]
    assert per_call["ends-at-T"] == [1, 0] and per_call["ends-at-T+1"] == [0, 1, 0]
    assert [n for n, _ in dr.calls(dr.case("ends-at-T+1"))] == [k + dr.P + 99, 1, 400 - (k + dr.P + 100)]
    assert per_call["three-calls"] == [0, 0, 0, 1]
    assert [d.size for _, d in dr.calls(dr.case("three-calls"))] == [1, 0, 0, 0]                  # admitted by the first, pending over three
    assert max(n for n, _ in dr.calls(dr.case("three-calls"))[1:3]) < 99                          # calls shorter than H = F - 1
    ov = dr.reference(dr.case("overlap"))[0][0]
    assert ov["start"].tolist() == [k + dr.P, k + 2 * dr.P + 20]                                  # the second starts inside the first
    ad = dr.reference(dr.case("adjacent"))[0][0]
    assert ad["start"].tolist() == [k + dr.P, k + 2 * dr.P + 24] and dr.records(dr.cases()[dr.case("adjacent")], ad["values"]).shape == (2, 8)
    assert sum(per_call["300-frames"]) == 300 and sum(per_call["past-the-grid"]) == 300
    for cs in dr.cases():
        assert sum(per_call[cs.name]) >= 1
    big = dr.cases()[dr.case("past-the-grid")]
    assert 300 * big.F > fr.GRID_CAP * dr.WG                                                      # more lanes than one pass of the largest grid
    for K in (1, 2):
        assert dr.records(big._replace(K=K), np.zeros((1, big.F), np.int64)).shape[1] // 4 * (32 // K) * 300 > fr.GRID_CAP * dr.WG


# ------------------------------------------------------------------ part 4: the loop, on the reference
@pytest.mark.parametrize("quarter", fr.LOOP_QUARTERS)
@pytest.mark.parametrize("dd", sr.LOOP_DD)
def test_the_loop_on_the_reference_alone(dd, quarter):
    L, S = sr.LOOP_L, sr.LOOP_S
    v, x, h = fr.loop_signal(dd, quarter)
    assert fr.LOOP_WORD == dr.WORD and fr.LOOP_NPAY == 2048
    e = oracle.timing_push(x.astype(np.complex128), S, sr.LOOP_D, sr.LOOP_BETA)
    ref = SymSyncRef(h, L, S)
    ref.set_timing(symsync_ref.tau_from_estimate(e, h.size, L, S))
    y = ref.run_c(x).astype(np.complex64)
    dets = dr.detect(y)
    assert dets.size == 1
    cs = dr.Case("loop", y, 2048, 32, dr.GUARD - 1, 2, None, False, 1.0, (), None)
    frames, left = dr.ref_frames(cs, y, dr.plan(y, dets, []))
    assert left == 0 and dr.joined(frames, "index").size == 1
    errs = rx_ref.bit_errors(dr.records(cs, dr.joined(frames, "values"))[0], rx_ref.pack(v, 2), 2 * v.size)
    print("dd=%d quarter=%d: %d bit errors of %d" % (dd, quarter, errs, 2 * v.size))
    assert errs == 0 and 2 * v.size == 4096


# ------------------------------------------------------------------ part 5: the library without a device
@pytest.fixture(scope="module")
def c():
    import __graft_entry__ as g

    g.build()
    import comms_rs_amd as c

    return c


# (what the error names, arguments of comms_deframe_create in front of the device)
BAD_CREATE = [("n_payload", (0, 32, 30, 2, None, 0)), ("n_payload", ((1 << 20) + 1, 32, 30, 2, None, 0)), ("lookback", (64, 32, (1 << 20) + 1, 2, None, 0)),
              ("offset", (64, (1 << 20) + 1, 30, 2, None, 0)), ("bits_per_sym", (64, 32, 30, 3, None, 0)), ("bits_per_sym", (64, 32, 30, 0, None, 0)),
              ("flags", (64, 32, 30, 2, None, 2))]


def test_arguments_are_checked_before_the_device(c):
    from comms_rs_amd import _lib

    lib = _lib.lib()
    assert _lib.SYM_LLR not in (_lib.SYM_C32, _lib.SYM_BITS, _lib.IQ_C32, _lib.IQ_I16, _lib.IQ_U8, _lib.BITS_U8, _lib.BITS_PACKED)
    for names, args in BAD_CREATE:
        h = C.c_void_p()
        assert lib.comms_deframe_create(*args, 0, C.byref(h)) == 1 and not h, args
        assert names in lib.comms_last_error().decode(), (args, lib.comms_last_error())
    assert lib.comms_deframe_create(64, 32, 30, 2, None, 0, 0, None) == 1
    m = C.c_size_t()
    assert lib.comms_deframe_state_len(64, 30, C.byref(m)) == 0 and m.value == 63
    assert lib.comms_deframe_state_len(8, 30, C.byref(m)) == 0 and m.value == 30
    assert lib.comms_deframe_state_len(1, 0, C.byref(m)) == 0 and m.value == 0
    assert lib.comms_deframe_state_len(1 << 20, 0, C.byref(m)) == 0 and (1 << 20) >= 65536           # the documented limit
    assert lib.comms_deframe_state_len(0, 0, C.byref(m)) == 1 and lib.comms_deframe_state_len(8, 30, None) == 1
    with pytest.raises(c.CommsError) as e:
        c.DeframeNode(0, 32, 30)
    assert e.value.code == 1
    assert lib.comms_deframe_destroy(None) == 0 and lib.comms_deframe_frame_bytes(None) == 0
    n = C.c_size_t()
    for call in (lambda: lib.comms_deframe_run_dev(None, None, 0, None, 0, None, 0, None, C.byref(n), None),
                 lambda: lib.comms_deframe_run(None, None, 0, None, 0, None, 0, None, C.byref(n)),
                 lambda: lib.comms_deframe_frames_ready(None, 0, None, 0, C.byref(n)), lambda: lib.comms_deframe_flush(None, C.byref(n)),
                 lambda: lib.comms_deframe_get_state(None, None, 0), lambda: lib.comms_deframe_set_state(None, None, 0),
                 lambda: lib.comms_deframe_get_position(None, None), lambda: lib.comms_deframe_set_position(None, 0),
                 lambda: lib.comms_deframe_get_pending(None, None, 0, C.byref(n)), lambda: lib.comms_deframe_set_pending(None, None, 0),
                 lambda: lib.comms_deframe_set_word_energy(None, 1.0), lambda: lib.comms_deframe_set_output_format(None, 0),
                 lambda: lib.comms_deframe_set_llr_scale(None, 1.0), lambda: lib.comms_deframe_get_kernel(None, 8, None, 0),
                 lambda: lib.comms_deframe_set_timer(None, None)):
        assert call() == 1


def test_deframer_has_no_cpu_fallback(c):
    if c.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(c.CommsError) as e:
        c.DeframeNode(64, 32, 30)
    assert e.value.code == 2
