"""CPU checks behind tests/test_gpu_syncest.py (no GPU needed).
Part 1: tests/syncest_ref.py's f64 restatement (ref_sums) has the oracle's angles, so its SUMS are a reference for
timing_sum / freq_sum; every angle input is coherent enough.
Part 2: the numpy model of syncest_kernel's arithmetic (f32 rotor table, f32 filter, f64 products and sum) against the oracle
on every input the GPU test uses: the measured distance is what the GPU tolerance (four times it) rests on.
Part 3: the loop the estimators exist for, on the reference alone: timing estimate -> tau -> symbols -> 4th-power phase
estimate -> rotation -> bits; one of the four quarter-turn hypotheses has zero bit errors.
Part 4: what of comms_syncest_* needs no device."""
import ctypes as C

import numpy as np
import pytest

import oracle
import rx_ref
import symsync_ref
import syncest_ref as sr
from symsync_ref import SymSyncRef
from test_estimators import freq_stream


# ------------------------------------------------------------------ parts 1 and 2
def test_restatement_has_the_oracle_angles_and_inputs_are_coherent():
    for idx, (name, n, d, alpha, x) in enumerate(sr.cases()):
        ref = sr.reference(idx)
        assert abs(np.angle(ref["fs"]) - ref["freq"]) <= 1e-12, (name, n, d)
        if x.size < 2:
            assert ref["fs"] == 0 and ref["freq"] == 0.0
        else:
            assert abs(ref["fs"]) / ref["fa"] > sr.MIN_COHERENCE, (name, n, d)
        if ref["ta"] == 0.0:          # no delayed product, or alpha = 0 (q(t) is identically zero)
            assert ref["ts"] == 0 and ref["timing"] == 0.0 and (x.size <= n * d or alpha == 0.0), (name, n, d)
        else:
            assert sr.circ(sr.timing_of(ref["ts"], n), ref["timing"], n) <= 1e-12, (name, n, d)
            assert abs(ref["ts"]) / ref["ta"] > sr.MIN_COHERENCE, (name, n, d)


def test_model_distance_from_the_oracle_on_every_gpu_input():
    """The figures in syncest_ref.py (MODEL_TIMING_DISTANCE, MODEL_SUM_DISTANCE) are the largest seen here."""
    worst_t = worst_s = 0.0
    for idx, (name, n, d, alpha, x) in enumerate(sr.cases()):
        ref = sr.reference(idx)
        ts, fs = sr.model_sums(x, n, d, alpha)
        assert abs(fs - ref["fs"]) <= sr.FREQ_SUM_TOL * ref["fa"]          # the frequency arithmetic is f64 in the model too
        if ref["ta"] == 0.0:
            assert ts == 0
            continue
        dt = sr.circ(sr.timing_of(ts, n), ref["timing"], n)
        ds = abs(ts - ref["ts"]) / ref["ta"]
        print("%-22s n=%d d=%2d alpha=%.2f len=%7d: timing %+.6f, model off by %.3e samples, sum by %.3e of sum|terms|"
              % (name, n, d, alpha, x.size, ref["timing"], dt, ds))
        assert dt <= sr.MAX_MODEL_DISTANCE, (name, n, d, dt)               # else: replace the input
        worst_t, worst_s = max(worst_t, dt), max(worst_s, ds)
    print("largest: %.4e samples, %.4e of sum|terms|" % (worst_t, worst_s))
    assert worst_t <= sr.MODEL_TIMING_DISTANCE and worst_s <= sr.MODEL_SUM_DISTANCE
    assert sr.TIMING_TOL == 4 * sr.MODEL_TIMING_DISTANCE and sr.TIMING_SUM_TOL == 4 * sr.MODEL_SUM_DISTANCE


def test_an_estimate_at_the_wrap_compares_circularly():
    # (2, 5): the signal's peaks sit half a symbol from the block's start -- the oracle's own estimate lands on either side
    seen = {np.sign(sr.reference(idx)["timing"]) for idx, (name, n, d, _, x) in enumerate(sr.cases()) if (n, d) == (2, 5) and x.size >= sr.TILE - 1}
    assert seen == {-1.0, 1.0}
    assert sr.circ(0.99996, -0.99996, 2) < 1e-4 and sr.circ(0.5, -0.5, 2) == 1.0


def test_frequency_on_the_reference_test_signal():
    # frequency_estimator.rs's test: truth 0.123456789, its bound 0.01 -- still met by the stream rounded to Complex<f32>
    x = freq_stream(np.random.default_rng(0), 0.123456789).astype(np.complex64)
    ts, fs = sr.model_sums(x, 4, 4, 0.25)
    assert abs(np.angle(fs) - oracle.frequency_offset_estimate(x.astype(np.complex128))) <= sr.ANGLE_TOL
    assert abs(0.123456789 - np.angle(fs)) < 0.01


# ------------------------------------------------------------------ part 3: the loop, on the reference
def loop_on_reference(dd):
    """(timing estimate, [bit errors of the four hypotheses], bits compared)."""
    L, S = sr.LOOP_L, sr.LOOP_S
    v, x, h = sr.loop_signal(dd)
    e = oracle.timing_push(x.astype(np.complex128), S, sr.LOOP_D, sr.LOOP_BETA)
    tau = symsync_ref.tau_from_estimate(e, h.size, L, S)
    ref = SymSyncRef(h, L, S)
    ref.set_timing(tau)
    y = ref.run_c(x)
    ph = oracle.psk_phase_estimate(y.astype(np.complex64).astype(np.complex128), 4)
    errs = []
    for rot in sr.loop_rotations(ph):
        got = rx_ref.decide((y * np.exp(1j * rot)).astype(np.complex64), rx_ref.QPSK_DEF)
        n_err, n_bits = sr.loop_bit_errors(got, v, h)
        errs.append(n_err)
    return e, errs, n_bits


@pytest.mark.parametrize("dd", sr.LOOP_DD)
def test_the_loop_on_the_reference_alone(dd):
    e, errs, n_bits = loop_on_reference(dd)
    print("dd=%d: estimate %+.4f samples, bit errors of the four quarter turns %s of %d" % (dd, e, errs, n_bits))
    assert n_bits > 3500 and min(errs) == 0 and sorted(errs)[1] > n_bits // 4
    if dd == 64:
        assert abs(abs(e) - sr.LOOP_S / 2.0) < 0.01        # the estimate at the wrap


# ------------------------------------------------------------------ part 4: the library without a device
@pytest.fixture(scope="module")
def c():
    import __graft_entry__ as g

    g.build()
    import comms_rs_amd as c

    return c


def test_arguments_are_checked_before_the_device(c):
    from comms_rs_amd import _lib

    lib = _lib.lib()
    h = C.c_void_p()
    for n, d, alpha in ((8, 64, 0.25), (257, 1, 0.25), (0, 4, 0.25), (4, 0, 0.25), (4, 4, 1.5), (4, 4, -0.1), (4, 4, float("nan")),
                        (256, 2, 0.25)):
        assert lib.comms_syncest_create(n, d, alpha, 0, C.byref(h)) == 1 and not h, (n, d, alpha)
    assert lib.comms_syncest_create(4, 4, 0.25, 0, None) == 1
    for bad in ((8, 64, 0.25), (257, 1, 0.25), (4, 4, 1.5)):
        with pytest.raises(c.CommsError) as e:
            c.SyncEstimatorNode(*bad)
        assert e.value.code == 1
    assert lib.comms_syncest_destroy(None) == 0
    out = (C.c_double * 6)()
    for call in (lambda: lib.comms_syncest_run_dev(None, None, 0, out, None), lambda: lib.comms_syncest_run(None, None, 0, out),
                 lambda: lib.comms_syncest_get_kernel(None, 8, None, 0), lambda: lib.comms_syncest_set_timer(None, None),
                 lambda: lib.comms_psk_phase_estimate_c32(None, 0, 0, C.byref(C.c_double()), 0),
                 lambda: lib.comms_psk_phase_estimate_c32_dev(None, 0, 0, C.byref(C.c_double()), 0, None),
                 lambda: lib.comms_qam_phase_estimate_c32(None, 4, C.byref(C.c_double()), 0),
                 lambda: lib.comms_qam_phase_estimate_c32(None, 0, None, 0)):
        assert call() == 1


def test_sync_estimator_has_no_cpu_fallback(c):
    if c.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(c.CommsError) as e:
        c.SyncEstimatorNode(4, 4, 0.25)
    assert e.value.code == 2
    with pytest.raises(c.CommsError) as e:
        c.psk_phase_estimate_c32(np.ones(4, np.complex64), 4)
    assert e.value.code == 2
