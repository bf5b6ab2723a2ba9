"""CPU checks behind tests/test_gpu_framesync.py (no GPU needed).
Part 1: the numpy model of framesync_kernel's arithmetic against the f64 definition on every block the GPU test uses: the
measured distances are what the GPU tolerances (four times them) rest on.
Part 2: a condition on the INPUTS: every metric keeps DECISION_MARGIN from the threshold and every detection beats its guard
window by it, so that no rounding within the tolerance can flip a decision and indices can be compared exactly.
Part 3: the definition cut into calls and flushed equals the uncut one -- the latency rule.
Part 4: the loop the node exists for, on the reference alone and with NO hypotheses: timing estimate -> symbols -> detection ->
derotation by arg c -> payload bits from index + P.
Part 5: what of comms_framesync_* needs no device."""
import ctypes as C

import numpy as np
import pytest

import framesync_ref as fr
import oracle
import rx_ref
import symsync_ref
import syncest_ref as sr
from symsync_ref import SymSyncRef


# ------------------------------------------------------------------ the words are what they claim to be
def test_words():
    W = fr.words()
    assert [w.size for w in W.values()] == [13, 63, 32, 2, 512]
    for name in ("barker13", "mseq63"):
        w = W[name].real.astype(np.int64)
        assert set(w) == {-1, 1}
    b = W["barker13"].real
    assert max(abs(np.correlate(b, b, "full")[:12])) == 1                        # Barker: aperiodic sidelobes of at most 1
    m = W["mseq63"].real
    assert int(np.sum(m == -1)) == 32                                              # an m-sequence: 32 ones, 31 zeros ...
    assert all(np.dot(m, np.roll(m, s)) == -1 for s in range(1, 63))               # ... periodic sidelobes of exactly -1
    for name, (thr, G) in fr.SETUP.items():
        assert 0 < thr <= 1 and 0 <= G <= 512 and 2 <= W[name].size <= 512


# ------------------------------------------------------------------ parts 1 and 2
def test_model_distance_from_the_definition_on_every_gpu_input():
    """The figures in framesync_ref.py (MODEL_METRIC_DISTANCE, MODEL_CORR_DISTANCE) are the largest seen here."""
    worst_m = worst_c = 0.0
    for idx, (name, wn, thr, G, y, ties) in enumerate(fr.cases()):
        p = fr.words()[wn]
        ref = fr.reference(idx)
        k, c, m, e, mm = fr.model_detect(y, p, thr, G)
        assert np.array_equal(k, ref["index"]), (name, k, ref["index"])
        Ep = float(np.sum(np.abs(p.astype(np.complex128)) ** 2))
        dm = float(np.max(np.abs(m - ref["m"]), initial=0.0))
        dc = float(np.max(np.abs(c - ref["c"]) / np.sqrt(Ep * ref["e"]), initial=0.0))
        de = float(np.max(np.abs(e - ref["e"]) / ref["e"], initial=0.0))
        fin = np.isfinite(ref["metrics"])
        dall = float(np.max(np.abs(mm.astype(np.float64)[fin] - ref["metrics"][fin]), initial=0.0))
        print("%-18s %-8s P=%3d G=%3d len=%7d: %3d detections, metric off by %.3e (all positions %.3e), corr by %.3e, energy by %.3e"
              % (name, wn, p.size, G, y.size, k.size, dm, dall, dc, de))
        worst_m, worst_c = max(worst_m, dm, dall), max(worst_c, dc, de)       # the energy shares the correlation's bound
    print("largest: metric %.4e, corr %.4e of sqrt(Ep e)" % (worst_m, worst_c))
    assert worst_m <= fr.MODEL_METRIC_DISTANCE and worst_c <= fr.MODEL_CORR_DISTANCE
    assert fr.METRIC_TOL == 4 * fr.MODEL_METRIC_DISTANCE and fr.CORR_TOL == 4 * fr.MODEL_CORR_DISTANCE
    assert fr.DECISION_MARGIN >= 8 * fr.MODEL_METRIC_DISTANCE


def test_every_decision_has_its_margin():
    for idx, (name, wn, thr, G, y, ties) in enumerate(fr.cases()):
        ref = fr.reference(idx)
        mm = ref["metrics"]
        fin = mm[np.isfinite(mm)]
        gap = float(np.min(np.abs(fin - thr), initial=1.0))
        assert gap >= fr.DECISION_MARGIN, (name, "a metric lies %.3e from the threshold" % gap)
        for k, m in zip(ref["index"], ref["m"]):
            i = k + G
            others = np.concatenate([mm[i - G: i], mm[i + 1: i + G + 1]])
            if ties:
                others = others[others != m]          # identical windows: identical bits on every implementation
            assert np.all(m - others >= fr.DECISION_MARGIN), (name, k)
        # ... and every position over the threshold that is NO detection loses to a neighbour by the margin (or ties with it)
        with np.errstate(invalid="ignore"):
            over = np.nonzero(mm[G: G + y.size] >= thr)[0]
        for k in np.setdiff1d(over, ref["index"]):
            i = k + G
            nb = np.concatenate([mm[i - G: i], mm[i + 1: i + G + 1]])
            with np.errstate(invalid="ignore"):
                beaten = np.any(nb - mm[i] >= fr.DECISION_MARGIN) or np.any(np.isnan(nb))
            assert beaten or (ties and np.any(nb[:G] == mm[i])), (name, k)


def test_expected_detections_of_the_special_streams():
    got = {cs[0]: fr.reference(i)["index"].tolist() for i, cs in enumerate(fr.cases())}
    for tag, P, G in (("w13", 13, 12), ("w63", 63, 62), ("w32", 32, 31), ("w512", 512, 511)):
        edge = fr.TILE - (P + G) + 1
        assert got[tag + "-A"] == [0, fr.TILE - P, fr.TILE], tag
        assert got[tag + "-B"] == [1, edge - 1, fr.TILE - 1], tag
        assert got[tag + "-C"] == [edge, fr.TILE + 1], tag
    for k in (0, fr.TILE - 2, fr.TILE):                                       # p2: any pair (a, -a) of the payload is a match too
        assert k in got["w2-A"]
    assert got["two-apart-G+1"] == [100, 121] and len(got["two-apart-G"]) == 1
    assert got["largest-guard"] == [100, 613, 1400]
    assert got["tie-repeat"] == [50, 200]                                     # the earliest of equals, once per run of words
    assert got["all-zero"] == [] and got["constant"] == [] and got["constant-p2"] == [] and got["shorter-than-word"] == []
    assert got["one-nan"] == [100, 400]                                       # the word at 295 holds the NaN
    big = got["past-the-grid"]
    assert {7, (fr.GRID_CAP // 2) * fr.TILE + fr.TILE - 5, fr.N_BIG - 20} <= set(big) and len(big) == 23


# ------------------------------------------------------------------ the dense streams (tests/test_gpu_dense_metrics.py)
def test_dense_streams_model_distance_and_every_position_a_detection():
    """At every position of the dense streams the model's metric stays within MODEL_METRIC_DISTANCE and its correlation within
    MODEL_CORR_DISTANCE of the definition; the energy of 512 taps does not (DENSE_CORR_DISTANCE records it).  And what the dense
    GPU test rests on: no e is 0, every metric of the model and of the definition exceeds 1e-12, both report every position."""
    worst = 0.0
    for wn in fr.DENSE_WORDS:
        y, p = fr.dense_stream(wn), fr.words()[wn]
        assert y.size == fr.DENSE_N + p.size - 1
        k, c, m, e, _ = fr.ref_detect(y, p, fr.DENSE_THR, 0)
        km, cm, mm, em, _ = fr.dense_detect(wn, fr.DENSE_THR)
        assert np.array_equal(k, np.arange(y.size)) and np.array_equal(km, k), wn
        Ep = float(np.sum(np.abs(p.astype(np.complex128)) ** 2))
        dm, dc, de = np.max(np.abs(mm - m)), np.max(np.abs(cm - c) / np.sqrt(Ep * e)), np.max(np.abs(em - e) / e)
        print("dense %-8s %d positions: metric off by %.3e, corr by %.3e, energy by %.3e; metrics %.3e ... %.3f" % (wn, y.size, dm, dc, de, mm.min(), mm.max()))
        assert dm <= fr.MODEL_METRIC_DISTANCE and dc <= fr.MODEL_CORR_DISTANCE and de <= fr.DENSE_CORR_DISTANCE, wn
        assert min(e.min(), em.min()) > 0 and min(m.min(), mm.min()) > 1e-12 and mm.max() > 0.9, wn
        worst = max(worst, dc, de)
    assert worst <= fr.DENSE_CORR_DISTANCE <= 1.05 * worst


def test_dense_picks_cover_every_lane_column_of_both_passes():
    for wn in fr.DENSE_WORDS:
        P, T = fr.words()[wn].size, fr.dense_stream(wn).size
        m = fr.dense_sums(wn)[3][: fr.DENSE_N]
        lo, hi = np.percentile(m, [20, 80])
        first = fr.first_pass_picks(wn)
        assert sorted(first) == list(range(8)) and len({k // fr.TILE for k in first.values()}) >= 2, wn
        for col, k in first.items():
            r = (k - (1 - P)) % fr.TILE                   # a single call's first decided position is -(P + 0) + 1
            assert r % 8 == col and lo <= m[k] <= hi and min(np.sum(m >= m[k]), np.sum(m < m[k])) >= 800, (wn, col)
        G = fr.LATE_GUARD
        late = fr.late_pass_picks(wn)
        peaks = set(fr.dense_detect(wn, fr.DENSE_THR, G)[0].tolist())
        assert sorted(late) == list(range(8)) and len({k for k, _ in late.values()}) == 8, wn
        for col, (k, n1) in late.items():
            r = k - (n1 - (P + G) + 1)                    # counted from the second call's first decided position
            assert k in peaks and 0 <= n1 and r < min(fr.TILE, T - n1), (wn, col)
            assert fr.PASS <= r + G < fr.TILE + 2 * G and (r + G) % 8 == col, (wn, col)     # metric r + G: second pass, that column


# ------------------------------------------------------------------ part 3
def test_cut_and_flushed_equals_uncut():
    rng = np.random.default_rng(5)
    for name in ("w13-A", "w32-B", "two-apart-G+1", "tie-repeat", "one-nan", "shorter-than-word", "w2-A"):
        idx = fr.case(name)
        _, wn, thr, G, y, _ = fr.cases()[idx]
        p = fr.words()[wn]
        want = fr.reference(idx)["index"]
        P = p.size
        for cuts in ([], [1], [P - 1], [P + G], sorted(rng.integers(0, y.size + 1, 9).tolist()), list(range(1, min(y.size, 64)))):
            cuts = [c for c in cuts if c <= y.size]
            got = fr.ref_detect_cut(y, p, thr, G, cuts)
            assert np.array_equal(got, want), (name, cuts, got, want)


# ------------------------------------------------------------------ part 4: the loop, on the reference, nothing searched
def loop_on_reference(dd, quarter):
    L, S = sr.LOOP_L, sr.LOOP_S
    v, x, h = fr.loop_signal(dd, quarter)
    word = fr.words()[fr.LOOP_WORD]
    e = oracle.timing_push(x.astype(np.complex128), S, sr.LOOP_D, sr.LOOP_BETA)
    ref = SymSyncRef(h, L, S)
    ref.set_timing(symsync_ref.tau_from_estimate(e, h.size, L, S))
    y = ref.run_c(x).astype(np.complex64)
    k, c, m, _, _ = fr.ref_detect(y, word, fr.LOOP_THR, word.size - 1)
    assert k.size == 1, (dd, quarter, k, m)
    first = int(k[0]) + word.size
    pay = y[first: first + fr.LOOP_NPAY].astype(np.complex128) * np.exp(-1j * np.angle(c[0]))
    assert pay.size == fr.LOOP_NPAY
    got = rx_ref.decide(pay.astype(np.complex64), rx_ref.QPSK_DEF)
    return int(k[0]), float(m[0]), float(np.angle(c[0])), rx_ref.bit_errors(rx_ref.pack(got, 2), rx_ref.pack(v, 2), 2 * v.size)


@pytest.mark.parametrize("quarter", fr.LOOP_QUARTERS)
@pytest.mark.parametrize("dd", sr.LOOP_DD)
def test_the_loop_on_the_reference_alone(dd, quarter):
    k, m, ph, errs = loop_on_reference(dd, quarter)
    print("dd=%d quarter=%d: word at symbol %d, metric %.4f, rotation %+.4f rad, %d bit errors of %d" % (dd, quarter, k, m, ph, errs, 2 * fr.LOOP_NPAY))
    assert errs == 0 and m > 0.9


# ------------------------------------------------------------------ part 5: the library without a device
@pytest.fixture(scope="module")
def c():
    import __graft_entry__ as g

    g.build()
    import comms_rs_amd as c

    return c


BAD_CREATE = [("n_word", dict(n_word=1)), ("n_word", dict(n_word=513)), ("guard", dict(guard=513)), ("threshold", dict(thr=0.0)),
              ("threshold", dict(thr=1.5)), ("threshold", dict(thr=float("nan"))), ("threshold", dict(thr=-0.5)), ("word", dict(word=None)),
              ("word", dict(word=np.array([1, np.nan], np.complex64))), ("word", dict(word=np.array([1, np.inf], np.complex64))),
              ("word", dict(word=np.zeros(4, np.complex64)))]


def create_args(word=fr.words()["barker13"], n_word=None, thr=0.8, guard=12):
    ptr = None if word is None else np.ascontiguousarray(word, np.complex64).ctypes.data_as(C.c_void_p)
    return ptr, (13 if word is None else len(word)) if n_word is None else n_word, thr, guard


def test_arguments_are_checked_before_the_device(c):
    from comms_rs_amd import _lib

    lib = _lib.lib()
    for names, kw in BAD_CREATE:
        h = C.c_void_p()
        ptr, n, thr, guard = create_args(**kw)
        assert lib.comms_framesync_create(ptr, n, thr, guard, 0, C.byref(h)) == 1 and not h, kw
        assert names in lib.comms_last_error().decode(), (kw, lib.comms_last_error())
    assert lib.comms_framesync_create(*create_args(), 0, None) == 1
    m = C.c_size_t()
    assert lib.comms_framesync_state_len(13, 12, C.byref(m)) == 0 and m.value == 13 + 24 - 1
    assert lib.comms_framesync_state_len(2, 0, C.byref(m)) == 0 and m.value == 1
    assert lib.comms_framesync_state_len(1, 0, C.byref(m)) == 1 and lib.comms_framesync_state_len(13, 513, C.byref(m)) == 1
    assert lib.comms_framesync_state_len(13, 12, None) == 1
    with pytest.raises(c.CommsError) as e:
        c.FrameSyncNode(np.ones(1, np.complex64), 0.5, 0)
    assert e.value.code == 1
    assert lib.comms_framesync_destroy(None) == 0
    n = C.c_size_t()
    for call in (lambda: lib.comms_framesync_run_dev(None, None, 0, None, 0, C.byref(n), None),
                 lambda: lib.comms_framesync_run(None, None, 0, None, 0, C.byref(n)),
                 lambda: lib.comms_framesync_flush(None, None, 0, C.byref(n)),
                 lambda: lib.comms_framesync_get_state(None, None, 0), lambda: lib.comms_framesync_set_state(None, None, 0),
                 lambda: lib.comms_framesync_get_position(None, None), lambda: lib.comms_framesync_set_position(None, 0),
                 lambda: lib.comms_framesync_set_threshold(None, 0.5), lambda: lib.comms_framesync_get_kernel(None, 8, None, 0),
                 lambda: lib.comms_framesync_set_timer(None, None)):
        assert call() == 1


def test_frame_synchroniser_has_no_cpu_fallback(c):
    if c.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(c.CommsError) as e:
        c.FrameSyncNode(fr.words()["barker13"], 0.8, 12)
    assert e.value.code == 2
