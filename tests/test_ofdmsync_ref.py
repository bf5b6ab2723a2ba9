"""What the GPU tests of the OFDM synchroniser rest on, checked without a GPU: the definition's own properties, the distance of
the f32 model of the kernels' order from the definition (METRIC_BOUND and CORRECT_BOUND are four times it), that no decision
of any test stream lies within 2 METRIC_BOUND of flipping, and that the link's inputs decode in the reference chain."""
import ctypes as C
import functools

import numpy as np
import pytest

import ofdm_ref as r
import ofdmsync_ref as o


# ---------------------------------------------------------------- the definition
def clean_frame(eps=0.0, gain=1.0, lead=300):
    f = o.small_format(n_syms=2)
    x, starts = o.build_stream(f, (lead,), eps, 9, sigma=0.0, tail=400)
    return f, (x.astype(np.complex128) * gain), int(starts[0])


def test_metric_lies_in_the_unit_interval():
    for cs in o.cases():
        _, _, m = o.ref_metric(cs.x, cs.L, cs.W, -cs.G, cs.x.size + 1)
        assert m.min() >= 0.0 and m.max() <= 1.0 + 1e-12, cs.name


def test_metric_ignores_amplitude_rotation_and_cfo():
    f, x, _ = clean_frame()
    x = x + 0.05 * np.random.default_rng(3).standard_normal(x.size)
    L = f.sym_len
    _, _, m0 = o.ref_metric(x, L, L, 0, x.size)
    n = np.arange(x.size)
    for y in (x * 37.5, x * np.exp(1.234j), x * np.exp(1j * 0.7 * np.pi / L * n), x * np.exp(-1j * 0.031 * n) * 1e-3):
        _, _, m = o.ref_metric(y, L, L, 0, x.size)
        assert np.max(np.abs(m - m0)) < 1e-9


@pytest.mark.parametrize("eps", [0.0, 0.3 * np.pi / 80, -0.9 * np.pi / 80])
def test_clean_frame_peaks_at_its_first_sample_and_gives_its_cfo(eps):
    f, x, start = clean_frame(eps, gain=0.3 * np.exp(2.2j))
    L = f.sym_len
    # without a channel the two training symbols repeat exactly over the window at the frame's first sample
    y = np.zeros(x.size, np.complex128)
    y[start: start + f.frame_samples] = r.ref_mod(f, r.data_values(f, 1)).ravel()
    y = y * np.exp(1j * eps * np.arange(y.size)) * 0.3 * np.exp(2.2j)
    det = o.ref_detect(y, L, L, 40, 0, 0.5)
    assert det.size == 1 and det["d"][0] == start and abs(det["m"][0] - 1.0) < 1e-12
    assert abs(o.ref_cfo(det["P"][0], L) - eps) < 1e-12
    # through the three-tap channel the first two of the window's L products see the silence in front of the frame: the peak
    # stays within the channel's length of the first sample, and the angle of P moves by less than 2 / L
    det = o.ref_detect(x, L, L, 40, 0, 0.5)
    assert det.size == 1 and 0 <= det["d"][0] - start <= 2 and abs(o.ref_cfo(det["P"][0], L) - eps) < 2.0 / L / L


def test_correct_inverts_the_applied_cfo():
    x, cfo = o.correct_input(1280, 3)
    n = np.arange(1280)
    turned = x.astype(np.complex128) * np.exp(1j * cfo[:, None] * n[None, :])
    assert np.max(np.abs(o.ref_correct(turned, cfo) - x)) < 1e-12
    assert np.array_equal(o.ref_correct(x, np.zeros(3)), x.astype(np.complex128))


# ---------------------------------------------------------------- the bounds
def streams():
    """(name, L, W, G, A, thr, stream) of every GPU comparison with the definition."""
    out = [(cs.name,) + (cs.L, cs.W, cs.G, cs.A, cs.thr, cs.x) for cs in o.cases()]
    out.append(("late", 80, 80, 40, 8, 0.5, o.case("sym80").x[: o.late_cut()]))
    out.append(("seams", 80, 80, 40, 8, 0.5, o.seam_stream()[0]))
    out.append(("link", 80, 80, o.LINK_GUARD, o.LINK_ADVANCE, o.LINK_THRESHOLD, link_x()))
    return out


@functools.lru_cache(maxsize=None)
def link_x():
    f = o.link_ofdm()
    return o.link_stream(r.ref_mod(f, o.link_transmit()[4]))[0]


def metric_distance(x, L, W, G):
    P, R, m = o.ref_metric(x, L, W, -G, x.size + G + 1)
    Pm, Rm, mm = o.model_metric(x, L, W, -G, x.size + G + 1)
    ok = R > 0
    return max(float(np.max(np.abs(Pm[ok] - P[ok]) / R[ok])), float(np.max(np.abs(Rm[ok] - R[ok]) / R[ok])), float(np.max(np.abs(mm - m))))


def unsafe_positions(x, L, W, G, thr, bound):
    """Positions whose decision could flip under an error of `bound` in every metric."""
    _, _, m = o.ref_metric(x, L, W, -G, x.size + G + 1)
    thr = float(np.float32(thr))
    bad = list(np.flatnonzero(np.abs(m - thr) <= 2 * bound) - G)
    for k in np.flatnonzero(m >= thr):
        if k - G < 0 or k + G >= m.size:
            continue
        before, after = m[k - G: k], m[k + 1: k + G + 1]
        if np.all(m[k] > before) and np.all(m[k] >= after):
            safe = np.all(m[k] - before > 2 * bound) and np.all(m[k] - after > 2 * bound)
        else:
            safe = np.any(before - m[k] > 2 * bound) or np.any(after - m[k] > 2 * bound)
        if not safe:
            bad.append(k - G)
    return bad


def test_metric_bound_is_four_times_the_models_distance():
    worst = 0.0
    for name, L, W, G, A, thr, x in streams():
        dist = metric_distance(x, L, W, G)
        print("%s: model_metric is %.3e from ref_metric" % (name, dist))
        worst = max(worst, dist)
    print("worst %.3e, METRIC_MODEL_WORST %.3e, METRIC_BOUND %.3e" % (worst, o.METRIC_MODEL_WORST, o.METRIC_BOUND))
    assert worst <= o.METRIC_MODEL_WORST <= 1.05 * worst and o.METRIC_BOUND == 4 * o.METRIC_MODEL_WORST


def test_correct_bound_is_four_times_the_models_distance():
    worst = 0.0
    for F, n_frames in o.CORRECT_SHAPES:
        x, cfo = o.correct_input(F, n_frames)
        dist = o.correct_distance(o.model_correct(x, cfo), o.ref_correct(x, cfo), x)
        print("records of %d x %d: model_correct is %.3e from ref_correct" % (F, n_frames, dist))
        worst = max(worst, dist)
    print("worst %.3e, CORRECT_MODEL_WORST %.3e, CORRECT_BOUND %.3e" % (worst, o.CORRECT_MODEL_WORST, o.CORRECT_BOUND))
    assert worst <= o.CORRECT_MODEL_WORST <= 1.05 * worst and o.CORRECT_BOUND == 4 * o.CORRECT_MODEL_WORST
    x, _ = o.correct_input(1280, 3)
    assert np.array_equal(o.model_correct(x, np.zeros(3)), x)                       # cfo = 0: the record's values


def test_every_decision_is_safe():
    for name, L, W, G, A, thr, x in streams():
        assert unsafe_positions(x, L, W, G, thr, o.METRIC_BOUND) == [], name


def test_streams_are_what_the_issue_asks_for():
    for cs in o.cases():
        assert cs.x.size <= 40000 and 3 <= o.reference(cs.name).size, (cs.name, cs.x.size, o.reference(cs.name).size)
    assert [(cs.L, cs.W, cs.G, cs.A) for cs in o.cases()] == [(80, 80, 40, 8), (32, 32, 16, 0), (64, 16, 8, 4), (7, 13, 3, 0),
                                                             (1280, 1280, 512, 128)]
    # the frames of the repeated-symbol cases are found at their first samples (the channel may move the peak by its length)
    x, starts = o.seam_stream()
    det = o.ref_detect(x, 80, 80, 40, 8, 0.5)
    assert x.size == (1 << 20) + 3 and np.array_equal(det["d"], starts)
    first = o.TILE - 200 + 1
    assert list(starts[:3]) == [first - 1, first + 2 * o.TILE, first + 4 * o.TILE + 1] and starts[3] > x.size - o.TILE


def test_model_detections_equal_the_references():
    for name, L, W, G, A, thr, x in streams():
        a = o.ref_detect(x, L, W, G, A, thr)
        b = o.ref_detect(x, L, W, G, A, thr, metric=o.model_metric)
        assert np.array_equal(a["index"], b["index"]), name


# ---------------------------------------------------------------- the dense streams (tests/test_gpu_dense_metrics.py)
@pytest.mark.parametrize("L,W", o.DENSE_SHAPES)
def test_dense_stream_model_distance_and_every_position_a_detection(L, W):
    """At every position of a dense stream the model stays within METRIC_MODEL_WORST of the definition; and what the dense GPU
    test rests on: no R is 0 inside the stream, every metric that has a product inside the stream exceeds 1e-12 in the model and
    in the definition, and both report exactly those positions under DENSE_THR."""
    x = o.dense_stream(L, W)
    n = x.size
    assert n == o.DENSE_N + W + L - 1
    P, R, m = o.ref_metric(x, L, W, 0, n + 1)
    Pm, Rm, mm = o.dense_model(L, W)
    assert not np.any(R[:n] == 0) and not np.any(Rm[:n] == 0) and R[n] == 0 and Rm[n] == 0
    dist = max(float(np.max(np.abs(Pm[:n] - P[:n]) / R[:n])), float(np.max(np.abs(Rm[:n] - R[:n]) / R[:n])), float(np.max(np.abs(mm - m))))
    low = min(float(m[: n - L].min()), float(mm[: n - L].min()))
    print("dense (%d, %d): model_metric is %.3e from ref_metric over %d positions; metrics %.3e ... %.3f" % (L, W, dist, n, low, mm.max()))
    assert dist <= o.METRIC_MODEL_WORST
    assert low > 1e-12 and mm.max() > 0.75 and not np.any(m[n - L:]) and not np.any(mm[n - L:])
    a, b = o.dense_expected(x, L, W), o.dense_expected(x, L, W, metric=o.ref_metric)
    assert np.array_equal(a["index"], np.arange(n - L)) and np.array_equal(b["index"], a["index"])
    assert np.array_equal(a["m"].astype(np.float32), mm[: n - L])                                     # the records ARE the model's values


def test_dense_picks_hit_every_class_the_kernel_distinguishes():
    assert o.branch_classes(33) == [(c, 1) for c in range(8)]                # a window of 33 always ends in the next block
    assert {(c, 0) for c in range(8)} <= set(o.branch_classes(13))           # one of 13 may lie inside a block, at every column
    seen = set()
    for L, W in o.DENSE_SHAPES[1:-1]:
        picks, m = o.class_picks(L, W), o.dense_model(L, W)[2][: o.DENSE_N]
        assert sorted(picks) == o.branch_classes(W), (L, W)
        lo, hi = np.percentile(m, [20, 80])
        for (col, branch), d in picks.items():
            # the kernel's own arithmetic on the lane's first element idx0 (the image starts on a multiple of 32)
            idx0 = d - d % 8
            kd, ke0, ke = idx0 >> 5, (idx0 + W - 1) >> 5, (d + W - 1) >> 5
            assert d % 8 == col and branch == (0 if ke == kd else 1 if ke == ke0 else 2) and ke in (kd, ke0, ke0 + 1)
            assert 0 <= d < o.DENSE_N and lo <= m[d] <= hi
            assert min(np.sum(m >= m[d]), np.sum(m < m[d])) >= 800          # thousands of positions around the threshold
        seen |= {b for _, b in picks}
        assert len({d // o.TILE for d in picks.values()}) >= 2               # spread over the tiles
    assert seen == {0, 1, 2}


@pytest.mark.parametrize("L,W", o.DENSE_RESIDUE_SHAPES)
def test_dense_largest_guard_model_and_definition_agree(L, W):
    x = o.dense_stream(L, W)
    for r in (0, 1, 31):
        a = o.dense_expected(x, L, W, G=o.DENSE_GUARD, lead=o.DENSE_LEAD + r)
        b = o.dense_expected(x, L, W, G=o.DENSE_GUARD, lead=o.DENSE_LEAD + r, metric=o.ref_metric)
        assert a.size >= 3 and np.array_equal(a["index"], b["index"]), (L, W, r)

def test_dense_far_positions_keep_the_block_alignment():
    assert all(K % o.BLK == 0 and o.FAR_BASE + 31 + K + o.dense_stream(2048, 2048).size <= 1 << 62 for K in o.FAR_SHIFTS)
    assert all(s in o.DENSE_SHAPES for s in o.DENSE_RESIDUE_SHAPES + o.DENSE_FAR_SHAPES)


def test_fma32_rounds_once():
    """(1 + 2^-23)(1 - 2^-23) + (255 + 3 2^-16) = M - 2^-46 with M = 256 + 3 2^-16, the midpoint of the f32 neighbours
    256 + 2^-15 and 256 + 2^-14.  In f64 (steps of 2^-44 there) the sum rounds to M, and M rounds to the even neighbour
    256 + 2^-14; the single rounding of an FMA gives 256 + 2^-15."""
    f32 = np.float32
    a, b, c = np.full(3, 1 + 2.0 ** -23, f32), np.full(3, 1 - 2.0 ** -23, f32), np.full(3, 255 + 3 * 2.0 ** -16, f32)
    assert float(a[0]) * float(b[0]) + float(c[0]) == 256 + 3 * 2.0 ** -16                  # what f64 makes of it
    assert np.all(o.fma32(a, b, c) == f32(256 + 2.0 ** -15)) and np.all(o.fma32(-a, b, -c) == -f32(256 + 2.0 ** -15))
    one = np.ones(3, f32)
    assert np.all(o.fma32(one, one, c) ==f32(256 + 2.0 ** -14))                        # the tie itself goes to even
    assert np.all(o.fma32(a, a, c) == f32(256 + 2.0 ** -14))                                  # M + 2^-22 + 2^-46: up
    import framesync_ref as fr
    assert np.all(fr._fma(a, b, c) == f32(256 + 2.0 ** -15))                                  # (a, b, acc): the same function


# ---------------------------------------------------------------- the link
def test_link_decodes_in_the_reference_chain_and_not_without_the_correction():
    f = o.link_format()
    payload = o.link_transmit()[0]
    x = link_x()
    _, starts = o.link_stream(r.ref_mod(o.link_ofdm(), o.link_transmit()[4]))
    det, recs, cfo, z, (got, passed, crc) = o.link_reference(x)
    assert det.size == o.LINK_FRAMES and np.all(np.abs(det["d"] - starts) <= 2)          # every frame found, inside the prefix
    assert np.all(det["index"] <= starts) and np.all(starts - det["index"] <= o.LINK_ADVANCE)
    assert np.max(np.abs(cfo - o.LINK_EPS)) < 0.02 * o.LINK_EPS
    assert passed.all() and np.array_equal(got, payload)
    _, _, _, _, (_, passed_raw, _) = o.link_reference(x, correct=False)
    print("without the correction %d of %d frames pass" % (int(passed_raw.sum()), o.LINK_FRAMES))
    assert not passed_raw.all()
    assert f["E"] == 4 * o.link_ofdm().data_syms


# ---------------------------------------------------------------- argument limits (shared with the GPU test)
GOOD = dict(lag=80, window=80, threshold=0.5, guard=40, advance=8, n_frame=320)
BAD_CREATE = [("lag", dict(lag=0)), ("lag", dict(lag=o.MAX_LAG + 1)), ("window", dict(window=1)), ("window", dict(window=o.MAX_WINDOW + 1)),
              ("threshold", dict(threshold=0.0)), ("threshold", dict(threshold=1.0000001)), ("threshold", dict(threshold=float("nan"))),
              ("guard", dict(guard=o.MAX_GUARD + 1)), ("advance", dict(advance=o.MAX_ADVANCE + 1)), ("n_frame", dict(n_frame=o.MAX_FRAME + 1))]
LIMITS = [dict(lag=1, window=2), dict(lag=o.MAX_LAG, window=o.MAX_WINDOW, guard=o.MAX_GUARD, advance=o.MAX_ADVANCE, n_frame=o.MAX_FRAME),
          dict(threshold=1.0, guard=0, advance=0, n_frame=0)]


def create_args(**kw):
    a = dict(GOOD, **kw)
    return a["lag"], a["window"], a["threshold"], a["guard"], a["advance"], a["n_frame"]


def test_bad_arguments_are_refused_before_the_device_is_touched():
    """No GPU is needed to be refused: COMMS_ERR_ARG comes before any device call."""
    import __graft_entry__ as g

    g.build()
    import comms_rs_amd as c

    lib = c.lib()
    for names, kw in BAD_CREATE:
        h = C.c_void_p()
        assert lib.comms_ofdmsync_create(*create_args(**kw), 0, C.byref(h)) == c.COMMS_ERR_ARG and not h, kw
        assert names in lib.comms_last_error().decode(), (kw, lib.comms_last_error())
    n = C.c_size_t()
    assert lib.comms_ofdmsync_state_len(80, 80, 40, C.byref(n)) == 0 and n.value == 80 + 80 + 2 * 40 - 1
    assert lib.comms_ofdmsync_state_len(0, 80, 40, C.byref(n)) == c.COMMS_ERR_ARG
    assert lib.comms_ofdmsync_run_dev(None, None, 0, None, None, 0, C.byref(n), None) == c.COMMS_ERR_ARG
    assert lib.comms_ofdmsync_correct_run_dev(None, None, 0, None, None, None) == c.COMMS_ERR_ARG
