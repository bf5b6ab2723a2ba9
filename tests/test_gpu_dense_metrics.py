"""GPU tests of framesync_kernel and ofdmsync_detect_kernel at EVERY position, against the f32 models of their stated order of
operations (framesync_ref.model_detect, ofdmsync_ref.model_metric), bit for bit.  Both kernels write nothing but their
detections; with guard 0 the peak rule is "m >= thr", so a tiny threshold turns every position into a detection, and a
threshold that IS a model metric turns the metric the kernel decides with (the register-window path of framesync_kernel, the
shared `mid` of ofdmsync_detect_kernel, neither of which is ever reported) into a set of thousands of memberships.  The same
streams then run at every residue of the first index modulo 32, with one NaN, and at positions past 2^32.  Streams, picks and
models come from tests/ofdmsync_ref.py and tests/framesync_ref.py; tests/test_ofdmsync_ref.py and tests/test_framesync_ref.py
check on the CPU what these tests rest on.  Run with -m gpu."""
import re

import numpy as np
import pytest

import framesync_ref as fr
import ofdmsync_ref as o

pytestmark = pytest.mark.gpu
VALUES = ("corr_re", "corr_im", "metric", "energy")
NAN = np.complex64(complex(np.nan, 1.0))
NAN_AT = o.TILE + 1000                  # a sample whose positions the middle tile of a single call decides


@pytest.fixture(scope="module")
def c():
    import comms_rs_amd as c

    assert c.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested (no CPU fallback)"
    return c


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ulps(a, b):
    return int(np.max(np.abs(bits(a).astype(np.int64) - bits(b).astype(np.int64)), initial=0))


def values(rec):
    """Every byte of the records but their indices."""
    return b"".join(np.ascontiguousarray(rec[f]).tobytes() for f in VALUES)


def restart(node, position=0, thr=None):
    """The same handle as a fresh one at `position`: zero state, nothing pending."""
    if thr is not None:
        node.set_threshold(float(thr))
    return node.set_position(int(position)).set_state(np.zeros(node.state_len(), np.complex64))


def whole(node, x):
    """One call and a flush: (all records, records of the call, records of the flush)."""
    a, b = node.run(x, raw=True), node.flush(raw=True)
    a, b = (a[0], b[0]) if isinstance(a, tuple) else (a, b)          # OfdmSyncNode returns (records, cfo)
    return np.concatenate([a, b]), a, b


def same_bits(got, index, re_, im, energy, metric, own, what):
    """Records against a model's: count, indices, then the sums and the metric bit for bit.  `own` is f32(num / den) formed
    from the GPU's own returned sums: where the sums agree and the metric does not, it tells a division that is not correctly
    rounded from everything else."""
    assert got.size == index.size, (what, got.size, index.size)
    assert np.array_equal(got["index"].astype(np.int64), index), what
    for field, want in (("corr_re", re_), ("corr_im", im), ("energy", energy)):
        off = np.flatnonzero(bits(got[field]) != bits(want))
        assert off.size == 0, "%s: %s differs from the model at %d of %d records, first at index %d, by up to %d ulps" % (
            what, field, off.size, got.size, int(index[off[0]]), ulps(got[field], want))
    off = np.flatnonzero(bits(got["metric"]) != bits(metric))
    assert off.size == 0, "%s: the sums agree, the metric differs from the model at %d records by up to %d ulps; from f32(num / den) " \
        "of the returned sums it differs by up to %d ulps" % (what, off.size, ulps(got["metric"], metric), ulps(got["metric"], own))


# ================================================================== the OFDM synchroniser
def o_kernel(node, n):
    name = node.kernel(n)
    assert name.startswith("ofdmsync_detect_kernel"), name
    return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", name)}


def o_check(got, want, what):
    pr, pi, R = got["corr_re"], got["corr_im"], got["energy"]
    own = (pr * pr + pi * pi) / (R * R)                              # float32 throughout, every operation rounded on its own
    same_bits(got, want["index"], want["P"].real, want["P"].imag, want["R"], want["m"], own, what)


def nan_free_records_survive(clean, got, reach, what):
    hit = np.isin(clean["index"].astype(np.int64), reach)
    assert int(hit.sum()) == reach.size, what                        # every position that holds the NaN was a record before
    assert got.size == clean.size - reach.size and got.tobytes() == clean[~hit].tobytes(), what


# ------------------------------------------------------------------ 1. every position, bit for bit
@pytest.mark.parametrize("L,W", o.DENSE_SHAPES)
def test_ofdmsync_every_position_equals_the_model(c, L, W):
    x = o.dense_stream(L, W)
    node = c.OfdmSyncNode(L, W, o.DENSE_THR, 0)
    got, first, last = whole(node, x)
    assert got.size == x.size - L                                    # every position that has a product inside the stream
    assert first.size == x.size - (W + L) + 1 > 16 and last.size == W - 1      # the second copy-back and the sort, on thousands
    o_check(got, o.dense_expected(x, L, W), "(%d, %d)" % (L, W))
    assert node.position() == x.size and node.found == last.size


# ------------------------------------------------------------------ 2. the decision path: thresholds that are model values
@pytest.mark.parametrize("L,W", o.DENSE_SHAPES[1:-1])
def test_ofdmsync_decides_with_the_models_metric_in_every_class(c, L, W):
    """ms[] shows through decisions only.  Per (lane column, branch) one position d: with thr = the model's m[d] exactly, the
    detections are the model's {m >= thr}, d among them -- a metric one ulp low in that class loses d, a systematic error moves
    many of the thousands of memberships."""
    x, m = o.dense_stream(L, W), o.dense_model(L, W)[2]
    picks = o.class_picks(L, W)
    assert sorted(picks) == o.branch_classes(W)
    node = c.OfdmSyncNode(L, W, o.DENSE_THR, 0)
    for (col, branch), d in picks.items():
        got, _, _ = whole(restart(node, 0, m[d]), x)
        want = np.flatnonzero(m >= m[d])
        assert want.size >= 800 and x.size - want.size >= 800
        idx = got["index"].astype(np.int64)
        assert d in idx and np.array_equal(idx, want), ((L, W), col, o.BRANCHES[branch], d, np.setxor1d(idx, want)[:8])


# ------------------------------------------------------------------ 3. every residue of `off`, the large guard, a NaN
@pytest.mark.parametrize("L,W", o.DENSE_RESIDUE_SHAPES)
def test_ofdmsync_every_residue_of_the_first_index(c, L, W):
    x = o.dense_stream(L, W)
    node = c.OfdmSyncNode(L, W, o.DENSE_THR, 0)
    assert o_kernel(node, x.size)["lds"] <= 160 * 1024
    for r in range(o.BLK):
        lead = o.DENSE_LEAD + r
        got, _, _ = whole(restart(node, lead), x)
        o_check(got, o.dense_expected(x, L, W, lead=lead), "(%d, %d) at %d" % (L, W, lead))
        assert node.position() == lead + x.size


@pytest.mark.parametrize("L,W", o.DENSE_RESIDUE_SHAPES)
def test_ofdmsync_largest_guard_at_the_extreme_residues(c, L, W):
    """Guard 512 under the tiny threshold: the guard scan runs at every position of the 3072-metric layout, and the records are
    the local maxima (tests/test_ofdmsync_ref.py: the model and the definition agree on them)."""
    x = o.dense_stream(L, W)
    node = c.OfdmSyncNode(L, W, o.DENSE_THR, o.DENSE_GUARD)
    assert o_kernel(node, x.size)["lds"] <= 160 * 1024
    for r in (0, 1, 31):
        lead = o.DENSE_LEAD + r
        got, _, _ = whole(restart(node, lead), x)
        want = o.dense_expected(x, L, W, G=o.DENSE_GUARD, lead=lead)
        assert want.size >= 3
        o_check(got, want, "(%d, %d) guard %d at %d" % (L, W, o.DENSE_GUARD, lead))


@pytest.mark.parametrize("L,W", [(7, 13), (31, 33), (80, 80)])
def test_ofdmsync_one_nan_takes_exactly_its_windows(c, L, W):
    x = o.dense_stream(L, W)
    node = c.OfdmSyncNode(L, W, o.DENSE_THR, 0)
    clean, _, _ = whole(node, x)
    bad = x.copy()
    bad[NAN_AT] = NAN
    got, _, _ = whole(restart(node), bad)
    nan_free_records_survive(clean, got, o.nan_reach(NAN_AT, L, W), (L, W))


# ------------------------------------------------------------------ 4. positions past 2^32
@pytest.mark.parametrize("L,W", o.DENSE_FAR_SHAPES)
def test_ofdmsync_positions_past_2_32(c, L, W):
    x = o.dense_stream(L, W)
    node = c.OfdmSyncNode(L, W, o.DENSE_THR, 0)
    for r in o.FAR_RESIDUES:
        s = o.FAR_BASE + r
        near, _, near_last = whole(restart(node, s), x)
        o_check(near, o.dense_expected(x, L, W, lead=s), "(%d, %d) at %d" % (L, W, s))
        assert near_last.size == W - 1
        for K in o.FAR_SHIFTS:
            assert K % o.BLK == 0
            far, _, far_last = whole(restart(node, s + K), x)
            assert far.size == near.size and far_last.size == near_last.size, (s, K)
            assert np.array_equal(far["index"], near["index"] + np.uint64(K)), (s, K)
            assert int(far_last["index"][-1]) == s + K + x.size - L - 1                  # the index the flush reports
            assert values(far) == values(near), (s, K)
            assert node.position() == s + K + x.size
        assert s + o.FAR_SHIFTS[0] < 1 << 32 < s + o.FAR_SHIFTS[0] + x.size                  # that call crosses 2^32


# ================================================================== the frame synchroniser
def f_check(got, model, Ep, what):
    idx, cc, m, e, _ = model
    cr, ci, en = got["corr_re"], got["corr_im"], got["energy"]
    own = (cr * cr + ci * ci) / (np.float32(Ep) * en)
    same_bits(got, idx, cc.real, cc.imag, e, m, own, what)


def f_energy(wn):
    p = fr.words()[wn]
    return np.float32(np.sum(p.real.astype(np.float64) ** 2 + p.imag.astype(np.float64) ** 2))


@pytest.mark.parametrize("wn", fr.DENSE_WORDS)
def test_framesync_every_position_equals_the_model(c, wn):
    y, p = fr.dense_stream(wn), fr.words()[wn]
    node = c.FrameSyncNode(p, fr.DENSE_THR, 0)
    k = node.kernel(y.size)
    assert "tile=%d " % fr.TILE in k and "tiles=3 " in k
    got, first, last = whole(node, y)
    assert got.size == y.size and first.size == y.size - p.size + 1 > 16 and last.size == p.size - 1
    f_check(got, fr.dense_detect(wn, fr.DENSE_THR), f_energy(wn), wn)
    assert node.position() == y.size


@pytest.mark.parametrize("wn", fr.DENSE_WORDS)
def test_framesync_decides_with_the_models_metric_in_every_column(c, wn):
    """The decision metric comes from the register window, the reported one from the scalar loop.  Per lane column of the first
    pass one position k at guard 0: with thr = the model's m[k] exactly, the detections are the model's {m >= thr}, k among them."""
    y, p = fr.dense_stream(wn), fr.words()[wn]
    m = fr.dense_sums(wn)[3]
    node = c.FrameSyncNode(p, fr.DENSE_THR, 0)
    picks = fr.first_pass_picks(wn)
    assert sorted(picks) == list(range(8))
    for col, k in picks.items():
        got, _, _ = whole(restart(node, 0, m[k]), y)
        want = np.flatnonzero(m >= m[k])
        assert want.size >= 800 and y.size - want.size >= 800
        idx = got["index"].astype(np.int64)
        assert k in idx and np.array_equal(idx, want), (wn, col, k, np.setxor1d(idx, want)[:8])


@pytest.mark.parametrize("wn", fr.DENSE_WORDS)
def test_framesync_decides_with_the_models_metric_in_the_last_partial_pass(c, wn):
    """With guard 0 a tile's 2048 metrics are one full pass.  Guard 8 adds a second pass of 16 metrics, of which 2048 .. 2055 are
    decided positions: one per lane column.  A peak k of the model is put there by cutting the stream so that the second call
    decides it at r = 2040 + column; with thr = the model's m[k] exactly the records are the model's, k among them, bit for bit."""
    y, p, G = fr.dense_stream(wn), fr.words()[wn], fr.LATE_GUARD
    m = fr.dense_sums(wn, G)[3]
    node = c.FrameSyncNode(p, fr.DENSE_THR, G)
    picks = fr.late_pass_picks(wn)
    assert sorted(picks) == list(range(8))
    for col, (k, n1) in picks.items():
        thr = m[k + G]
        restart(node, 0, thr)
        parts = [node.run(y[:n1], raw=True), node.run(y[n1:], raw=True), node.flush(raw=True)]
        model = fr.dense_detect(wn, thr, G)
        assert k in parts[1]["index"].astype(np.int64) and k in model[0], (wn, col, k, n1)
        f_check(np.concatenate(parts), model, f_energy(wn), "%s column %d" % (wn, col))


@pytest.mark.parametrize("wn", fr.DENSE_WORDS)
def test_framesync_one_nan_takes_exactly_its_windows(c, wn):
    y, p = fr.dense_stream(wn), fr.words()[wn]
    node = c.FrameSyncNode(p, fr.DENSE_THR, 0)
    clean, _, _ = whole(node, y)
    bad = y.copy()
    bad[NAN_AT] = NAN
    got, _, _ = whole(restart(node), bad)
    nan_free_records_survive(clean, got, np.arange(NAN_AT - p.size + 1, NAN_AT + 1), wn)


@pytest.mark.parametrize("wn", fr.DENSE_FAR_WORDS)
def test_framesync_positions_past_2_32(c, wn):
    y, p = fr.dense_stream(wn), fr.words()[wn]
    node = c.FrameSyncNode(p, fr.DENSE_THR, 0)
    model = fr.dense_detect(wn, fr.DENSE_THR)
    for r in o.FAR_RESIDUES:
        s = o.FAR_BASE + r
        near, _, near_last = whole(restart(node, s), y)
        # a word's sums do not depend on where it lies: from s on, the records of the run at 0 (test 1's model); in front of
        # s, the P - 1 positions whose words begin in the zero state
        assert near.size == y.size + p.size - 1 and int(near["index"][0]) == s - p.size + 1 and near_last.size == p.size - 1
        tail = near[p.size - 1:].copy()
        tail["index"] -= np.uint64(s)
        f_check(tail, model, f_energy(wn), "%s at %d" % (wn, s))
        for K in o.FAR_SHIFTS:
            far, _, far_last = whole(restart(node, s + K), y)
            assert far.size == near.size and far_last.size == near_last.size, (s, K)
            assert np.array_equal(far["index"], near["index"] + np.uint64(K)), (s, K)
            assert int(far_last["index"][-1]) == s + K + y.size - 1                      # the index the flush reports
            assert values(far) == values(near), (s, K)
            assert node.position() == s + K + y.size
        assert s + o.FAR_SHIFTS[0] < 1 << 32 < s + o.FAR_SHIFTS[0] + y.size


# ================================================================== the deframer behind them
def test_deframe_indices_on_both_sides_of_2_32(c):
    """Frames of 64 symbols (C32) from detections below and above 2^32, one complete in its call, one pending across a call
    boundary, one passed a call late (its first symbols come from the state): the records, and the headers but for the shift,
    are those of the same calls around 8192."""
    F, look, back = 64, 64, 100
    rng = np.random.default_rng(64)
    y = ((rng.standard_normal(700) + 1j * rng.standard_normal(700)) / np.sqrt(2)).astype(np.complex64)
    plan = [(150, (-90, 20)), (250, (30, 100, 280)), (300, (400,))]       # (symbols, detection indices relative to the base)
    frames_per_call = [1, 3, 2]

    def run(base):
        node = c.DeframeNode(F, 0, look).set_position(base - back)
        recs, heads, pend, at = [], [], [], 0
        for n, rel in plan:
            dets = np.zeros(len(rel), c.FRAME_DETECTION_DTYPE)
            for i, k in enumerate(rel):
                turn = np.exp(1j * (0.37 * k + 0.1))
                dets[i] = (base + k, 3.0 * turn.real, 3.0 * turn.imag, 0.9, 10.0)
            recs.append(node.run(y[at: at + n], dets))
            heads.append(node.headers.copy())
            pend.append(node.pending())
            at += n
            assert node.position() == base - back + at
        return recs, heads, pend

    near, far = run(8192), run(1 << 32)
    shift = np.uint64((1 << 32) - 8192)
    assert [a.shape[0] for a in near[0]] == [a.shape[0] for a in far[0]] == frames_per_call
    assert [p.size for p in far[2]] == [1, 1, 0]                           # base + 20, then base + 280, wait for the next call
    for a, ha, pa, b, hb, pb in zip(*near, *far):
        assert a.tobytes() == b.tobytes()
        for u, v in ((ha, hb), (pa, pb)):
            assert np.array_equal(v["index"], u["index"] + shift) and np.array_equal(v["start"], u["start"] + shift)
            assert all(u[f].tobytes() == v[f].tobytes() for f in ("rot_re", "rot_im", "gain", "metric"))
    idx = np.concatenate(far[1])["index"].astype(np.int64) - (1 << 32)
    assert idx.tolist() == [-90, 20, 30, 100, 280, 400]
    # and they are the frames: the symbols from the index on, turned back by the detection's angle (the f32 rotor is within
    # 2^-24 sqrt 2 of it, the f32 complex product adds less than 2^-22: together below 4e-7)
    for k, rec in zip(idx.tolist(), np.concatenate(far[0])):
        want = y[back + k: back + k + F].astype(np.complex128) * np.exp(-1j * (0.37 * k + 0.1))
        assert np.max(np.abs(rec - want)) <= 4e-7 * np.max(np.abs(want))
