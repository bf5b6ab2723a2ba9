"""The spectrum estimator (comms_spectrum_*, SpectrumNode) on the GPU against include/comms_hip.h's "spectrum estimator": the
rows against tests/spectrum_ref.py at its bounds for every size, hop and averaging count of its case table; the exactly
representable cases; and the stream contract -- a row's bits do not depend on how the stream is cut into calls, on a restore from
state, position and accumulators, on the stream index itself, or on a non-finite sample in another row."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spectrum_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def c():
    import __graft_entry__ as g

    g.build()
    import comms_rs_amd as c

    assert c.device_count() >= 1
    return c


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run_cut(node, x, cuts):
    """The rows of x fed in calls that end at `cuts` (and at len(x)), concatenated."""
    rows, at = [], 0
    for end in list(cuts) + [len(x)]:
        want = node.out_len(end - at)
        got = node.run(x[at:end])
        assert got.shape == (want, node.n_fft)
        rows.append(got)
        at = end
    return np.concatenate(rows)


# ---- accuracy ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,hop", ref.cases())
def test_rows_against_the_reference(c, n_fft, hop):
    w = c.window_taps("hann", n_fft)
    x = ref.signal(max(ref.n_samples(n_fft, hop, k) for k in ref.AVGS), 100 + n_fft + hop)
    for avg in ref.AVGS:
        xs = x[: ref.n_samples(n_fft, hop, avg)]
        node = c.SpectrumNode(n_fft, w, hop, avg)
        assert node.scale == pytest.approx(ref.psd_scale(w, avg), rel=1e-12)
        got = node.run(xs)
        P = ref.ref_rows(xs, w, hop, avg, float(np.float32(node.scale)))
        assert got.dtype == np.float32 and got.shape[0] == ref.out_len(0, len(xs), n_fft, hop, avg) >= 3
        ref.check_rows(got, P, avg, "N=%d H=%d K=%d" % (n_fft, hop, avg))
        assert node.position == len(xs)


# ---- exact cases -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft", ref.SIZES)
def test_constant_input_is_exact(c, n_fft):
    """x = 1 under a rect window: X[0] = N and every other bin a difference of equal numbers."""
    for avg, hop, order in ((1, n_fft // 2, "natural"), (3, n_fft, "centred"), (33, 3 * n_fft // 8 + 1, "natural"), (97, n_fft // 2, "centred")):
        scale = 2.0 ** -9
        node = c.SpectrumNode(n_fft, "rect", hop, avg, scale, order)
        got = node.run(np.ones(n_fft + (3 * avg - 1) * hop + hop // 2, np.complex64))
        want = np.zeros((3, n_fft), np.float32)
        want[:, n_fft // 2 if order == "centred" else 0] = avg * n_fft * n_fft * scale
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (n_fft, avg, hop, order)   # (+0, not -0)


@pytest.mark.parametrize("n_fft", ref.SIZES)
def test_segment_amplitudes_fix_the_row_assignment(c, n_fft):
    """H = N and a constant a_s in 1 .. 8 per segment: row r is exactly scale N^2 sum a_s^2 over its own K segments, in one call and
    cut inside segments, chunks and rows."""
    rng = np.random.default_rng(n_fft)
    for avg in (1, 3, 32, 33, 97):
        n_rows = 4
        a = rng.integers(1, 9, n_rows * avg + avg // 2).astype(np.float64)
        x = np.repeat(a, n_fft).astype(np.complex64)
        scale = 2.0 ** -12
        want = np.zeros((n_rows, n_fft), np.float32)
        want[:, 0] = scale * n_fft * n_fft * (a[: n_rows * avg] ** 2).reshape(n_rows, avg).sum(axis=1)
        cuts = [5 * n_fft // 2, (avg + 1) * n_fft + 3, (2 * avg + 40) * n_fft]
        for cut in ([], sorted(k for k in cuts if k < len(x))):
            got = run_cut(c.SpectrumNode(n_fft, "rect", n_fft, avg, scale), x, cut)
            assert np.array_equal(bits(got), bits(want)), (n_fft, avg, cut)


# ---- cuts ------------------------------------------------------------------------------------------------------------------------
CUT_CASES = [(64, 32, 3), (64, 25, 33), (64, 1, 65), (256, 128, 97), (512, 517, 32), (1024, 512, 3), (1024, 385, 65)]


@pytest.mark.parametrize("n_fft,hop,avg", CUT_CASES)
def test_cuts_do_not_change_the_rows(c, n_fft, hop, avg):
    w = c.window_taps("hann", n_fft)
    x = ref.signal(ref.n_samples(n_fft, hop, avg), 7)
    new = lambda: c.SpectrumNode(n_fft, w, hop, avg, order="centred")  # noqa: E731
    whole = new().run(x)
    ref.check_rows(whole, ref.ref_rows(x, w, hop, avg, float(np.float32(new().scale)), "centred"), avg, "N=%d H=%d K=%d" % (n_fft, hop, avg))
    seg_end = lambda s: s * hop + n_fft  # noqa: E731  (the call that ends here completes segment s)
    plans = {
        "at 1": [1],
        "at N - 1": [n_fft - 1],
        "at N": [n_fft],
        "inside a chunk": [seg_end(min(avg, 32) // 2) + 1],
        "at a chunk boundary": [seg_end(min(avg, 32) - 1)],
        "inside a row": [seg_end(avg + avg // 2), seg_end(2 * avg + 1) + hop // 2],
        "an empty call": [seg_end(3), seg_end(3)],
        "three calls shorter than N": [n_fft + 10, n_fft + 10 + n_fft // 3, n_fft + 10 + 2 * (n_fft // 3), n_fft + 10 + n_fft - 1],
    }
    for name, cuts in plans.items():
        got = run_cut(new(), x, cuts)
        assert np.array_equal(bits(got), bits(whole)), (name, cuts)


@pytest.mark.parametrize("n_fft,hop,avg", [(64, 25, 33), (1024, 512, 3)])
def test_run_dev_writes_its_rows_and_nothing_else(c, n_fft, hop, avg):
    x = ref.signal(ref.n_samples(n_fft, hop, avg), 8)
    whole = c.SpectrumNode(n_fft, "hann", hop, avg).run(x)
    node = c.SpectrumNode(n_fft, "hann", hop, avg)
    rows = node.out_len(len(x))
    out_bytes, guard = rows * n_fft * 4, 256
    d_in, d_out = c.DeviceBuf(x.nbytes), c.DeviceBuf(out_bytes + guard)
    d_in.upload(x)
    d_out.upload(np.full(out_bytes + guard, 0xA5, np.uint8))
    node.run_dev(d_in.ptr, len(x), d_out.ptr)
    got = d_out.download(np.uint8, out_bytes + guard)
    assert np.array_equal(got[:out_bytes].view(np.uint32).reshape(rows, n_fft), bits(whole))
    assert np.all(got[out_bytes:] == 0xA5)
    node.run_dev(d_in.ptr, 0, 0)   # an empty call launches nothing and needs no pointers
    assert node.position == len(x)


# ---- restore ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,hop,avg", [(64, 32, 3), (128, 49, 97), (1024, 512, 65), (256, 261, 33)])
def test_restore_mid_row_and_mid_chunk(c, n_fft, hop, avg):
    x = ref.signal(ref.n_samples(n_fft, hop, avg), 9)
    new = lambda: c.SpectrumNode(n_fft, "hamming", hop, avg)  # noqa: E731
    whole = new().run(x)
    stop = (avg + avg // 2 + (1 if avg > 32 else 0)) * hop + n_fft + 3   # inside row 1, and for K > 32 inside a chunk of it
    first = new()
    head = first.run(x[:stop])
    assert ref.segments_before(stop, n_fft, hop) % avg != 0
    assert avg <= 32 or (ref.segments_before(stop, n_fft, hop) % avg) % 32 != 0
    second = new()
    second.state = first.state
    second.position = first.position
    second.acc = first.acc
    assert second.position == stop and np.array_equal(bits(second.acc), bits(first.acc))
    tail = second.run(x[stop:])
    assert np.array_equal(bits(np.concatenate([head, tail])), bits(whole))
    # without the accumulators the row that was open differs, and only that one
    third = new()
    third.state, third.position = first.state, stop
    lossy = third.run(x[stop:])
    assert not np.array_equal(bits(lossy[0]), bits(tail[0])) and np.array_equal(bits(lossy[1:]), bits(tail[1:]))


# ---- set_position ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,hop,avg", [(64, 64, 3), (64, 69, 33), (128, 64, 3), (1024, 385, 65), (512, 256, 32)])
def test_rows_do_not_depend_on_the_stream_index(c, n_fft, hop, avg):
    """A handle moved to a multiple of H K at or above 2^40 starts a row with the first sample it is given, as a handle at
    position 0 does.  With H < N the segments that start before that position and end behind it are formed from the state
    (zeros here) and complete rows of their own first -- ceil((ceil(N / H) - 1) / K) of them: a shard's first rows, which a
    handle at position 0 does not have.  Every row after them carries the same bits."""
    x = ref.signal(ref.n_samples(n_fft, hop, avg), 10)
    at0 = c.SpectrumNode(n_fft, "hann", hop, avg).run(x)
    pos = -(-(1 << 40) // (hop * avg)) * (hop * avg)
    node = c.SpectrumNode(n_fft, "hann", hop, avg)
    node.position = pos
    assert node.position == pos
    straddling = -(-n_fft // hop) - 1
    extra = -(-straddling // avg)
    cut = len(x) // 2 + 1
    assert node.out_len(len(x)) == at0.shape[0] + extra
    got = np.concatenate([node.run(x[:cut]), node.run(x[cut:])])
    assert node.position == pos + len(x)
    assert got.shape[0] == at0.shape[0] + extra and np.array_equal(bits(got[extra:]), bits(at0))


# ---- non-finite input --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,hop,avg", [(64, 32, 3), (128, 49, 33), (1024, 512, 1), (512, 517, 3)])
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_a_non_finite_sample_reaches_its_rows_only(c, n_fft, hop, avg, bad):
    x = ref.signal(ref.n_samples(n_fft, hop, avg), 11)
    for window in ("hann", "blackman"):
        w = c.window_taps(window, n_fft)
        s = avg + 1                        # a segment of row 1
        for off in (0, n_fft // 3):        # hann's w[0] is 0
            t = s * hop + off
            clean, dirty = x.copy(), x.copy()
            clean[t] = 0
            dirty[t] = complex(bad, 0.0) if off else complex(0.0, bad)
            want = c.SpectrumNode(n_fft, w, hop, avg).run(clean)
            got = c.SpectrumNode(n_fft, w, hop, avg).run(dirty)
            covering = [q for q in range(ref.segments_before(len(x), n_fft, hop)) if q * hop <= t < q * hop + n_fft]
            hit = sorted({q // avg for q in covering if q // avg < want.shape[0]})
            assert 1 in hit
            for r in range(want.shape[0]):
                if r in hit:
                    assert not np.any(np.isfinite(got[r])), (window, off, r)
                else:
                    assert np.array_equal(bits(got[r]), bits(want[r])), (window, off, r)
    assert c.window_taps("hann", n_fft)[0] == 0.0


# ---- kernel names ------------------------------------------------------------------------------------------------------------------
def test_kernel_names(c):
    one = c.SpectrumNode(256, "hann", 128, 32).kernel(1 << 16)
    assert one.startswith("spectrum_kernel<256,") and "spectrum_rows_kernel" not in one and " + " not in one, one
    two = c.SpectrumNode(256, "hann", 128, 33).kernel(1 << 16)
    assert two.startswith("spectrum_kernel<256,") and two.count(" + spectrum_rows_kernel") == 1, two
    for name in (one, two):
        for key in ("wg=", "hop=128", "avg=", "chunks=", "rows=", "items=", "grid=", "max_grid=", "lds="):
            assert key in name, (key, name)
    assert "chunks=1 " in one and "chunks=2 " in two
