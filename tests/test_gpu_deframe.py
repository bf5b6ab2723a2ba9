"""GPU tests of the deframer (comms_deframe_*, deframe_kernel) against the f64 definition.  Streams, detections, call plans,
references and tolerances come from tests/deframe_ref.py; tests/test_deframe_ref.py measures on the CPU what the tolerances
rest on and checks that no decision of these inputs is within rounding of flipping.  Run with -m gpu."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import deframe_ref as dr
import framesync_ref as fr
import rx_ref
import symsync_ref
import syncest_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
FORMATS = ("c32", "bits", "llr")


@pytest.fixture(scope="module")
def c():
    import comms_rs_amd as c

    assert c.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested (no CPU fallback)"
    return c


def node_of(c, cs, fmt="c32"):
    node = c.DeframeNode(cs.F, cs.offset, cs.lookback, cs.K, None if cs.table is None else np.array(cs.table, np.complex64),
                         normalise=cs.normalise, word_energy=dr.word_energy() if cs.normalise else None)
    return node.set_output_format(fmt).set_llr_scale(cs.scale)


def run_plan(node, y, calls, dev=None):
    """The calls of a plan through run (or run_dev on the stream at `dev`): (frames of all calls, headers, frames per call)."""
    parts, heads, counts, at = [], [], [], 0
    for n, dets in calls:
        if dev is None:
            parts.append(node.run(y[at: at + n], dets))
        else:
            cap = node.frames_ready(n, dets)
            out = dev[1](max(1, cap * node.frame_bytes()))
            got = node.run_dev(dev[0] + 8 * at, n, dets, out.ptr, cap)
            assert got == cap
            parts.append(node._shape(out.download(np.uint8, cap * node.frame_bytes()), cap))
        heads.append(node.headers)
        counts.append(parts[-1].shape[0])
        at += n
    assert at == y.size
    return np.concatenate(parts), np.concatenate(heads), counts


def check_against_definition(c, idx, got, what):
    """got: {format: frames x ...} of case idx, against its reference."""
    cs = dr.cases()[idx]
    ref, _ = dr.reference(idx)
    z, values, llr = dr.joined(ref, "z"), dr.joined(ref, "values"), dr.joined(ref, "llr")
    fin = np.isfinite(z)
    assert got["c32"].shape == z.shape and np.array_equal(np.isfinite(got["c32"]), fin), (what, cs.name)
    dz = float(np.max(np.abs(got["c32"][fin] - z[fin]) / np.abs(z[fin])))
    assert np.array_equal(got["bits"], dr.records(cs, values)), (what, cs.name)             # padding bytes included
    assert got["llr"].shape == llr.shape and np.array_equal(np.isnan(got["llr"]), np.isnan(llr)), (what, cs.name)
    table = dr.table_of(cs).astype(np.complex128)
    dmax = np.max(np.abs(z[..., None] - table) ** 2, axis=-1)
    rel = np.abs(got["llr"] - llr).reshape(z.shape + (cs.K,)) / (float(np.float32(cs.scale)) * dmax)[..., None]
    dl = float(np.nanmax(rel))
    print("%s %s: %d frames, z off by %.3e of |z| (tolerance %.3e), LLR by %.3e of s max d (tolerance %.3e)"
          % (what, cs.name, z.shape[0], dz, dr.Z_TOL, dl, dr.LLR_TOL))
    assert dz <= dr.Z_TOL and dl <= dr.LLR_TOL, (what, cs.name, dz, dl)
    # the sign of every LLR is the decided bit
    bits = np.stack([np.unpackbits(r, bitorder="little")[: cs.F * cs.K] for r in got["bits"]]).reshape(-1, cs.F, cs.K)
    soft = got["llr"].reshape(-1, cs.F, cs.K)
    assert not np.any((soft > 0) & (bits == 1)) and not np.any((soft < 0) & (bits == 0)), (what, cs.name)
    # BITS is comms_sym_to_bits_dev on the node's own C32 output, frame by frame
    nb = -(-cs.F * cs.K // 8)
    tab = None if cs.table is None else np.array(cs.table, np.complex64)
    for f in sorted({0, z.shape[0] // 2, z.shape[0] - 1}):
        assert np.array_equal(c.sym_to_bits(got["c32"][f], cs.K, tab), got["bits"][f, :nb]), (what, cs.name, f)


# ------------------------------------------------------------------ 1. every case against the definition, over its call plan
@pytest.mark.parametrize("idx", range(len(dr.cases())), ids=lambda i: dr.cases()[i].name)
def test_case_against_the_definition(c, idx):
    cs = dr.cases()[idx]
    ref, left = dr.reference(idx)
    got = {}
    for fmt in FORMATS:
        node = node_of(c, cs, fmt)
        got[fmt], heads, counts = run_plan(node, cs.y, dr.calls(idx))
        assert counts == [r["index"].size for r in ref], (cs.name, fmt, counts)
        assert node.position() == cs.y.size and node.pending().size == left == 0
    check_against_definition(c, idx, got, "host")
    # the header fields: what the frame was made with
    assert np.array_equal(heads["index"].astype(np.int64), dr.joined(ref, "index")) and np.array_equal(heads["start"].astype(np.int64), dr.joined(ref, "start"))
    u, g = dr.joined(ref, "u"), dr.joined(ref, "g")
    assert np.array_equal(heads["rot_re"], u.real.astype(np.float32)) and np.array_equal(heads["rot_im"], u.imag.astype(np.float32))
    assert np.array_equal(heads["gain"], g.astype(np.float32)) and np.array_equal(heads["metric"], dr.joined(ref, "metric").astype(np.float32))
    if not cs.normalise:
        assert np.all(heads["gain"] == 1.0)


# ------------------------------------------------------------------ 2. past the grid, pointer forms, guard region
def test_more_lanes_than_one_pass_of_the_grid(c):
    idx = dr.case("past-the-grid")
    cs = dr.cases()[idx]
    d_y = c.DeviceBuf(8 * cs.y.size).upload(cs.y)                  # the input ends where its allocation ends
    for K in (2, 1):
        for fmt in FORMATS:
            node = node_of(c, cs._replace(K=K), fmt)
            name = node.kernel(300)
            assert name.startswith("deframe_kernel"), name
            k = {a: int(b) for a, b in re.findall(r"(\w+)=(\d+)", name)}
            assert k["wg"] == dr.WG and k["max_grid"] <= fr.GRID_CAP and k["lds"] == 0
            assert k["lanes"] > k["grid"] * k["wg"] and k["grid"] == k["max_grid"]       # lanes walk several items
            assert k["items"] == 300 * (node.frame_bytes() // 4 if fmt == "bits" else cs.F)
    got = {}
    for fmt in FORMATS:
        node = node_of(c, cs, fmt)
        got[fmt], _, _ = run_plan(node, cs.y, dr.calls(idx), dev=(d_y.ptr, c.DeviceBuf))
        host, _, _ = run_plan(node_of(c, cs, fmt), cs.y, dr.calls(idx))
        assert host.tobytes() == got[fmt].tobytes(), fmt               # host-pointer form == device form, bit for bit
    check_against_definition(c, idx, got, "device")


@pytest.mark.parametrize("name", ["F1-K1", "F17-K1", "F33-K2", "adjacent", "300-frames"])
def test_padding_is_zero_and_nothing_is_written_past_the_records(c, name):
    idx = dr.case(name)
    cs = dr.cases()[idx]
    d_y = c.DeviceBuf(8 * cs.y.size).upload(cs.y)
    for fmt in FORMATS:
        node = node_of(c, cs, fmt)
        want, _, _ = run_plan(node_of(c, cs, fmt), cs.y, dr.calls(idx))
        nf, fb = want.shape[0], node.frame_bytes()
        guard = 256
        out = c.DeviceBuf(nf * fb + guard).upload(np.full(nf * fb + guard, 0xA5, np.uint8))
        at = done = 0
        for n, dets in dr.calls(idx):
            done += node.run_dev(d_y.ptr + 8 * at, n, dets, out.ptr + done * fb, nf - done)
            at += n
        raw = out.download(np.uint8, nf * fb + guard)
        assert done == nf and raw[: nf * fb].tobytes() == want.tobytes(), (name, fmt)
        assert np.all(raw[nf * fb:] == 0xA5), (name, fmt)                # the guard region is untouched
        if fmt == "bits":
            nb = -(-cs.F * cs.K // 8)
            assert fb == -(-nb // 4) * 4 and not np.any(want[:, nb:])     # padding bytes ...
            tail = np.stack([np.unpackbits(r[:nb], bitorder="little")[cs.F * cs.K:] for r in want])
            assert not np.any(tail)                                       # ... and the trailing bits of the last byte


# ------------------------------------------------------------------ 3. cut invariance
@pytest.mark.parametrize("name", ["F2053-K1", "straddle", "overlap", "one-nan", "300-frames", "amp1e3-norm"])
def test_cuts_give_the_bits_of_the_uncut_stream(c, name):
    idx = dr.case(name)
    cs = dr.cases()[idx]
    dets = dr.detections(idx)
    rng = np.random.default_rng(11)
    for fmt in FORMATS:
        want, wh, _ = run_plan(node_of(c, cs, fmt), cs.y, dr.plan(cs.y, dets, []))
        for cuts in ([1], sorted(rng.integers(0, cs.y.size + 1, 9).tolist()), list(range(1, cs.y.size, max(37, cs.y.size // 40)))):
            got, gh, _ = run_plan(node_of(c, cs, fmt), cs.y, dr.plan(cs.y, dets, cuts))
            assert got.tobytes() == want.tobytes() and gh.tobytes() == wh.tobytes(), (name, fmt, cuts)


def test_a_detection_may_come_one_call_late(c):
    idx = dr.case("straddle")
    dets = dr.detections(idx)
    k = int(dets["index"][0])
    cut = k + dr.P + dr.GUARD                                          # the first call reports it; it is passed with the second
    cs = dr.cases()[idx]._replace(lookback=dr.GUARD - 1 + cut)         # a late detection reaches back by the reporting call's length as well
    want, _, _ = run_plan(node_of(c, cs, "bits"), cs.y, dr.plan(cs.y, dets, []))
    calls = [(cut, dets[:0]), (dr.GUARD - 1, dets), (cs.y.size - cut - dr.GUARD + 1, dets[:0])]
    got, _, counts = run_plan(node_of(c, cs, "bits"), cs.y, calls)
    assert got.tobytes() == want.tobytes() and sum(counts) == 1


# ------------------------------------------------------------------ 4. checkpoint
def test_checkpoint_moves_to_a_fresh_handle(c):
    idx = dr.case("three-calls")
    cs = dr.cases()[idx]
    calls = dr.calls(idx)
    for fmt in FORMATS:
        want, wh, _ = run_plan(node_of(c, cs, fmt), cs.y, calls)
        a = node_of(c, cs, fmt)
        at = 0
        for n, dets in calls[:2]:
            assert a.run(cs.y[at: at + n], dets).shape[0] == 0
            at += n
        state, pos, pend = a.state(), a.position(), a.pending()
        assert state.size == a.state_len() == max(cs.lookback, cs.F - 1) and pos == at and pend.size == 1    # in the middle of a pending frame
        assert np.array_equal(state, cs.y[:at][::-1][: state.size]) and np.array_equal(a.state(3), state[:3])   # raw symbols, newest first
        b = node_of(c, cs, fmt).set_state(state).set_position(pos).set_pending(pend)
        parts = []
        for n, dets in calls[2:]:
            parts.append(b.run(cs.y[at: at + n], dets))
            at += n
        assert np.concatenate(parts).tobytes() == want.tobytes() and b.headers.tobytes() == wh.tobytes(), fmt
    with pytest.raises(c.CommsError):                                  # complete at the position: no pending frame
        node_of(c, cs).set_position(10 ** 6).set_pending(pend)


# ------------------------------------------------------------------ 5. capacity, refusals, flush
def test_frames_ready_and_capacity(c):
    idx = dr.case("300-frames")
    cs = dr.cases()[idx]
    (n, dets), = dr.calls(idx)[:1]
    node = node_of(c, cs, "bits")
    ready = node.frames_ready(n, dets)
    assert ready == dr.reference(idx)[0][0]["index"].size > 250
    assert node.frames_ready(0, dets) < ready and node.frames_ready(n) == 0
    with pytest.raises(c.CommsError) as e:
        node.run(cs.y[:n], dets, cap=ready - 1)
    assert e.value.code == c.COMMS_ERR_ARG and "cap_frames" in str(e.value)
    assert node.position() == 0 and node.pending().size == 0 and not np.any(node.state())     # the refused call changed nothing
    want, _, _ = run_plan(node_of(c, cs, "bits"), cs.y, dr.calls(idx))
    got, _, _ = run_plan(node, cs.y, dr.calls(idx))
    assert got.tobytes() == want.tobytes()


def test_refused_detections_change_nothing(c):
    idx = dr.case("overlap")
    cs = dr.cases()[idx]
    dets = dr.detections(idx)
    assert dets.size == 2
    want, _, _ = run_plan(node_of(c, cs, "bits"), cs.y, dr.calls(idx))

    def bad(**kw):
        d = dets.copy()
        for key, (i, v) in kw.items():
            d[key][i] = v
        return d

    node = node_of(c, cs, "bits")
    cases = [("order", dets[::-1].copy(), 0), ("order", bad(index=(1, int(dets["index"][0]))), 0), ("zero", bad(corr_re=(0, 0.0), corr_im=(0, 0.0)), 0),
             ("finite", bad(corr_re=(1, np.nan)), 0), ("finite", bad(corr_im=(0, np.inf)), 0)]
    for word, d, _ in cases:
        with pytest.raises(c.CommsError) as e:
            node.run(cs.y, d)
        assert e.value.code == c.COMMS_ERR_ARG and word in str(e.value), (word, str(e.value))
        with pytest.raises(c.CommsError):
            node.frames_ready(cs.y.size, d)
        assert node.position() == 0 and node.pending().size == 0
    # stale: the payload starts more than lookback before the call
    k = int(dets["index"][0])
    first = k + cs.offset + cs.lookback + 1
    assert node.run(cs.y[:first]).shape[0] == 0
    with pytest.raises(c.CommsError) as e:
        node.run(cs.y[first:], dets)
    assert "stale" in str(e.value) and node.position() == first and node.pending().size == 0
    node.set_position(0).set_state(np.zeros(node.state_len(), np.complex64))
    got, _, _ = run_plan(node, cs.y, dr.calls(idx))                    # the handle is as good as new
    assert got.tobytes() == want.tobytes()
    # a normalising handle without the word's energy refuses its first detection
    nrm = c.DeframeNode(cs.F, cs.offset, cs.lookback, normalise=True)
    with pytest.raises(c.CommsError) as e:
        nrm.run(cs.y, dets)
    assert "energy" in str(e.value)
    lib, found = c.lib(), C.c_size_t()
    buf = c.DeviceBuf(8 * 64)
    assert lib.comms_deframe_run_dev(node._h, buf.ptr + 4, 8, None, 0, buf.ptr, 0, None, C.byref(found), None) == c.COMMS_ERR_ARG   # half a symbol off
    assert lib.comms_deframe_run_dev(node._h, buf.ptr, 8, None, 0, buf.ptr + 2, 0, None, C.byref(found), None) == c.COMMS_ERR_ARG
    assert lib.comms_deframe_set_output_format(node._h, 2) == c.COMMS_ERR_ARG
    for other in (c.SymbolSyncNode(np.ones(1, np.float32), 1, 1),):
        assert lib.comms_symsync_set_output_format(other._h, 3, 2, None) == c.COMMS_ERR_ARG       # COMMS_SYM_LLR is the deframer's alone


def test_flush_and_timer(c):
    idx = dr.case("three-calls")
    cs = dr.cases()[idx]
    node = node_of(c, cs, "llr")
    timer = c.KernelTimer(4).attach(node)
    n, dets = dr.calls(idx)[0]
    assert node.run(cs.y[:n], dets).shape[0] == 0 and node.pending().size == 1
    assert node.flush() == 1 and node.pending().size == 0 and node.position() == n and not np.any(node.state())
    assert node.flush() == 0
    assert node.run(cs.y[n:]).shape[0] == 0                              # the dropped frame does not come back
    ms = timer.read_ms()
    assert ms.size == 2 and np.all((ms > 0) & (ms < 100))
    timer.close()


# ------------------------------------------------------------------ 6. the loop it exists for
def loop_nodes(c, x, h):
    L, S = sr.LOOP_L, sr.LOOP_S
    word = fr.words()[fr.LOOP_WORD]
    est = c.SyncEstimatorNode(S, sr.LOOP_D, sr.LOOP_BETA).run(x)
    sync = c.SymbolSyncNode(h, L, S)
    sync.timing = symsync_ref.tau_from_estimate(est.timing, h.size, L, S)
    frames = c.FrameSyncNode(word, fr.LOOP_THR, word.size - 1)
    return sync, frames, word


@pytest.mark.parametrize("quarter", fr.LOOP_QUARTERS)
@pytest.mark.parametrize("dd", sr.LOOP_DD)
def test_the_loop_on_the_device(c, dd, quarter):
    """SymbolSyncNode -> FrameSyncNode -> DeframeNode (BITS) -> bit_errors against the transmitted payload, the samples never
    on the host: zero errors of 4096, with no rotation and no lag tried."""
    v, x, h = fr.loop_signal(dd, quarter)
    sync, frames, word = loop_nodes(c, x, h)
    n_sym = x.size // sr.LOOP_S
    d_x = c.DeviceBuf(8 * x.size).upload(x)
    d_y = c.DeviceBuf(8 * n_sym)
    sync.run_dev(d_x.ptr, x.size, d_y.ptr)
    deframe = c.DeframeNode(fr.LOOP_NPAY, word.size, word.size - 2).set_output_format("bits")
    d_bits, d_want = c.DeviceBuf(deframe.frame_bytes()), c.DeviceBuf(fr.LOOP_NPAY // 4)
    det = frames.run_dev(d_y.ptr, n_sym, raw=True)
    assert det.size == 1 and deframe.run_dev(d_y.ptr, n_sym, det, d_bits.ptr, 1) == 1
    d_want.upload(rx_ref.pack(v, 2))
    errs = c.bit_errors_dev(d_bits.ptr, d_want.ptr, 2 * fr.LOOP_NPAY)
    print("dd=%d quarter=%d: word at symbol %d, %d bit errors of %d" % (dd, quarter, det["index"][0], errs, 2 * fr.LOOP_NPAY))
    assert errs == 0 and 2 * fr.LOOP_NPAY == 4096


def test_the_loop_with_noise_llr_signs_are_the_bits(c):
    v, x, h = fr.loop_signal(5, 1)
    sigma = 0.35                                                       # per component of a sample; the matched filter's symbols come out near |y| = 5.7 with this much noise on each
    x = c.NoiseSource(77).awgn(x, sigma)
    sync, frames, word = loop_nodes(c, x, h)
    y = sync.run(x)
    det = frames.run(y) + frames.flush()
    assert len(det) == 1
    out = {}
    for fmt in ("bits", "llr"):
        node = c.DeframeNode(fr.LOOP_NPAY, word.size, word.size - 2, normalise=True, word_energy=2.0 * word.size).set_output_format(fmt)
        node.set_llr_scale(0.5 / sigma ** 2)
        out[fmt] = node.run(y, det)
        assert out[fmt].shape[0] == 1
    hard = (out["llr"][0] < 0).astype(np.uint8)
    assert np.all(out["llr"][0] != 0) and np.array_equal(np.packbits(hard, bitorder="little"), out["bits"][0])
    errs = rx_ref.bit_errors(out["bits"][0], rx_ref.pack(v, 2), 2 * v.size)
    print("sigma %.2f: %d bit errors of %d" % (sigma, errs, 2 * v.size))
    assert errs < 2 * v.size // 4                                      # noisy, yet a link


# ------------------------------------------------------------------ 7. host graph
def test_host_graph_nodes(c):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "comms_rs_amd", "host"), "-s"], timeout=600)
    out = subprocess.run([os.path.join(ROOT, "comms_rs_amd", "lib", "test_deframe_nodes_gpu")], capture_output=True,
                         text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all passed" in out.stdout
