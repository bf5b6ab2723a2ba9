"""GPU tests of the frame synchroniser (comms_framesync_*, framesync_kernel) against the f64 definition.  Words, streams,
references and tolerances come from tests/framesync_ref.py; tests/test_framesync_ref.py measures on the CPU what the
tolerances rest on and checks that no decision of these inputs is within rounding of flipping.  Run with -m gpu."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import framesync_ref as fr
import rx_ref
import symsync_ref
import syncest_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def c():
    import comms_rs_amd as c

    assert c.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested (no CPU fallback)"
    return c


def kernel_of(node, n):
    name = node.kernel(n)
    assert name.startswith("framesync_kernel"), name
    return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", name)}


def node_of(c, idx):
    _, wn, thr, G, _, _ = fr.cases()[idx]
    return c.FrameSyncNode(fr.words()[wn], thr, G)


def whole(node, y, dev=None):
    """One call and a flush: the structured array of all detections."""
    a = node.run(y, raw=True) if dev is None else node.run_dev(dev, y.size, raw=True)
    return np.concatenate([a, node.flush(raw=True)])


def check(got, idx, what):
    """Detections against case idx's reference: indices exactly, values within the tolerances of framesync_ref.py."""
    name, wn, thr, G, y, _ = fr.cases()[idx]
    ref = fr.reference(idx)
    p = fr.words()[wn].astype(np.complex128)
    Ep = float(np.sum(np.abs(p) ** 2))
    assert np.array_equal(got["index"].astype(np.int64), ref["index"]), (what, name, got["index"], ref["index"])
    if not got.size:
        return
    corr = got["corr_re"].astype(np.float64) + 1j * got["corr_im"].astype(np.float64)
    dm = np.max(np.abs(got["metric"] - ref["m"]))
    dc = np.max(np.abs(corr - ref["c"]) / np.sqrt(Ep * ref["e"]))
    de = np.max(np.abs(got["energy"] - ref["e"]) / ref["e"])
    print("%s %s: %d detections, metric off by %.3e (tolerance %.3e), corr by %.3e, energy by %.3e (tolerance %.3e)"
          % (what, name, got.size, dm, fr.METRIC_TOL, dc, de, fr.CORR_TOL))
    assert dm <= fr.METRIC_TOL and dc <= fr.CORR_TOL and de <= fr.CORR_TOL, (what, name, dm, dc, de)


# ------------------------------------------------------------------ 1. every case against the definition
@pytest.mark.parametrize("idx", [i for i, cs in enumerate(fr.cases()) if cs[0] != "past-the-grid"], ids=lambda i: fr.cases()[i][0])
def test_case_against_the_definition(c, idx):
    name, wn, thr, G, y, _ = fr.cases()[idx]
    node = node_of(c, idx)
    k = kernel_of(node, y.size)
    assert k["tile"] == fr.TILE and k["word"] == fr.words()[wn].size and k["guard"] == G and k["max_grid"] <= fr.GRID_CAP
    assert k["tiles"] == -(-y.size // fr.TILE)
    got = whole(node, y)
    check(got, idx, "host")
    assert node.position() == y.size
    buf = c.DeviceBuf(8 * y.size).upload(y)                       # the input ends where its allocation ends
    again = whole(node_of(c, idx), y, buf.ptr)
    assert got.tobytes() == again.tobytes()                       # host-pointer form == device form, bit for bit


# ------------------------------------------------------------------ 2. cut invariance
@pytest.mark.parametrize("name", ["w13-A", "w32-B", "w512-A", "w2-A", "tie-repeat", "one-nan"])
def test_cuts_give_the_bits_of_the_uncut_stream(c, name):
    idx = fr.case(name)
    _, wn, thr, G, y, _ = fr.cases()[idx]
    P = fr.words()[wn].size
    want = whole(node_of(c, idx), y)
    assert want.size == fr.reference(idx)["index"].size
    # the planted words sit before, across and after these cuts: [0, P) straddles the cuts at 1, 8 and 7 + P; the guard
    # window of the word at 0 or 1 ends across the cut at 7 + 2 P + G - 1; the words around TILE straddle the last two
    sizes = [1, 7, P - 1, P + G, fr.TILE - 1, fr.TILE + 1]
    node = node_of(c, idx)
    parts, at = [], 0
    while at < y.size:
        for n in sizes:
            n = min(n, y.size - at)
            parts.append(node.run(y[at: at + n], raw=True))
            assert node.found == parts[-1].size
            at += n
            if at == y.size:
                break
    parts.append(node.flush(raw=True))
    got = np.concatenate(parts)
    assert got.tobytes() == want.tobytes(), (name, got, want)
    assert node.position() == y.size


# ------------------------------------------------------------------ 3. past the grid
def test_more_tiles_than_the_persistent_grid(c):
    idx = fr.case("past-the-grid")
    _, wn, thr, G, y, _ = fr.cases()[idx]
    node = node_of(c, idx)
    k = kernel_of(node, y.size)
    assert k["tiles"] > k["grid"] == k["max_grid"]                 # workgroups walk several tiles
    buf = c.DeviceBuf(8 * y.size).upload(y)
    got = whole(node, y, buf.ptr)
    check(got, idx, "grid cap")
    assert got.size > 16                                           # more than come back with the count: the second copy
    assert whole(node_of(c, idx), y).tobytes() == got.tobytes()    # device scratch route of the host entry
    # a short call afterwards reads back only its own detections
    small = fr.case("w13-A")
    node.set_position(0)
    check(whole(node, fr.cases()[small][4]), small, "short after long")


# ------------------------------------------------------------------ 4, 5. checkpoint and shard
def test_checkpoint_moves_to_a_fresh_handle(c):
    idx = fr.case("w13-A")
    _, wn, thr, G, y, _ = fr.cases()[idx]
    P = fr.words()[wn].size
    want = whole(node_of(c, idx), y)
    for stop in (5, fr.TILE - P + 3, fr.TILE + 1):                 # inside the first word; inside the one at TILE - P; behind TILE
        a = node_of(c, idx)
        first = a.run(y[:stop], raw=True)
        state, pos = a.state(), a.position()
        assert state.size == a.state_len() == P + 2 * G - 1 and pos == stop
        keep = min(stop, state.size)
        assert np.array_equal(state[:keep], y[:stop][::-1][:keep]) and not np.any(state[keep:])   # raw symbols, newest first
        assert np.array_equal(a.state(3), state[:3])
        b = node_of(c, idx).set_state(state).set_position(pos)
        got = np.concatenate([first, b.run(y[stop:], raw=True), b.flush(raw=True)])
        assert got.tobytes() == want.tobytes(), stop


def test_shard_with_its_halo_reports_absolute_indices(c):
    idx = fr.case("w13-A")
    _, wn, thr, G, y, _ = fr.cases()[idx]
    P = fr.words()[wn].size
    H = P + 2 * G - 1
    want = whole(node_of(c, idx), y)
    t0 = fr.TILE - 3                                               # the word at TILE - P ends inside the halo, TILE's starts behind t0
    node = node_of(c, idx).set_position(t0).set_state(y[t0 - H: t0][::-1])
    got = np.concatenate([node.run(y[t0:], raw=True), node.flush(raw=True)])
    # the shard decides the positions from t0 - P - G + 1 on
    mine = want[want["index"].astype(np.int64) >= t0 - P - G + 1]
    assert mine.size == 2 and got.tobytes() == mine.tobytes()


# ------------------------------------------------------------------ 6. output capacity and pointer forms
def test_capacity_and_pointer_forms(c):
    idx = fr.case("w2-A")                                          # many detections: every pair (a, -a) of the payload
    _, wn, thr, G, y, _ = fr.cases()[idx]
    want = whole(node_of(c, idx), y)
    n_run = node_of(c, idx).run(y, raw=True).size
    assert n_run > 100
    node = node_of(c, idx)
    got = node.run(y, cap=5, raw=True)
    assert got.size == 5 and node.found == n_run and got.tobytes() == want[:5].tobytes()     # the lowest indices, the true count
    node = node_of(c, idx)
    assert node.run(y, cap=0, raw=True).size == 0 and node.found == n_run                    # NULL out, cap 0: counts only
    lib, found = c.lib(), C.c_size_t()
    buf = c.DeviceBuf(8 * (y.size + 1))
    assert buf.ptr % 16 == 0
    buf.upload(np.concatenate([np.full(1, 1e6 + 1e6j, np.complex64), y]))                   # the symbol in front must not be read
    node = node_of(c, idx)
    assert lib.comms_framesync_run_dev(node._h, buf.ptr + 8, y.size, None, 0, C.byref(found), None) == 0 and found.value == n_run
    node = node_of(c, idx)
    off = np.concatenate([node.run_dev(buf.ptr + 8, y.size, raw=True), node.flush(raw=True)])
    assert off.tobytes() == want.tobytes()
    assert node.run(y[:0], raw=True).size == 0 and node.position() == y.size                 # n == 0 changes nothing


# ------------------------------------------------------------------ 7. threshold
def test_threshold_changes_between_calls(c):
    idx = fr.case("w13-A")
    _, wn, thr, G, y, _ = fr.cases()[idx]
    w = fr.words()[wn]
    want = whole(node_of(c, idx), y)
    cut = 1000
    node = c.FrameSyncNode(w, 1.0, G)                              # nothing in a noisy stream reaches 1
    assert node.run(y[:cut], raw=True).size == 0
    node.set_threshold(thr)                                        # the history is raw symbols: nothing to recompute
    got = np.concatenate([node.run(y[cut:], raw=True), node.flush(raw=True)])
    # positions up to cut - P - G were decided at the old threshold; the rest at the new one
    mine = want[want["index"].astype(np.int64) > cut - w.size - G]
    assert mine.size == 2 and got.tobytes() == mine.tobytes()
    with pytest.raises(c.CommsError):
        node.set_threshold(0.0)


# ------------------------------------------------------------------ 8. argument errors
def test_arguments(c):
    from test_framesync_ref import BAD_CREATE, create_args

    lib = c.lib()
    for names, kw in BAD_CREATE:
        h = C.c_void_p()
        ptr, n, thr, guard = create_args(**kw)
        assert lib.comms_framesync_create(ptr, n, thr, guard, 0, C.byref(h)) == c.COMMS_ERR_ARG and not h, kw
        assert names in lib.comms_last_error().decode(), (kw, lib.comms_last_error())
    node = c.FrameSyncNode(fr.words()["qpsk512"], 1.0, 512)       # the limits themselves are accepted
    timer = c.KernelTimer(4).attach(node)
    buf = c.DeviceBuf(8 * 4096)
    out = np.zeros(4, c.FRAME_DETECTION_DTYPE)
    po, found = out.ctypes.data_as(C.c_void_p), C.c_size_t()
    assert lib.comms_framesync_run_dev(node._h, buf.ptr + 4, 8, po, 4, C.byref(found), None) == c.COMMS_ERR_ARG   # half a symbol off
    assert "d_in" in lib.comms_last_error().decode()
    assert lib.comms_framesync_run_dev(node._h, None, 8, po, 4, C.byref(found), None) == c.COMMS_ERR_ARG
    assert lib.comms_framesync_run_dev(node._h, buf.ptr, 8, None, 4, C.byref(found), None) == c.COMMS_ERR_ARG
    assert "out" in lib.comms_last_error().decode()
    assert lib.comms_framesync_run_dev(node._h, buf.ptr, 8, po, 4, None, None) == c.COMMS_ERR_ARG
    assert lib.comms_framesync_set_threshold(node._h, 1.5) == c.COMMS_ERR_ARG and "threshold" in lib.comms_last_error().decode()
    st = np.zeros(node.state_len() + 1, np.complex64)
    assert lib.comms_framesync_set_state(node._h, st.ctypes.data_as(C.c_void_p), st.size - 1) == 0
    assert lib.comms_framesync_set_state(node._h, st.ctypes.data_as(C.c_void_p), st.size) == c.COMMS_ERR_ARG
    assert lib.comms_framesync_get_state(node._h, st.ctypes.data_as(C.c_void_p), st.size) == c.COMMS_ERR_ARG
    assert node.position() == 0 and timer.read_ms().size == 0     # none of the refused calls touched the node
    node.run(np.zeros(4096, np.complex64))
    ms = timer.read_ms()
    assert ms.size == 1 and 0 < ms[0] < 100
    timer.close()


# ------------------------------------------------------------------ 9. the loop it exists for, nothing searched
@pytest.mark.parametrize("quarter", fr.LOOP_QUARTERS)
@pytest.mark.parametrize("dd", sr.LOOP_DD)
def test_the_loop_on_the_device(c, dd, quarter):
    """SyncEstimatorNode -> tau -> SymbolSyncNode symbols -> FrameSyncNode -> MixerNode at -arg(corr) on the payload from
    index + P -> sym_to_bits -> bit_errors against the transmitted payload: zero, with no rotation and no lag tried
    (tests/test_framesync_ref.py: so has the reference chain)."""
    L, S = sr.LOOP_L, sr.LOOP_S
    v, x, h = fr.loop_signal(dd, quarter)
    word = fr.words()[fr.LOOP_WORD]
    est = c.SyncEstimatorNode(S, sr.LOOP_D, sr.LOOP_BETA).run(x)
    sync = c.SymbolSyncNode(h, L, S)
    sync.timing = symsync_ref.tau_from_estimate(est.timing, h.size, L, S)
    n_sym = x.size // S
    d_x = c.DeviceBuf(8 * x.size).upload(x)
    d_y = c.DeviceBuf(8 * n_sym)
    sync.run_dev(d_x.ptr, x.size, d_y.ptr)                         # symbols stay on the device (null stream throughout)
    frames = c.FrameSyncNode(word, fr.LOOP_THR, word.size - 1)
    det = frames.run_dev(d_y.ptr, n_sym) + frames.flush()
    assert len(det) == 1, det
    d = det[0]
    first = d.index + word.size
    assert first + fr.LOOP_NPAY <= n_sym
    d_pay, d_bits, d_want = c.DeviceBuf(8 * fr.LOOP_NPAY), c.DeviceBuf(fr.LOOP_NPAY // 4), c.DeviceBuf(fr.LOOP_NPAY // 4)
    c.MixerNode(0.0, -d.phase).run_dev(d_y.ptr + 8 * first, fr.LOOP_NPAY, d_pay.ptr)
    c.sym_to_bits_dev(d_pay.ptr, fr.LOOP_NPAY, 2, d_bits.ptr)
    d_want.upload(rx_ref.pack(v, 2))
    errs = c.bit_errors_dev(d_bits.ptr, d_want.ptr, 2 * fr.LOOP_NPAY)
    print("dd=%d quarter=%d: word at symbol %d, metric %.4f, rotation %+.4f rad, %d bit errors of %d"
          % (dd, quarter, d.index, d.metric, d.phase, errs, 2 * fr.LOOP_NPAY))
    assert errs == 0 and d.metric > 0.9


# ------------------------------------------------------------------ 10. host graph
def test_host_graph_nodes(c):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "comms_rs_amd", "host"), "-s"], timeout=600)
    out = subprocess.run([os.path.join(ROOT, "comms_rs_amd", "lib", "test_framesync_nodes_gpu")], capture_output=True,
                         text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all passed" in out.stdout
