"""GPU tests of the OFDM synchroniser (comms_ofdmsync_*, ofdmsync_detect_kernel and ofdmsync_correct_kernel) against the f64
definition.  Streams, references and bounds come from tests/ofdmsync_ref.py; tests/test_ofdmsync_ref.py measures on the CPU
what the bounds rest on and checks that no decision of these inputs is within rounding of flipping.  Run with -m gpu."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ofdm_ref as r
import ofdmsync_ref as o
import symmap_ref as sm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def c():
    import comms_rs_amd as c

    assert c.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested (no CPU fallback)"
    return c


def kernel_of(node, n):
    name = node.kernel(n)
    assert name.startswith("ofdmsync_detect_kernel"), name
    return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", name)}


def node_of(c, cs, n_frame=0):
    return c.OfdmSyncNode(cs.L, cs.W, cs.thr, cs.G, advance=cs.A, n_frame=n_frame)


def joined(parts):
    """[(detections, cfo), ...] -> one structured array and one cfo array."""
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def whole(node, x, dev=None):
    """One call and a flush."""
    a = node.run(x, raw=True) if dev is None else node.run_dev(dev, x.size, raw=True)
    return joined([a, node.flush(raw=True)])


def check(got, cfo, ref, L, what):
    """Detections against the reference's: indices exactly, corr and energy within METRIC_BOUND of R, the metric within
    METRIC_BOUND, cfo within the image of that bound through atan2 / L."""
    assert np.array_equal(got["index"].astype(np.int64), ref["index"]), (what, got["index"], ref["index"])
    if not got.size:
        return
    corr = got["corr_re"].astype(np.float64) + 1j * got["corr_im"].astype(np.float64)
    dc = np.max(np.abs(corr - ref["P"]) / ref["R"])
    de = np.max(np.abs(got["energy"] - ref["R"]) / ref["R"])
    dm = np.max(np.abs(got["metric"] - ref["m"]))
    reach = np.arcsin(np.minimum(1.0, o.METRIC_BOUND * ref["R"] / np.abs(ref["P"]))) / L
    dw = np.abs(cfo - o.ref_cfo(ref["P"], L))
    print("%s: %d detections, corr off by %.3e, energy by %.3e, metric by %.3e (bound %.3e), cfo by %.3e (bound %.3e)"
          % (what, got.size, dc, de, dm, o.METRIC_BOUND, dw.max(), reach.min()))
    assert dc <= o.METRIC_BOUND and de <= o.METRIC_BOUND and dm <= o.METRIC_BOUND and np.all(dw <= reach + 1e-15), what
    # cfo is atan2 of the returned corr in f64, over L (two libraries' atan2 may differ in the last place: |atan2| <= pi)
    assert np.all(np.abs(cfo - np.arctan2(got["corr_im"].astype(np.float64), got["corr_re"].astype(np.float64)) / L) <= 1e-15 / L)


# ------------------------------------------------------------------ 1. every case against the definition
@pytest.mark.parametrize("name", [cs.name for cs in o.cases()])
def test_case_against_the_definition(c, name):
    cs = o.case(name)
    node = node_of(c, cs)
    k = kernel_of(node, cs.x.size)
    assert k["tile"] == o.TILE and k["lag"] == cs.L and k["window"] == cs.W and k["guard"] == cs.G and k["lds"] <= 160 * 1024
    assert k["tiles"] == k["grid"] == -(-cs.x.size // o.TILE)
    got, cfo = whole(node, cs.x)
    check(got, cfo, o.reference(name), cs.L, name)
    assert node.position() == cs.x.size
    buf = c.DeviceBuf(8 * cs.x.size).upload(cs.x)                 # the input ends where its allocation ends
    again, cfo2 = whole(node_of(c, cs), cs.x, buf.ptr)
    assert got.tobytes() == again.tobytes() and cfo.tobytes() == cfo2.tobytes()      # host-pointer form == device form, bit for bit


# ------------------------------------------------------------------ 2. cut invariance
@pytest.mark.parametrize("name", [cs.name for cs in o.cases()])
def test_cuts_give_the_bits_of_the_uncut_stream(c, name):
    cs = o.case(name)
    want, want_cfo = whole(node_of(c, cs), cs.x)
    tile = kernel_of(node_of(c, cs), 1)["tile"]
    rng = np.random.default_rng(31)
    for sizes in ([tile, tile + 1, 7, 1], [1, 7, tile + 1, tile], [int(v) for v in rng.integers(1, 3 * tile, 64)]):
        node = node_of(c, cs)
        parts, at, i = [], 0, 0
        while at < cs.x.size:
            n = min(sizes[i % len(sizes)], cs.x.size - at)
            parts.append(node.run(cs.x[at: at + n], raw=True))
            assert node.found == parts[-1][0].size
            at, i = at + n, i + 1
        parts.append(node.flush(raw=True))
        got, cfo = joined(parts)
        assert got.tobytes() == want.tobytes() and cfo.tobytes() == want_cfo.tobytes(), (name, sizes[:4])
        assert node.position() == cs.x.size


@pytest.mark.parametrize("name", [cs.name for cs in o.cases()])
def test_single_sample_calls_across_a_peak_and_its_decision(c, name):
    """Calls of one sample decide one position each (n < G + 1: a list of one entry, and all of the tile but its first
    position lies past n).  Two stretches of them: while the second frame's peak enters the stream, and while the samples
    arrive that decide the positions around it -- the peak d is decided by the call that brings sample d + W + L + G - 1."""
    cs = o.case(name)
    want, want_cfo = whole(node_of(c, cs), cs.x)
    peaks = [int(v) for v in o.reference(name)["d"]]
    d, reach = peaks[1], cs.W + cs.L + cs.G - 1
    assert 24 < d and d + reach + 48 < cs.x.size
    alone = set(range(d - 24, d + 24)) | set(range(d + reach - 48, d + reach + 48))      # the samples that come alone
    cuts = sorted({0, cs.x.size} | alone | {t + 1 for t in alone})
    node = node_of(c, cs)
    parts, decided_alone = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        parts.append(node.run(cs.x[a:b], raw=True))
        assert node.found == parts[-1][0].size
        if b - a == 1:       # sample a decides position a - reach alone: a detection exactly where the reference has a peak
            assert node.found == ((a - reach) in peaks), (name, a)
            decided_alone.append(a - reach)
    assert d in decided_alone and len(decided_alone) >= 96
    parts.append(node.flush(raw=True))
    got, cfo = joined(parts)
    assert got.tobytes() == want.tobytes() and cfo.tobytes() == want_cfo.tobytes(), name
    assert node.position() == cs.x.size


def test_capacity_returns_the_lowest_indices_and_the_true_count(c):
    cs = o.case("prefix64")
    want, want_cfo = node_of(c, cs).run(cs.x, raw=True)
    assert want.size > 10
    node = node_of(c, cs)
    got, cfo = node.run(cs.x, cap=5, raw=True)
    assert got.size == 5 and node.found == want.size and got.tobytes() == want[:5].tobytes() and cfo.tobytes() == want_cfo[:5].tobytes()
    node = node_of(c, cs)
    assert node.run(cs.x, cap=0, raw=True)[0].size == 0 and node.found == want.size       # NULL out, cap 0: counts only
    assert node.run(cs.x[:0], raw=True)[0].size == 0 and node.position() == cs.x.size     # n == 0 changes nothing


# ------------------------------------------------------------------ 3. tile seams
def test_tile_seams_and_a_ragged_last_tile(c):
    x, starts = o.seam_stream()
    node = c.OfdmSyncNode(80, 80, 0.5, 40, advance=8)
    k = kernel_of(node, x.size)
    assert k["tiles"] == k["grid"] == 513 and x.size % o.TILE == 3
    first = o.TILE - (80 + 80 + 40) + 1                            # the first position tile 1 decides
    assert [int(s) - first for s in starts[:3]] == [-1, 2 * o.TILE, 4 * o.TILE + 1]
    buf = c.DeviceBuf(8 * x.size).upload(x)
    got, cfo = whole(node, x, buf.ptr)
    ref = o.ref_detect(x, 80, 80, 40, 8, 0.5)
    assert np.array_equal(ref["d"], starts)
    check(got, cfo, ref, 80, "seams")


# ------------------------------------------------------------------ 4. NaN, silence, flush
def test_nan_silence_and_flush(c):
    cs = o.case("sym80")
    clean = o.reference("sym80")
    x = cs.x.copy()
    at = int(clean["d"][1]) + 30                                   # inside the second frame's first training symbol
    x[at] = np.nan
    ref = o.ref_detect(x, cs.L, cs.W, cs.G, cs.A, cs.thr)
    got, cfo = whole(node_of(c, cs), x)
    check(got, cfo, ref, cs.L, "one NaN")
    reach = (got["index"].astype(np.int64) + cs.A > at - (cs.W + cs.L + cs.G)) & (got["index"].astype(np.int64) + cs.A <= at + cs.G)
    assert not reach.any()                                         # no detection whose window or guard holds the NaN
    far = clean[(clean["d"] + cs.W + cs.L + cs.G <= at) | (clean["d"] - cs.G > at)]
    assert far.size == clean.size - 1 and set(far["index"]) <= set(got["index"].astype(np.int64))
    assert whole(node_of(c, cs), np.zeros(5000, np.complex64))[0].size == 0
    # a frame whose guard window ends after the stream: reported by flush, and by nothing afterwards
    d = int(clean["d"][-1])
    cut = o.late_cut()                                             # one sample short of the call that reports it
    assert cut == d + cs.W + cs.L + cs.G - 1
    node = node_of(c, cs)
    early, early_cfo = node.run(cs.x[:cut], raw=True)
    assert early.size == clean.size - 1
    late, late_cfo = node.flush(raw=True)
    assert late.size == 1 and int(late["index"][0]) == d - cs.A and node.position() == cut
    ref_cut = o.ref_detect(cs.x[:cut], cs.L, cs.W, cs.G, cs.A, cs.thr)
    check(np.concatenate([early, late]), np.concatenate([early_cfo, late_cfo]), ref_cut, cs.L, "flush")
    after = joined([node.run(cs.x[cut:], raw=True), node.flush(raw=True)])[0]
    assert not np.any(after["index"].astype(np.int64) < cut)       # no index below the flush is reported again


# ------------------------------------------------------------------ 5. checkpoint
def test_checkpoint_moves_to_a_fresh_handle(c):
    cs = o.case("sym80")
    want, want_cfo = whole(node_of(c, cs), cs.x)
    H = cs.W + cs.L + 2 * cs.G - 1
    for stop in (5, int(o.reference("sym80")["d"][1]) + 100, o.TILE + 1):
        a = node_of(c, cs)
        first = a.run(cs.x[:stop], raw=True)
        state, pos = a.state(), a.position()
        assert state.size == a.state_len() == H and pos == stop
        keep = min(stop, H)
        assert np.array_equal(state[:keep], cs.x[:stop][::-1][:keep]) and not np.any(state[keep:])   # raw samples, newest first
        b = node_of(c, cs).set_state(state).set_position(pos)
        got, cfo = joined([first, b.run(cs.x[stop:], raw=True), b.flush(raw=True)])
        assert got.tobytes() == want.tobytes() and cfo.tobytes() == want_cfo.tobytes(), stop


# ------------------------------------------------------------------ 6. argument checks and the timer
def test_arguments_and_timer(c):
    from test_ofdmsync_ref import BAD_CREATE, LIMITS, create_args

    lib = c.lib()
    for names, kw in BAD_CREATE:
        h = C.c_void_p()
        assert lib.comms_ofdmsync_create(*create_args(**kw), 0, C.byref(h)) == c.COMMS_ERR_ARG and not h, kw
        assert names in lib.comms_last_error().decode(), (kw, lib.comms_last_error())
    for kw in LIMITS:                                              # the limits themselves are accepted, and run
        lag, window, thr, guard, adv, n_frame = create_args(**kw)
        node = c.OfdmSyncNode(lag, window, thr, guard, advance=adv, n_frame=n_frame)
        assert node.run(np.zeros(3000, np.complex64))[0] == [] and kernel_of(node, 3000)["lds"] <= 160 * 1024
    node = c.OfdmSyncNode(80, 80, 0.5, 40)                         # n_frame = 0: no correct stage
    buf = c.DeviceBuf(8 * 4096)
    w = np.zeros(1)
    pw = w.ctypes.data_as(C.c_void_p)
    assert lib.comms_ofdmsync_correct_run_dev(node._h, buf.ptr, 1, pw, buf.ptr + 2048, None) == c.COMMS_ERR_ARG
    assert "n_frame" in lib.comms_last_error().decode()
    node = c.OfdmSyncNode(80, 80, 0.5, 40, advance=8, n_frame=64)
    timer = c.KernelTimer(4).attach(node)
    out = np.zeros(4, c.FRAME_DETECTION_DTYPE)
    po, found = out.ctypes.data_as(C.c_void_p), C.c_size_t()
    assert lib.comms_ofdmsync_run_dev(node._h, buf.ptr + 4, 8, po, None, 4, C.byref(found), None) == c.COMMS_ERR_ARG   # half a sample off
    assert "d_in" in lib.comms_last_error().decode()
    assert lib.comms_ofdmsync_run_dev(node._h, None, 8, po, None, 4, C.byref(found), None) == c.COMMS_ERR_ARG
    assert lib.comms_ofdmsync_run_dev(node._h, buf.ptr, 8, None, None, 4, C.byref(found), None) == c.COMMS_ERR_ARG
    assert lib.comms_ofdmsync_run_dev(node._h, buf.ptr, 8, po, None, 4, None, None) == c.COMMS_ERR_ARG
    assert lib.comms_ofdmsync_set_threshold(node._h, 1.5) == c.COMMS_ERR_ARG and "threshold" in lib.comms_last_error().decode()
    st = np.zeros(node.state_len() + 1, np.complex64)
    assert lib.comms_ofdmsync_set_state(node._h, st.ctypes.data_as(C.c_void_p), st.size - 1) == 0
    assert lib.comms_ofdmsync_set_state(node._h, st.ctypes.data_as(C.c_void_p), st.size) == c.COMMS_ERR_ARG
    assert lib.comms_ofdmsync_get_state(node._h, st.ctypes.data_as(C.c_void_p), st.size) == c.COMMS_ERR_ARG
    # the correct stage's shell: alignment, overlap (in place on the device is an overlap), NULL, a missing cfo table
    assert lib.comms_ofdmsync_correct_run_dev(node._h, buf.ptr + 8, 1, pw, buf.ptr + 2048, None) == c.COMMS_ERR_ARG
    assert lib.comms_ofdmsync_correct_run_dev(node._h, buf.ptr, 1, pw, buf.ptr, None) == c.COMMS_ERR_ARG
    assert lib.comms_ofdmsync_correct_run_dev(node._h, buf.ptr, 2, pw, buf.ptr + 8 * 64 + 16, None) == c.COMMS_ERR_ARG
    assert lib.comms_ofdmsync_correct_run_dev(node._h, None, 1, pw, buf.ptr, None) == c.COMMS_ERR_ARG
    assert lib.comms_ofdmsync_correct_run_dev(node._h, buf.ptr, 1, None, buf.ptr + 2048, None) == c.COMMS_ERR_ARG
    assert lib.comms_ofdmsync_correct_run_dev(node._h, None, 0, None, None, None) == c.COMMS_OK
    assert node.position() == 0 and timer.read_ms().size == 0     # none of the refused calls touched the node
    node.run(np.zeros(4096, np.complex64))
    node.correct(np.ones((3, 64), np.complex64), np.zeros(3))
    ms = timer.read_ms()
    assert ms.size == 2 and np.all(ms > 0) and np.all(ms < 100)    # both kernels
    timer.close()


# ------------------------------------------------------------------ 7. the correct stage
@pytest.mark.parametrize("F,n_frames", o.CORRECT_SHAPES)
def test_correct_stage(c, F, n_frames):
    x, cfo = o.correct_input(F, n_frames)
    want = o.ref_correct(x, cfo)
    node = c.OfdmSyncNode(80, 80, 0.5, 40, n_frame=F)
    got = node.correct(x, cfo)
    dist = o.correct_distance(got, want, x)
    print("records of %d x %d: %.3e from ref_correct (bound %.3e)" % (F, n_frames, dist, o.CORRECT_BOUND))
    assert dist <= o.CORRECT_BOUND
    assert np.array_equal(node.correct(x, np.zeros(n_frames)), x)                  # cfo = 0 is the identity
    # the device form: the same bits, nothing past n_frames records, and a record does not depend on its place in the call
    pad = 64
    d_in = c.DeviceBuf(x.nbytes).upload(x)
    d_out = c.DeviceBuf(x.nbytes + 8 * pad).upload(np.full(x.size + pad, np.nan + 1j * np.nan, np.complex64))
    node.correct_dev(d_in.ptr, n_frames, cfo, d_out.ptr)
    back = d_out.download(np.complex64, x.size + pad)
    assert back[: x.size].tobytes() == got.tobytes() and np.all(np.isnan(back[x.size:].real))
    if n_frames > 1:
        assert node.correct(x[-1:], cfo[-1:]).tobytes() == got[-1:].tobytes()
    # a non-finite cfo is refused and the output stays at its preset
    bad = cfo.copy()
    bad[-1] = np.inf
    d_out.upload(np.full(x.size + pad, np.nan + 1j * np.nan, np.complex64))
    with pytest.raises(c.CommsError) as e:
        node.correct_dev(d_in.ptr, n_frames, bad, d_out.ptr)
    assert e.value.code == c.COMMS_ERR_ARG and np.all(np.isnan(d_out.download(np.complex64, x.size + pad).real))
    if F <= 1280:                                                  # the host-pointer form works in place
        y = x.copy()
        w = np.ascontiguousarray(cfo)
        p = y.ctypes.data_as(C.c_void_p)
        assert c.lib().comms_ofdmsync_correct_run(node._h, p, n_frames, w.ctypes.data_as(C.c_void_p), p) == c.COMMS_OK
        assert y.tobytes() == got.tobytes()


# ------------------------------------------------------------------ 8. the link
def test_link_needs_the_correction(c):
    """CRC-24 -> K = 7 rate 3/4 -> 16-QAM -> OfdmModNode -> 12 frames at random gaps, three-tap channel, CFO, noise, fed in three
    uneven calls -> OfdmSyncNode -> DeframeNode (C32) -> correct -> OfdmDemodNode (cpe) -> DemapNode -> RateDematchNode ->
    ViterbiNode -> CrcCheckNode: every frame found, every CRC good, the payload bits exact.  The same records without
    correct() fail their CRCs."""
    f, fmt = o.link_format(), o.link_ofdm()
    p, frames = f["p"], o.LINK_FRAMES
    payload, framed, coded, sent, sym = o.link_transmit()
    table = c.qam_table(o.LINK_M)
    att = c.CrcAttachNode(p.W, p.poly, p.init, p.xorout, f["T"])
    enc = c.ConvEncoderNode(f["info"])
    match = c.RateMatchNode(f["N"], f["pattern"])
    mapper = c.SymbolMapNode(o.LINK_M, table, f["E"])
    args, kw = fmt.node_args()
    mod, dem = c.OfdmModNode(*args, **kw), c.OfdmDemodNode(*args, **kw)
    assert match.n_tx_bits == f["E"] and mapper.out_frame_syms == mod.data_syms == f["F"]
    tx = mod.run(mapper.run(match.run(enc.run(att.run(sm.pack_records(payload))))))
    want_tx = r.ref_mod(fmt, sym)
    assert tx.shape == (frames, fmt.frame_samples) and np.max(np.abs(tx - want_tx)) <= 1e-5 * np.max(np.abs(want_tx))
    x, starts = o.link_stream(tx)
    # receive, in three uneven calls
    sync = c.OfdmSyncNode.for_format(dem, o.LINK_THRESHOLD, o.LINK_GUARD, advance=o.LINK_ADVANCE)
    assert (sync.lag, sync.window, sync.n_frame) == (80, 80, fmt.frame_samples)
    deframe = c.DeframeNode(fmt.frame_samples, 0, sync.lookback)
    cuts = [0] + [int(v * x.size) for v in o.LINK_CUTS] + [x.size]
    records, cfos, indices, known = [], [], [], {}
    for a, b in zip(cuts[:-1], cuts[1:]):
        dets, cfo = sync.run(x[a:b], raw=True)
        known.update(zip(dets["index"].tolist(), cfo.tolist()))
        got = deframe.run(x[a:b], dets)
        records.append(got)
        indices += deframe.headers["index"].tolist()
    assert sync.flush()[0] == [] and deframe.flush() == 0
    records = np.concatenate(records)
    cfos = np.array([known[i] for i in indices])
    assert len(indices) == frames and np.all(np.array(indices) <= starts) and np.all(starts - np.array(indices) <= o.LINK_ADVANCE)
    assert np.max(np.abs(cfos - o.LINK_EPS)) < 0.02 * o.LINK_EPS
    demap = c.DemapNode(o.LINK_M, table, f["F"]).set_output_format("llr").set_llr_scale(o.LINK_LLR_SCALE)
    dematch = c.RateDematchNode(f["N"], f["pattern"], record_llrs=f["F"] * o.LINK_M)
    dec = c.ViterbiNode(f["info"], qscale=o.LINK_QSCALE)
    chk = c.CrcCheckNode(p.W, p.poly, p.init, p.xorout, f["T"])

    def behind(recs):
        return chk.run(dec.run(dematch.run(demap.run(dem.run(recs)))))

    got, passed, _ = behind(sync.correct(records, cfos))
    assert passed.all() and chk.n_failed == 0
    assert np.array_equal(sm.unpack_records(got, f["T"]), payload)
    _, passed_raw, _ = behind(records)
    print("without correct() %d of %d frames pass" % (int(passed_raw.sum()), frames))
    assert not passed_raw.all() and chk.n_failed >= 1


# ------------------------------------------------------------------ the C++ host nodes
def test_host_graph_nodes(c):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "comms_rs_amd", "host"), "-s"], timeout=600)
    out = subprocess.run([os.path.join(ROOT, "comms_rs_amd", "lib", "test_ofdmsync_nodes_gpu")], capture_output=True, text=True, timeout=300,
                         cwd=ROOT)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all passed" in out.stdout
