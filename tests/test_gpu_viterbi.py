"""GPU tests of the convolutional encoder and the Viterbi decoder (comms_convenc_*, comms_viterbi_*; conv_encode_kernel,
viterbi_kernel) against tests/viterbi_ref.py.  The decisions are integer arithmetic, so bits and final metrics are compared
exactly; tests/test_viterbi_ref.py checks the reference itself and pins the noisy point of the loop.  Run with -m gpu."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import viterbi_ref as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
GUARD = 256
CODES = [(K, n, t) for K in (3, 4, 5, 6, 7) for n in (2, 3) for t in (True, False)]
GEN_SETS = [pytest.param(K, n, name, id="%d-%d-%s" % (K, n, name)) for (K, n), sets in sorted(vr.GEN_CORNERS.items()) for name, _ in sets]


@pytest.fixture(scope="module")
def c():
    import comms_rs_amd as c

    assert c.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested (no CPU fallback)"
    return c


def decoder_of(c, cs):
    return c.ViterbiNode(cs.T, cs.K, cs.gens, terminated=cs.terminated, record_llrs=cs.record_llrs, qscale=cs.qscale)


def fields(name):
    return {a: int(b) for a, b in re.findall(r"(\w+)=(\d+)", name)}


def decode_dev(c, node, llr):
    """run_dev on uploaded records into a 0xFF-filled buffer with a guard region behind it: (records, metrics)."""
    frames = llr.shape[0]
    fb = node.out_frame_bytes
    d_llr = c.DeviceBuf(llr.nbytes).upload(llr)
    d_bits = c.DeviceBuf(frames * fb + GUARD).upload(np.full(frames * fb + GUARD, 0xFF, np.uint8))
    d_met = c.DeviceBuf(4 * frames + GUARD).upload(np.full(4 * frames + GUARD, 0xFF, np.uint8))
    node.run_dev(d_llr.ptr, frames, d_bits.ptr, d_met.ptr)
    raw = d_bits.download(np.uint8, frames * fb + GUARD)
    met = d_met.download(np.uint8, 4 * frames + GUARD)
    assert np.all(raw[frames * fb:] == 0xFF) and np.all(met[4 * frames:] == 0xFF), "the guard region was written"
    return raw[: frames * fb].reshape(frames, fb), met[: 4 * frames].view(np.int32)


def check_case(c, cs, node=None):
    sent, llr, bits, metric = vr.case_data(cs)
    node = decoder_of(c, cs) if node is None else node
    assert node.in_frame_bytes == 4 * cs.record_llrs and node.out_frame_bytes == vr.record_bytes(cs.T)
    got, met = decode_dev(c, node, llr)
    want = vr.pack_records(bits)                                           # padding bits and bytes 0
    assert np.array_equal(met, metric), (cs, met[:4], metric[:4])
    assert np.array_equal(got, want), (cs, int(np.count_nonzero(vr.unpack_records(got, cs.T) != bits)))
    return node


# ------------------------------------------------------------------ 1. decoder: every code, termination, seam and input
@pytest.mark.parametrize("K,n,terminated", CODES)
def test_decoder_is_the_reference_bit_for_bit(c, K, n, terminated):
    for i, steps in enumerate(vr.step_counts(K)):
        if terminated and steps < K:
            continue                                                        # T = steps - (K - 1) >= 1
        kind = vr.KINDS[(i + K + n) % len(vr.KINDS)] if steps not in (1000, vr.LDS_STEPS, vr.LDS_STEPS + 1) else "noisy"
        cs = vr.make_case(K, n, terminated, steps, 1 + i % 3, kind)
        node = check_case(c, cs)
        k = node.kernel(cs.frames)
        assert k.startswith("viterbi_kernel<%d,%s>" % (n, "lds" if steps <= vr.LDS_STEPS else "workspace")), k
        assert fields(k)["seam"] == vr.LDS_STEPS and fields(k)["waves"] == vr.WAVES and fields(k)["steps"] == steps


@pytest.mark.parametrize("kind", vr.KINDS)
@pytest.mark.parametrize("K,n,terminated", [(7, 2, True), (5, 3, False), (3, 2, False), (7, 3, True)])
def test_every_input_kind(c, K, n, terminated, kind):
    """Noise in which the reference itself errs, all ties, NaN / inf / huge values, and records longer than n * steps with NaN
    in the unused part -- at a block seam, inside a block and in the workspace form."""
    for steps in (65, 128, 300, vr.LDS_STEPS + 1):
        check_case(c, vr.make_case(K, n, terminated, steps, 3, kind))
    if kind == "special":                                                  # the same with a scale that moves the clamp
        check_case(c, vr.make_case(K, n, terminated, 129, 2, kind, qscale=-2.5))
        check_case(c, vr.make_case(K, n, terminated, 129, 2, kind, qscale=0.0))


def test_the_longest_frame(c):
    cs = vr.make_case(7, 2, False, vr.MAX_STEPS, 1, "noisy")
    node = check_case(c, cs)
    k = fields(node.kernel(1))
    assert k["workspace"] == vr.WAVES * vr.MAX_STEPS * 8 and k["lds"] == 0


def test_more_frames_than_the_largest_grid_holds_waves(c):
    small = c.ViterbiNode(6, 3, vr.GENS[(3, 2)], terminated=False)
    k = fields(small.kernel(10 ** 6))
    assert k["grid"] == k["max_grid"] >= 256                               # the largest grid: the smallest LDS share
    frames = k["grid"] * k["waves"] + 5
    for K, n, terminated, steps in ((3, 2, False, 6), (7, 3, True, 70)):
        cs = vr.make_case(K, n, terminated, steps, frames, "noisy")
        node = check_case(c, cs)
        kk = fields(node.kernel(frames))
        assert frames > kk["grid"] * kk["waves"] and kk["grid"] == kk["max_grid"]     # waves decode several frames
    # the workspace form with more frames than waves: its grid is capped by the workspace budget
    long_node = c.ViterbiNode(vr.MAX_STEPS, 7, terminated=False)
    kk = fields(long_node.kernel(10 ** 6))
    assert kk["workspace"] <= 256 << 20 and kk["grid"] == kk["max_grid"]
    cs = vr.make_case(3, 2, False, vr.LDS_STEPS + 1, 11, "noisy")
    assert fields(decoder_of(c, cs).kernel(2))["grid"] == 1
    check_case(c, cs)


def test_host_pointer_run_equals_run_dev(c):
    for cs in (vr.make_case(7, 2, True, 300, 3, "noisy"), vr.make_case(5, 3, False, vr.LDS_STEPS + 1, 2, "wide")):
        _, llr, bits, metric = vr.case_data(cs)
        node = decoder_of(c, cs)
        got, met = node.run(llr, metrics=True)
        dev, dmet = decode_dev(c, decoder_of(c, cs), llr)
        assert got.tobytes() == dev.tobytes() == vr.pack_records(bits).tobytes() and np.array_equal(met, dmet) and np.array_equal(met, metric)
        assert node.run(llr).tobytes() == got.tobytes()                     # metrics are optional
        assert node.run(np.zeros((0, cs.record_llrs), np.float32)).shape == (0, node.out_frame_bytes)


@pytest.mark.parametrize("steps", [300, vr.LDS_STEPS + 1])
def test_a_second_call_on_the_handle_equals_a_fresh_handle(c, steps):
    """Stale survivors or workspace would show here: more frames first, then fewer and different ones."""
    first = vr.make_case(7, 2, True, steps, 9, "noisy")
    second = vr.make_case(7, 2, True, steps, 2, "special")
    node = check_case(c, first)
    check_case(c, second, node)
    check_case(c, first, node)


# ------------------------------------------------------------------ 2. encoder
@pytest.mark.parametrize("K,n,terminated", CODES)
def test_encoder_is_the_reference_bit_for_bit(c, K, n, terminated):
    rng = np.random.default_rng(K * 100 + n * 10 + terminated)
    gens = vr.GENS[(K, n)]
    for i, steps in enumerate(vr.step_counts(K)):
        T = steps - (K - 1 if terminated else 0)
        if T < 1:
            continue
        frames = 1 + i % 3
        node = c.ConvEncoderNode(T, K, gens, terminated=terminated)
        fin, fout = node.in_frame_bytes, node.out_frame_bytes
        assert fin == vr.record_bytes(T) and fout == vr.record_bytes(n * steps)
        sent = rng.integers(0, 2, (frames, T), dtype=np.uint8)
        records = vr.pack_records(sent)
        dirty = records.copy()                                             # bits from T on do not count
        dirty |= ~vr.pack_records(np.ones((frames, T), np.uint8))
        want = vr.pack_records(vr.ref_encode(sent, K, gens, terminated))
        d_in = c.DeviceBuf(frames * fin).upload(dirty)
        d_out = c.DeviceBuf(frames * fout + GUARD).upload(np.full(frames * fout + GUARD, 0xFF, np.uint8))
        node.run_dev(d_in.ptr, frames, d_out.ptr)
        raw = d_out.download(np.uint8, frames * fout + GUARD)
        assert np.array_equal(raw[: frames * fout].reshape(frames, fout), want), (K, n, terminated, steps)
        assert np.all(raw[frames * fout:] == 0xFF)
        assert node.run(records).tobytes() == want.tobytes()               # host pointers


def test_encoder_past_the_grid_and_timers(c):
    node = c.ConvEncoderNode(40, 7, vr.GENS[(7, 3)])                        # 138 coded bits: 5 words, the last one mostly padding
    k = fields(node.kernel(10 ** 7))
    assert k["grid"] == k["max_grid"] and k["wg"] == 256
    frames = k["grid"] * k["wg"] // 5 + 77
    assert fields(node.kernel(frames))["words"] > k["grid"] * k["wg"]      # lanes walk several words
    sent = np.random.default_rng(9).integers(0, 2, (frames, 40), dtype=np.uint8)
    timer = c.KernelTimer(2).attach(node)
    got = node.run(vr.pack_records(sent))
    assert got.tobytes() == vr.pack_records(vr.ref_encode(sent, 7, vr.GENS[(7, 3)], True)).tobytes()
    ms = timer.read_ms()
    assert ms.size == 1 and 0 < ms[0] < 100
    timer.close()
    cs = vr.make_case(7, 2, True, 300, 3, "noisy")
    dec = decoder_of(c, cs)
    timer = c.KernelTimer(2).attach(dec)
    check_case(c, cs, dec)
    ms = timer.read_ms()
    assert ms.size == 1 and 0 < ms[0] < 100
    timer.close()


# ------------------------------------------------------------------ 2b. generators off the one set per (K, n)
@pytest.mark.parametrize("K,n,name", GEN_SETS)
def test_generator_corners_decode_bit_for_bit(c, K, n, name):
    """Generators without the input bit, without the oldest register bit (the two branches into a state tie whenever their
    metrics do), a single bit beside all ones, one generator n times, random sets: the tie rules decide most bits here."""
    gens = dict(vr.GEN_CORNERS[(K, n)])[name]
    for terminated in (True, False):
        for steps in vr.corner_steps(K):
            for cs, llr, bits, metric in vr.corner_data(K, n, gens, terminated, steps):
                assert cs.gens == gens and cs.frames == llr.shape[0] == 3
                got, met = decode_dev(c, decoder_of(c, cs), llr)
                assert np.array_equal(met, metric), (cs, met, metric)
                assert np.array_equal(got, vr.pack_records(bits)), (cs, int(np.count_nonzero(vr.unpack_records(got, cs.T) != bits)))


@pytest.mark.parametrize("K,n", sorted(vr.GEN_CORNERS))
def test_generator_corners_encode_bit_for_bit(c, K, n):
    rng = np.random.default_rng(K * 10 + n)
    for name, gens in vr.GEN_CORNERS[(K, n)]:
        for terminated in (True, False):
            for steps in vr.corner_steps(K)[:3]:
                T, frames = steps - (K - 1 if terminated else 0), 3
                node = c.ConvEncoderNode(T, K, gens, terminated=terminated)
                fin, fout = node.in_frame_bytes, node.out_frame_bytes
                assert fin == vr.record_bytes(T) and fout == vr.record_bytes(n * steps)
                sent = rng.integers(0, 2, (frames, T), dtype=np.uint8)
                records = vr.pack_records(sent)
                dirty = records | ~vr.pack_records(np.ones((frames, T), np.uint8))   # bits from T on do not count
                want = vr.pack_records(vr.ref_encode(sent, K, gens, terminated))
                d_in = c.DeviceBuf(frames * fin).upload(dirty)
                d_out = c.DeviceBuf(frames * fout + GUARD).upload(np.full(frames * fout + GUARD, 0xFF, np.uint8))
                node.run_dev(d_in.ptr, frames, d_out.ptr)
                raw = d_out.download(np.uint8, frames * fout + GUARD)
                assert np.array_equal(raw[: frames * fout].reshape(frames, fout), want), (K, n, name, terminated, steps)
                assert np.all(raw[frames * fout:] == 0xFF)
                assert node.run(records).tobytes() == want.tobytes()               # host pointers


# ------------------------------------------------------------------ 3. the loop on the device
def test_the_coded_loop_on_the_device(c):
    """PRNS bits -> ConvEncoderNode -> QPSK -> AwgnNode (seeded) -> DeframeNode (LLR, one synthetic detection per frame) ->
    ViterbiNode, nothing on the host in between: the decoded bits are ref_decode of the downloaded LLRs, and the sent bits,
    while the hard decisions of the same LLRs are not."""
    frames, T = vr.LOOP_FRAMES, vr.LOOP_T
    mask, state, width = vr.LOOP_PRNS
    enc = c.ConvEncoderNode(T)                                              # the defaults: K = 7, (171, 133), terminated
    assert enc.in_frame_bytes == T // 8 and enc.out_frame_bytes == vr.LOOP_RECORD
    n_sym = frames * vr.LOOP_SYMS
    d_info, d_coded = c.DeviceBuf(frames * T // 8), c.DeviceBuf(frames * vr.LOOP_RECORD)
    d_tx, d_rx = c.DeviceBuf(4 * n_sym), c.DeviceBuf(8 * n_sym)
    c.PrnsNode(mask, state, width).run_dev(frames * T, d_info.ptr, packed=True)
    enc.run_dev(d_info.ptr, frames, d_coded.ptr)
    assert c.lib().comms_qpsk_byte_mod_dev(d_coded.ptr, frames * vr.LOOP_RECORD, d_tx.ptr, 0, None) == c.COMMS_OK
    c.NoiseSource(vr.LOOP_SEED).set_input_format("i16", 1.0).awgn_dev(d_tx.ptr, n_sym, vr.LOOP_SIGMA, d_rx.ptr)
    deframe = c.DeframeNode(vr.LOOP_F, 0, 0).set_output_format("llr").set_llr_scale(vr.LOOP_LLR_SCALE)
    det = np.zeros(frames, c.FRAME_DETECTION_DTYPE)
    det["index"], det["corr_re"], det["metric"] = np.arange(frames) * vr.LOOP_SYMS, 1.0, 1.0
    assert deframe.frame_bytes() == 4 * vr.LOOP_CODED
    d_llr = c.DeviceBuf(frames * 4 * vr.LOOP_CODED)
    assert deframe.run_dev(d_rx.ptr, n_sym, det, d_llr.ptr, frames) == frames
    dec = c.ViterbiNode(T, record_llrs=vr.LOOP_CODED, qscale=vr.LOOP_QSCALE)
    d_bits, d_met = c.DeviceBuf(frames * dec.out_frame_bytes), c.DeviceBuf(4 * frames)
    dec.run_dev(d_llr.ptr, frames, d_bits.ptr, d_met.ptr)
    errs = c.bit_errors_dev(d_bits.ptr, d_info.ptr, frames * T)             # T is a multiple of 32: the records have no padding
    # what the host sees afterwards
    sent = vr.unpack_records(d_info.download(np.uint8, frames * T // 8).reshape(frames, -1), T)
    assert np.array_equal(sent, vr.loop_bits())
    llr = d_llr.download(np.float32, frames * vr.LOOP_CODED).reshape(frames, -1)
    got = vr.unpack_records(d_bits.download(np.uint8, frames * dec.out_frame_bytes).reshape(frames, -1), T)
    want, metric = vr.ref_decode(vr.ref_quantise(llr, vr.LOOP_QSCALE), vr.LOOP_K, vr.LOOP_GENS, T, True)
    coded = vr.ref_encode(sent, vr.LOOP_K, vr.LOOP_GENS, True)
    raw = int(np.count_nonzero((llr < 0) != (coded == 1)))
    print("Es/N0 %.1f dB: %d raw errors of %d coded bits, %d decoded errors of %d" % (vr.LOOP_ESN0_DB, raw, coded.size, errs, sent.size))
    assert np.array_equal(got, want) and np.array_equal(d_met.download(np.int32, frames), metric)
    assert np.array_equal(got, sent) and errs == 0
    assert raw > 0 and all(np.any((llr[f] < 0) != (coded[f] == 1)) for f in range(frames))
    # the model of tests/test_viterbi_ref.py is this channel: the same decisions but for values within rounding of zero
    _, model = vr.loop_model()
    assert np.max(np.abs(model - llr)) < 1e-4 * np.max(np.abs(model))


# ------------------------------------------------------------------ 4. refusals
def test_refusals_leave_nothing_behind(c):
    lib = c.lib()
    g72 = (C.c_uint32 * 3)(0o171, 0o133, 0o165)

    def gens(*v):
        return (C.c_uint32 * 3)(*(list(v) + [1] * (3 - len(v))))

    bad = [(2, 2, gens(3, 1), 0, 8), (8, 2, gens(0o371, 0o133), 0, 8), (7, 1, g72, 0, 8), (7, 4, g72, 0, 8), (7, 2, gens(0, 0o133), 0, 8),
           (7, 2, gens(0o171, 128), 0, 8), (5, 3, gens(0o25, 0o33, 32), 0, 8), (7, 2, g72, 2, 8), (7, 2, g72, -1, 8), (7, 2, g72, 0, 0),
           (7, 2, g72, 0, (1 << 16) - 5), (7, 2, g72, 1, (1 << 16) + 1), (5, 2, None, 0, 8), (7, 3, None, 0, 8)]
    for K, n, g, flags, T in bad:
        for create, extra in ((lib.comms_convenc_create, ()), (lib.comms_viterbi_create, (0,))):
            h = C.c_void_p(0xDEAD)
            assert create(K, n, g, flags, T, *extra, 0, C.byref(h)) == c.COMMS_ERR_ARG, (K, n, flags, T)
            assert not h.value                                             # no handle, nothing to destroy
    h = C.c_void_p(0xDEAD)
    assert lib.comms_viterbi_create(7, 2, g72, 0, 8, 2 * 14 - 1, 0, C.byref(h)) == c.COMMS_ERR_ARG and not h.value   # record_llrs < n * steps
    assert "record_llrs" in lib.comms_last_error().decode()
    assert lib.comms_viterbi_create(7, 2, g72, 0, 8, 0, 0, None) == c.COMMS_ERR_ARG
    with pytest.raises(c.CommsError) as e:
        c.ViterbiNode(8, 8)
    assert e.value.code == c.COMMS_ERR_ARG
    with pytest.raises(ValueError):
        c.ConvEncoderNode(8, 7, (0o171, 0o133), n=3)
    assert (1 << 16) - 6 + 6 == vr.MAX_STEPS
    c.ViterbiNode((1 << 16) - 6)                                           # exactly 2^16 steps is allowed
    dec, enc = c.ViterbiNode(8), c.ConvEncoderNode(8)
    for q in (np.nan, np.inf, -np.inf):
        assert lib.comms_viterbi_set_quant_scale(dec._h, C.c_float(q)) == c.COMMS_ERR_ARG
    buf = c.DeviceBuf(4096)
    for args in ((buf.ptr + 2, 1, buf.ptr + 1024, None), (buf.ptr, 1, buf.ptr + 1025, None), (buf.ptr, 1, buf.ptr + 1024, buf.ptr + 2050),
                 (None, 1, buf.ptr, None), (buf.ptr, 1, None, None)):
        assert lib.comms_viterbi_run_dev(dec._h, args[0], args[1], args[2], args[3], None) == c.COMMS_ERR_ARG, args
    for args in ((buf.ptr + 1, 1, buf.ptr + 1024), (buf.ptr, 1, buf.ptr + 1026), (None, 1, buf.ptr)):
        assert lib.comms_convenc_run_dev(enc._h, args[0], args[1], args[2], None) == c.COMMS_ERR_ARG, args
    assert lib.comms_viterbi_run_dev(None, buf.ptr, 1, buf.ptr, None, None) == c.COMMS_ERR_ARG
    assert lib.comms_viterbi_in_frame_bytes(None) == 0 and lib.comms_convenc_out_frame_bytes(None) == 0
    dec.run_dev(None, 0, None)                                             # no frames: nothing to do
    # the handles still work after the refused calls
    cs = vr.make_case(7, 2, True, 14, 2, "noisy")
    check_case(c, cs, dec)


# ------------------------------------------------------------------ 5. host graph
def test_host_graph_nodes(c):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "comms_rs_amd", "host"), "-s"], timeout=600)
    out = subprocess.run([os.path.join(ROOT, "comms_rs_amd", "lib", "test_viterbi_nodes_gpu")], capture_output=True,
                         text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all passed" in out.stdout
