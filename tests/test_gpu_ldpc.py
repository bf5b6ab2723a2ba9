"""GPU tests of the LDPC encoder and decoder (comms_ldpcenc_*, comms_ldpcdec_*; ldpc_encode_kernel, ldpc_decode_kernel)
against tests/ldpc_ref.py.  The arithmetic is integer and the schedule fixed, so bits and statuses are compared exactly;
tests/test_ldpc_ref.py checks the reference itself and pins the noisy points.  Run with -m gpu."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ldpc_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
GUARD = 256
ENCODER_FORMATS = [n for n, f in lr.FORMATS.items() if f.encoder]


@pytest.fixture(scope="module")
def c():
    import comms_rs_amd as c

    assert c.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested (no CPU fallback)"
    return c


def decoder_of(c, cs):
    f = lr.format_of(cs.fmt)
    return c.LdpcDecoderNode(lr.base_of(cs.fmt), f.Z, cs.max_iters, cs.norm16, cs.record_llrs, cs.qscale)


def fields(name):
    return {a: int(b) for a, b in re.findall(r"(\w+)=(\d+)", name)}


def decode_dev(c, node, llr):
    """run_dev on uploaded records into 0xFF-filled buffers with a guard region behind them: (records, statuses)."""
    frames = llr.shape[0]
    fb = node.out_frame_bytes
    d_llr = c.DeviceBuf(llr.nbytes).upload(llr)
    d_bits = c.DeviceBuf(frames * fb + GUARD).upload(np.full(frames * fb + GUARD, 0xFF, np.uint8))
    d_st = c.DeviceBuf(4 * frames + GUARD).upload(np.full(4 * frames + GUARD, 0xFF, np.uint8))
    node.run_dev(d_llr.ptr, frames, d_bits.ptr, d_st.ptr)
    raw = d_bits.download(np.uint8, frames * fb + GUARD)
    st = d_st.download(np.uint8, 4 * frames + GUARD)
    assert np.all(raw[frames * fb:] == 0xFF) and np.all(st[4 * frames:] == 0xFF), "the guard region was written"
    return raw[: frames * fb].reshape(frames, fb), st[: 4 * frames].view(np.int32)


def check_case(c, cs, node=None):
    f = lr.format_of(cs.fmt)
    T = (f.nb - f.mb) * f.Z
    _, llr, bits, status = lr.case_data(cs)
    node = decoder_of(c, cs) if node is None else node
    assert node.in_frame_bytes == 4 * cs.record_llrs and node.out_frame_bytes == lr.record_bytes(T)
    got, st = decode_dev(c, node, llr)
    want = lr.pack_records(bits)                                           # padding bits and bytes 0
    assert np.array_equal(st, status), (cs, st[:8], status[:8])
    assert np.array_equal(got, want), (cs, int(np.count_nonzero(lr.unpack_records(got, T) != bits)))
    return node


# ------------------------------------------------------------------ 1. decoder: every format, input, iteration limit and scale
@pytest.mark.parametrize("kind", lr.KINDS)
@pytest.mark.parametrize("fmt", list(lr.FORMATS))
def test_decoder_is_the_reference_bit_for_bit(c, fmt, kind):
    for max_iters in (1, 2, 20):
        for norm16 in (12, 16):
            check_case(c, lr.make_case(fmt, kind, max_iters=max_iters, norm16=norm16))
    if kind == "planted":                                                  # wrong bits that survive: the stopping test must see them,
        for max_iters in (1, 2, 20):                                       # also where two failing checks sit 64 apart in one lane
            cs = lr.make_case(fmt, kind, max_iters=max_iters, norm16=1)
            check_case(c, cs)
            assert np.count_nonzero(lr.case_data(cs)[3] < 0) == cs.frames - 1
    if kind == "special":                                                  # the same with a scale that moves the clamp
        for qscale in (-2.5, 0.0, 0.03):
            check_case(c, lr.make_case(fmt, kind, qscale=qscale))


# ------------------------------------------------------------------ 2. frame counts around a workgroup and past many of them
def test_frame_counts_around_a_workgroup(c):
    f = lr.FORMATS["A"]
    fpw = fields(c.LdpcDecoderNode(lr.base_of("A"), f.Z).kernel(1))["frames_per_wg"]
    assert fpw >= 2
    for frames in (1, fpw - 1, fpw + 1, 250 * fpw + 3):                     # the last one leaves a workgroup partly empty
        cs = lr.make_case("A", "noisy", frames=frames)
        node = check_case(c, cs)
        k = fields(node.kernel(frames))
        assert k["grid"] == -(-frames // fpw) and k["grid"] * fpw >= frames
    fpw_f = fields(c.LdpcDecoderNode(lr.base_of("F"), 128).kernel(2))["frames_per_wg"]
    check_case(c, lr.make_case("F", "noisy", frames=fpw_f + 1, max_iters=3))


# ------------------------------------------------------------------ 3. encoder
@pytest.mark.parametrize("fmt", ENCODER_FORMATS)
def test_encoder_is_the_reference_bit_for_bit(c, fmt):
    f = lr.FORMATS[fmt]
    B, Z = lr.base_of(fmt), f.Z
    N, T = f.nb * Z, (f.nb - f.mb) * Z
    node = c.LdpcEncoderNode(B, Z)
    fin, fout = node.in_frame_bytes, node.out_frame_bytes
    assert fin == lr.record_bytes(T) and fout == lr.record_bytes(N)
    fpw = fields(node.kernel(1))["frames_per_wg"]
    rng = np.random.default_rng(f.seed)
    for frames in (1, fpw + 1, 2 if fmt == "F" else 3 * fpw + 2):
        sent = rng.integers(0, 2, (frames, T), dtype=np.uint8)
        records = lr.pack_records(sent)
        dirty = records | ~lr.pack_records(np.ones((frames, T), np.uint8))   # bits from T on do not count
        want = lr.pack_records(lr.ref_encode(sent, B, Z))
        d_in = c.DeviceBuf(frames * fin).upload(dirty)
        d_out = c.DeviceBuf(frames * fout + GUARD).upload(np.full(frames * fout + GUARD, 0xFF, np.uint8))
        node.run_dev(d_in.ptr, frames, d_out.ptr)
        raw = d_out.download(np.uint8, frames * fout + GUARD)
        assert np.array_equal(raw[: frames * fout].reshape(frames, fout), want), (fmt, frames)
        assert np.all(raw[frames * fout:] == 0xFF)
        assert node.run(records).tobytes() == want.tobytes()               # host pointers
        k = fields(node.kernel(frames))
        assert k["grid"] * k["frames_per_wg"] >= frames and k["Z"] == Z and k["lds"] <= 160 * 1024
    assert node.run(np.zeros((0, fin), np.uint8)).shape == (0, fout)
    node.run_dev(None, 0, None)


# ------------------------------------------------------------------ 4. host pointers
def test_host_pointer_run_equals_run_dev(c):
    for cs in (lr.make_case("B", "noisy"), lr.make_case("C", "wide", max_iters=5), lr.make_case("G", "special", qscale=-2.5)):
        _, llr, bits, status = lr.case_data(cs)
        node = decoder_of(c, cs)
        got, st = node.run(llr, status=True)
        dev, dst = decode_dev(c, decoder_of(c, cs), llr)
        assert got.tobytes() == dev.tobytes() == lr.pack_records(bits).tobytes() and np.array_equal(st, dst) and np.array_equal(st, status)
        assert node.run(llr).tobytes() == got.tobytes()                     # statuses are optional
        assert node.run(np.zeros((0, cs.record_llrs), np.float32)).shape == (0, node.out_frame_bytes)
        node.run_dev(None, 0, None)                                         # no frames: nothing to do


# ------------------------------------------------------------------ 5. nothing is left from one call to the next
@pytest.mark.parametrize("fmt", ["B", "C"])
def test_a_second_call_on_the_handle_equals_a_fresh_handle(c, fmt):
    """Stale posteriors, check records or statuses in LDS would show here: more frames first, then fewer and different ones."""
    first = lr.make_case(fmt, "noisy")
    second = lr.make_case(fmt, "zeros", frames=2, qscale=first.qscale)
    third = lr.make_case(fmt, "special", frames=3, qscale=first.qscale)
    node = check_case(c, first)
    check_case(c, second, node)
    check_case(c, third, node)
    check_case(c, first, node)


# ------------------------------------------------------------------ 5b. the corner table: shapes off the formats A ... G
@pytest.mark.parametrize("kind", lr.KINDS)
@pytest.mark.parametrize("fmt", list(lr.CORNERS))
def test_corner_decoder_is_the_reference_bit_for_bit(c, fmt, kind):
    """Workgroups of 2 and 3 waves, records of more than 64 chunks, full sign masks over two passes, Z = 2, 65 and 127, one and
    two block rows, a variable in 32 layers: tests/test_ldpc_ref.py says which format is which and what each can see."""
    f = lr.CORNERS[fmt]
    fpw = lr.frames_per_wg(f.mb, f.nb, f.Z)
    assert {2, 3} <= {lr.frames_per_wg(g.mb, g.nb, g.Z) for g in lr.CORNERS.values()}
    for cs in lr.corner_cases(fmt, kind):
        node = check_case(c, cs)
        k = fields(node.kernel(cs.frames))
        assert k["frames_per_wg"] == fpw and k["wg"] == 64 * fpw and k["grid"] == -(-cs.frames // fpw) > 1, (cs, k)
        assert cs.frames % fpw                                             # the last workgroup is partly empty
    if kind == "planted" and fmt == lr.CORNER_255:
        assert np.count_nonzero(lr.case_data(cs)[3] == -255) == cs.frames - 1


@pytest.mark.parametrize("fmt", lr.ENCODER_CORNERS)
def test_corner_encoder_is_the_reference_bit_for_bit(c, fmt):
    """r = 1 and r = mb - 2, s and t at 0 and Z - 1, Z = 2 and 65, and a record of 159 words: a partial second round of the packing."""
    f = lr.CORNERS[fmt]
    B, Z = lr.base_of(fmt), f.Z
    N, T = f.nb * Z, (f.nb - f.mb) * Z
    node = c.LdpcEncoderNode(B, Z)
    fin, fout = node.in_frame_bytes, node.out_frame_bytes
    assert fin == lr.record_bytes(T) and fout == lr.record_bytes(N) == 4 * lr.out_words(N)
    fpw = fields(node.kernel(1))["frames_per_wg"]
    rng = np.random.default_rng(f.seed)
    for frames in (2, fpw + 1, 2 * fpw + 3):
        sent = rng.integers(0, 2, (frames, T), dtype=np.uint8)
        records = lr.pack_records(sent)
        dirty = records | ~lr.pack_records(np.ones((frames, T), np.uint8))   # bits from T on do not count
        want = lr.pack_records(lr.ref_encode(sent, B, Z))
        d_in = c.DeviceBuf(frames * fin).upload(dirty)
        d_out = c.DeviceBuf(frames * fout + GUARD).upload(np.full(frames * fout + GUARD, 0xFF, np.uint8))
        node.run_dev(d_in.ptr, frames, d_out.ptr)
        raw = d_out.download(np.uint8, frames * fout + GUARD)
        assert np.array_equal(raw[: frames * fout].reshape(frames, fout), want), (fmt, frames)
        assert np.all(raw[frames * fout:] == 0xFF)
        assert node.run(records).tobytes() == want.tobytes()               # host pointers
        k = fields(node.kernel(frames))
        assert k["grid"] * k["frames_per_wg"] >= frames and k["Z"] == Z and k["lds"] <= 160 * 1024


@pytest.mark.parametrize("fmt", ["fpw2", "fpw3"])
def test_a_second_call_on_a_corner_handle_equals_a_fresh_handle(c, fmt):
    """As section 5 with workgroups of 2 and 3 waves: more frames first, then fewer and different ones, then the first again."""
    first = lr.make_case(fmt, "planted", norm16=1)
    second = lr.make_case(fmt, "noisy")
    third = lr.make_case(fmt, "zeros", frames=2, qscale=second.qscale)
    assert first.frames > second.frames > third.frames and (first.max_iters, first.record_llrs) == (second.max_iters, second.record_llrs)
    f = lr.CORNERS[fmt]
    node = c.LdpcDecoderNode(lr.base_of(fmt), f.Z, first.max_iters, first.norm16, first.record_llrs, first.qscale)
    check_case(c, first, node)
    node.set_quant_scale(second.qscale)
    for cs in (second, third):
        check_case(c, cs._replace(norm16=1), node)
    node.set_quant_scale(first.qscale)
    check_case(c, first, node)


# ------------------------------------------------------------------ 6. what the node reports
@pytest.mark.parametrize("fmt", list(lr.FORMATS))
def test_kernel_fields(c, fmt):
    f = lr.FORMATS[fmt]
    B = lr.base_of(fmt)
    node = c.LdpcDecoderNode(B, f.Z, max_iters=7)
    for frames in (0, 1, 5, 1000, 10 ** 6):
        name = node.kernel(frames)
        k = fields(name)
        assert name.startswith("ldpc_decode_kernel ") and k["grid"] * k["frames_per_wg"] >= frames and k["lds"] <= 160 * 1024
        assert (k["grid"] - 1) * k["frames_per_wg"] < frames or frames == 0 and k["grid"] == 0
        assert (k["mb"], k["nb"], k["Z"], k["max_iters"]) == (f.mb, f.nb, f.Z, 7) and k["edges"] == int(np.count_nonzero(B >= 0))
        assert k["waves"] == k["frames_per_wg"] >= 1 and k["wg"] == 64 * k["waves"]
        assert k["lds"] >= k["frames_per_wg"] * (2 * f.nb * f.Z + 8 * f.mb * f.Z)           # all state of a frame is in LDS


# ------------------------------------------------------------------ 7. timers
def test_kernel_timers(c):
    f = lr.FORMATS["B"]
    enc = c.LdpcEncoderNode(lr.base_of("B"), f.Z)
    sent = np.random.default_rng(9).integers(0, 2, (5, 12 * f.Z), dtype=np.uint8)
    timer = c.KernelTimer(2).attach(enc)
    got = enc.run(lr.pack_records(sent))
    assert got.tobytes() == lr.pack_records(lr.ref_encode(sent, lr.base_of("B"), f.Z)).tobytes()
    ms = timer.read_ms()
    assert ms.size == 1 and 0 < ms[0] < 100
    timer.close()
    cs = lr.make_case("B", "noisy")
    dec = decoder_of(c, cs)
    timer = c.KernelTimer(2).attach(dec)
    check_case(c, cs, dec)
    ms = timer.read_ms()
    assert ms.size == 1 and 0 < ms[0] < 100
    timer.close()


# ------------------------------------------------------------------ 8. the loop on the device
def test_the_coded_loop_on_the_device(c):
    """PRNS bits -> LdpcEncoderNode -> QPSK -> NoiseSource.awgn_dev (seeded) -> DeframeNode (LLR, one synthetic detection per
    frame) -> LdpcDecoderNode, nothing on the host in between: the decoded bits are ref_decode of the downloaded LLRs, and the
    sent bits, while the hard decisions of the same LLRs are wrong in every frame."""
    frames, T, N = lr.LOOP_FRAMES, lr.LOOP_T, lr.LOOP_N
    mask, state, width = lr.LOOP_PRNS
    B = lr.loop_base()
    enc = c.LdpcEncoderNode(B, lr.LOOP_Z)
    assert enc.in_frame_bytes == T // 8 and enc.out_frame_bytes == lr.LOOP_RECORD == N // 8
    n_sym = frames * lr.LOOP_SYMS
    d_info, d_coded = c.DeviceBuf(frames * T // 8), c.DeviceBuf(frames * lr.LOOP_RECORD)
    d_tx, d_rx = c.DeviceBuf(4 * n_sym), c.DeviceBuf(8 * n_sym)
    c.PrnsNode(mask, state, width).run_dev(frames * T, d_info.ptr, packed=True)
    enc.run_dev(d_info.ptr, frames, d_coded.ptr)
    assert c.lib().comms_qpsk_byte_mod_dev(d_coded.ptr, frames * lr.LOOP_RECORD, d_tx.ptr, 0, None) == c.COMMS_OK
    c.NoiseSource(lr.LOOP_SEED).set_input_format("i16", 1.0).awgn_dev(d_tx.ptr, n_sym, lr.LOOP_SIGMA, d_rx.ptr)
    deframe = c.DeframeNode(lr.LOOP_SYMS, 0, 0).set_output_format("llr").set_llr_scale(lr.LOOP_LLR_SCALE)
    det = np.zeros(frames, c.FRAME_DETECTION_DTYPE)
    det["index"], det["corr_re"], det["metric"] = np.arange(frames) * lr.LOOP_SYMS, 1.0, 1.0
    assert deframe.frame_bytes() == 4 * N
    d_llr = c.DeviceBuf(frames * 4 * N)
    assert deframe.run_dev(d_rx.ptr, n_sym, det, d_llr.ptr, frames) == frames
    dec = c.LdpcDecoderNode(B, lr.LOOP_Z, lr.LOOP_ITERS, qscale=lr.LOOP_QSCALE)
    assert dec.in_frame_bytes == deframe.frame_bytes()
    d_bits, d_st = c.DeviceBuf(frames * dec.out_frame_bytes), c.DeviceBuf(4 * frames)
    dec.run_dev(d_llr.ptr, frames, d_bits.ptr, d_st.ptr)
    errs = c.bit_errors_dev(d_bits.ptr, d_info.ptr, frames * T)             # T is a multiple of 32: the records have no padding
    # what the host sees afterwards
    sent = lr.unpack_records(d_info.download(np.uint8, frames * T // 8).reshape(frames, -1), T)
    assert np.array_equal(sent, lr.loop_bits())
    llr = d_llr.download(np.float32, frames * N).reshape(frames, -1)
    got = lr.unpack_records(d_bits.download(np.uint8, frames * dec.out_frame_bytes).reshape(frames, -1), T)
    want, status = lr.ref_decode(lr.ref_quantise(llr, lr.LOOP_QSCALE), B, lr.LOOP_Z, lr.LOOP_ITERS)
    coded = lr.ref_encode(sent, B, lr.LOOP_Z)
    raw = (llr < 0) != (coded == 1)
    print("Es/N0 %.1f dB: %d raw errors of %d coded bits, %d decoded errors of %d, statuses %s"
          % (lr.LOOP_ESN0_DB, int(raw.sum()), coded.size, errs, sent.size, status.tolist()))
    assert np.array_equal(got, want) and np.array_equal(d_st.download(np.int32, frames), status)
    assert np.array_equal(got, sent) and errs == 0 and np.all(status > 0)
    assert np.all(raw.any(axis=1))
    # the model of tests/test_ldpc_ref.py is this channel: the same decisions but for values within rounding of zero
    _, model = lr.loop_model()
    assert np.max(np.abs(model - llr)) < 1e-4 * np.max(np.abs(model))


# ------------------------------------------------------------------ 9. refusals
def test_refusals_leave_nothing_behind(c):
    lib = c.lib()

    def mat(B):
        return np.ascontiguousarray(B, np.int16)

    def refused(B, mb, nb, Z, what, encoder=False, dec_args=(20, 12, 0)):
        B = mat(B)
        p = B.ctypes.data_as(C.c_void_p)
        creates = [(lib.comms_ldpcenc_create, ())] if encoder else [(lib.comms_ldpcenc_create, ()), (lib.comms_ldpcdec_create, dec_args)]
        for create, extra in creates:
            h = C.c_void_p(0xDEAD)
            assert create(mb, nb, Z, p, *extra, 0, C.byref(h)) == c.COMMS_ERR_ARG, (mb, nb, Z, what)
            assert not h.value                                             # no handle, nothing to destroy
            assert what in lib.comms_last_error().decode(), (what, lib.comms_last_error().decode())

    big = np.zeros((65, 65), np.int16)
    good = lr.base_of("B").copy()                                          # (12, 24, 27)
    mb, nb, Z, kb = 12, 24, 27, 12
    # every limit one past its edge
    refused(big, 0, 8, 4, "mb")
    refused(big, 33, 40, 4, "mb")
    refused(good, 12, 12, 27, "nb")
    refused(big, 12, 65, 27, "nb")
    refused(good, 12, 24, 1, "Z")
    refused(good, 12, 24, 129, "Z")
    bad = good.copy()
    bad[3, 2] = Z
    refused(bad, mb, nb, Z, "base[3][2]")
    bad = good.copy()
    bad[4, 5] = -2
    refused(bad, mb, nb, Z, "base[4][5]")
    row1 = np.full((2, 40), -1, np.int16)
    row1[0, :3], row1[1, 7] = 0, 1
    refused(row1, 2, 40, 4, "block row 1")                                 # a row of 1 edge
    row33 = np.full((2, 40), -1, np.int16)
    row33[0, :33], row33[1, :2] = 0, 1
    refused(row33, 2, 40, 4, "block row 0")                                # a row of 33 edges
    row32 = row33.copy()
    row32[0, 32] = -1
    c.LdpcDecoderNode(row32, 4)                                            # exactly 32 is allowed
    for args, what in (((0, 12, 0), "max_iters"), ((256, 12, 0), "max_iters"), ((20, 0, 0), "norm16"), ((20, 17, 0), "norm16"),
                       ((20, 12, nb * Z - 1), "record_llrs")):
        h = C.c_void_p(0xDEAD)
        assert lib.comms_ldpcdec_create(mb, nb, Z, mat(good).ctypes.data_as(C.c_void_p), *args, 0, C.byref(h)) == c.COMMS_ERR_ARG and not h.value
        assert what in lib.comms_last_error().decode()
    p_good = mat(good).ctypes.data_as(C.c_void_p)
    assert lib.comms_ldpcdec_create(mb, nb, Z, p_good, 20, 12, 0, 0, None) == c.COMMS_ERR_ARG
    assert lib.comms_ldpcenc_create(mb, nb, Z, p_good, 0, None) == c.COMMS_ERR_ARG
    h = C.c_void_p(0xDEAD)
    assert lib.comms_ldpcdec_create(mb, nb, Z, None, 20, 12, 0, 0, C.byref(h)) == c.COMMS_ERR_ARG and not h.value
    with pytest.raises(c.CommsError) as e:
        c.LdpcDecoderNode(good, Z, max_iters=0)
    assert e.value.code == c.COMMS_ERR_ARG
    c.LdpcDecoderNode(good, Z, max_iters=255, norm16=1, record_llrs=nb * Z)  # the edges themselves are allowed
    # the encoder's structure: the decoder-only matrix and each single violation
    g = lr.FORMATS["G"]
    refused(lr.base_of("G"), g.mb, g.nb, g.Z, "encoder's form", encoder=True)
    r, s, _ = lr.encoder_structure(good)
    bad = good.copy()
    bad[mb - 1, kb] = (s + 1) % Z                                          # s != s'
    refused(bad, mb, nb, Z, "encoder's form", encoder=True)
    bad = good.copy()
    bad[[i for i in range(1, mb - 1) if i != r][0], kb] = 0                 # a fourth entry in column kb
    refused(bad, mb, nb, Z, "encoder's form", encoder=True)
    bad = good.copy()
    bad[0, kb + 1] = 1                                                     # a shift on the double diagonal
    refused(bad, mb, nb, Z, "encoder's form", encoder=True)
    two = np.array([[0, 1, 2, 0], [1, 0, 2, 0]], np.int16)
    refused(two, 2, 4, 5, "mb >= 3", encoder=True)                         # mb = 2
    c.LdpcDecoderNode(two, 5)                                              # ... which the decoder takes
    for B in (bad, lr.base_of("G")):
        c.LdpcDecoderNode(B, Z if B is bad else g.Z)
    # calls
    cs = lr.make_case("B", "noisy")
    dec, enc = decoder_of(c, cs), c.LdpcEncoderNode(good, Z)
    for q in (np.nan, np.inf, -np.inf):
        assert lib.comms_ldpcdec_set_quant_scale(dec._h, C.c_float(q)) == c.COMMS_ERR_ARG
    assert lib.comms_ldpcdec_set_quant_scale(None, C.c_float(1.0)) == c.COMMS_ERR_ARG
    buf = c.DeviceBuf(8192)
    out = buf.ptr + 4096
    for args in ((buf.ptr + 2, 1, out, None), (buf.ptr, 1, out + 1, None), (buf.ptr, 1, out, out + 1026), (None, 1, out, None),
                 (buf.ptr, 1, None, None), (buf.ptr, 1, buf.ptr + 2000, None)):
        assert lib.comms_ldpcdec_run_dev(dec._h, args[0], args[1], args[2], args[3], None) == c.COMMS_ERR_ARG, args
    for status in (buf.ptr + 2588, out + 40, buf.ptr, out):                # a status array inside the LLR records or the bit records
        assert lib.comms_ldpcdec_run_dev(dec._h, buf.ptr, 1, out, status, None) == c.COMMS_ERR_ARG, status - buf.ptr
        assert "d_status" in lib.comms_last_error().decode()
    for args in ((buf.ptr + 1, 1, out), (buf.ptr, 1, out + 2), (None, 1, out), (buf.ptr, 1, None), (buf.ptr, 1, buf.ptr + 20)):
        assert lib.comms_ldpcenc_run_dev(enc._h, args[0], args[1], args[2], None) == c.COMMS_ERR_ARG, args
    assert lib.comms_ldpcdec_run_dev(None, buf.ptr, 1, out, None, None) == c.COMMS_ERR_ARG
    assert lib.comms_ldpcenc_run_dev(None, buf.ptr, 1, out, None) == c.COMMS_ERR_ARG
    assert lib.comms_ldpcdec_in_frame_bytes(None) == 0 and lib.comms_ldpcdec_out_frame_bytes(None) == 0
    assert lib.comms_ldpcenc_in_frame_bytes(None) == 0 and lib.comms_ldpcenc_out_frame_bytes(None) == 0
    assert lib.comms_ldpcdec_destroy(None) == c.COMMS_OK and lib.comms_ldpcenc_destroy(None) == c.COMMS_OK
    # the handles still work after the refused calls
    check_case(c, cs, dec)
    sent = np.random.default_rng(3).integers(0, 2, (2, kb * Z), dtype=np.uint8)
    assert enc.run(lr.pack_records(sent)).tobytes() == lr.pack_records(lr.ref_encode(sent, good, Z)).tobytes()


# ------------------------------------------------------------------ 10. host graph
def test_host_graph_nodes(c):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "comms_rs_amd", "host"), "-s"], timeout=600)
    out = subprocess.run([os.path.join(ROOT, "comms_rs_amd", "lib", "test_ldpc_nodes_gpu")], capture_output=True,
                         text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all passed" in out.stdout
