"""GPU tests of the frame-check nodes (comms_crc_*; crc_attach_kernel, crc_check_kernel) against tests/crc_ref.py, the bit-serial
register of the header.  Only bits move, so every record, flag and crc is compared for equality; tests/test_crc_ref.py checks
the reference itself and pins the noisy point of the loop, tests/test_crc_tables.py the host arithmetic.  Run with -m gpu."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import crc_ref as cr
import ratematch_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
GUARD = 256


@pytest.fixture(scope="module")
def c():
    import comms_rs_amd as c

    assert c.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested (no CPU fallback)"
    return c


def fields(name):
    return {a: int(b) for a, b in re.findall(r"(\w+)=(\d+)", name)}


def nodes_of(c, p, T):
    return c.CrcAttachNode(p.W, p.poly, p.init, p.xorout, T), c.CrcCheckNode(p.W, p.poly, p.init, p.xorout, T)


def guarded(c, nbytes):
    """A 0xFF-filled device buffer of nbytes with a guard region behind it."""
    return c.DeviceBuf(nbytes + GUARD).upload(np.full(nbytes + GUARD, 0xFF, np.uint8))


def unguard(buf, nbytes):
    raw = buf.download(np.uint8, nbytes + GUARD)
    assert np.all(raw[nbytes:] == 0xFF), "the guard region was written"
    return raw[:nbytes]


def attach_dev(c, node, records, frames):
    d_in = c.DeviceBuf(max(records.nbytes, 4)).upload(records)
    d_out = guarded(c, frames * node.out_frame_bytes)
    node.run_dev(d_in.ptr, frames, d_out.ptr)
    return unguard(d_out, frames * node.out_frame_bytes).reshape(frames, -1)


def check_dev(c, node, records, frames, outputs=(True, True, True, True), counter=None):
    """run_dev into guarded buffers; outputs selects payload, pass, crc, n_failed (the others are NULL).  Returns what was
    selected, None elsewhere; the counter is a device buffer that is NOT zeroed when given."""
    d_in = c.DeviceBuf(max(records.nbytes, 4)).upload(records)
    sizes = (frames * node.out_frame_bytes, 4 * frames, 4 * frames)
    bufs = [guarded(c, n) if on else None for n, on in zip(sizes, outputs)]
    if outputs[3] and counter is None:
        counter = c.DeviceBuf(4).upload(np.zeros(1, np.uint32))
    node.run_dev(d_in.ptr, frames, *[b.ptr if b else None for b in bufs], counter.ptr if outputs[3] else None)
    raw = [unguard(b, n) if b else None for b, n in zip(bufs, sizes)]
    return (raw[0].reshape(frames, -1) if bufs[0] else None, raw[1].view(np.int32) if bufs[1] else None,
            raw[2].view(np.uint32) if bufs[2] else None, int(counter.download(np.uint32, 1)[0]) if outputs[3] else None)


def round_trip(c, p, T, frames, seed, nodes=None):
    """Attach on dirty payload records equals the reference, and the check of that output passes every frame.  Returns the
    dirty input, the attached records and the bits."""
    att, chk = nodes or nodes_of(c, p, T)
    assert att.in_frame_bytes == chk.out_frame_bytes == cr.record_bytes(T)
    assert att.out_frame_bytes == chk.in_frame_bytes == cr.record_bytes(T + p.W)
    bits, dirty = cr.dirty_payload(frames, T, seed)
    want = cr.pack_records(cr.ref_attach(bits, p))                          # padding bits and bytes 0
    got = attach_dev(c, att, dirty, frames)
    assert np.array_equal(got, want), (p, T, frames, np.flatnonzero(np.any(got != want, axis=1))[:5])
    coded = got | ~cr.pack_records(np.ones((frames, T + p.W), np.uint8))    # dirty beyond T + W
    payload, passed, crc, failed = check_dev(c, chk, coded, frames)
    assert np.all(passed == 1) and failed == 0, (p, T, frames, passed)
    assert np.array_equal(crc, cr.ref_crc(bits, p))
    assert np.array_equal(payload, cr.pack_records(bits))
    return dirty, want, bits


# ------------------------------------------------------------------ 1. the catalogue
@pytest.mark.parametrize("name", list(cr.CATALOGUE))
def test_catalogue_on_the_check_string(c, name):
    p, msb_first, crc, tail = cr.CATALOGUE[name]
    bits = cr.string_bits(cr.CHECK_STRING, msb_first)[None, :]
    att, chk = nodes_of(c, p, 72)
    records = cr.pack_records(bits)
    want = cr.pack_records(cr.ref_attach(bits, p))
    for got in (att.run(records), attach_dev(c, att, records, 1)):
        assert np.array_equal(got, want)
        if tail is not None:
            assert bytes(got[0, : 9 + len(tail)]) == cr.CHECK_STRING + tail
        if not msb_first:
            assert bytes(got[0, :9]) == cr.CHECK_STRING
    for payload, passed, got_crc in (chk.run(want), check_dev(c, chk, want, 1)[:3]):
        assert passed.tolist() == [1] and got_crc.tolist() == [crc] and np.array_equal(payload, records)
    assert chk.n_failed == 0


# ------------------------------------------------------------------ 2. shapes
@pytest.mark.parametrize("W", cr.WIDTHS)
def test_shapes_are_the_reference_bit_for_bit(c, W):
    p = cr.SHAPE_PARAMS[W]
    groups = set()
    for i, T in enumerate(cr.payload_lengths(W)):
        nodes = nodes_of(c, p, T)
        for frames in cr.frame_counts(T, i):
            round_trip(c, p, T, frames, 100 * W + i, nodes)
        for node, name in zip(nodes, ("crc_attach_kernel", "crc_check_kernel")):
            k = node.kernel(3)
            f = fields(k)
            assert k.startswith(name) and f["group"] == cr.group_of(T) and f["width"] == W and f["frames"] == 3 and f["lds"] == 0, k
            assert f["words"] == 3 * ((T + W + 31) // 32) and f["rounds"] == -(-((T + 31) // 32) // f["group"]), k
            groups.add(f["group"])
    assert groups == {1, 2, 4, 8, 16, 32, 64}


# ------------------------------------------------------------------ 3. failures
@pytest.mark.parametrize("W,T", [(24, 232), (32, 64), (16, 70), (5, 2100), (8, 24), (1, 31)])
def test_failed_frames_are_flagged_and_counted(c, W, T):
    """One flipped bit per frame: the first and last payload bit, every CRC bit, and a padding bit (where the record has one),
    which must still pass."""
    p = cr.SHAPE_PARAMS[W]
    _, chk = nodes_of(c, p, T)
    record_bits = 8 * chk.in_frame_bytes
    flips = [0, T - 1] + list(range(T, T + W)) + ([T + W, record_bits - 1] if record_bits > T + W else [])
    frames = len(flips)
    bits = np.random.default_rng(W).integers(0, 2, (frames, T), dtype=np.uint8)
    full = np.zeros((frames, record_bits), np.uint8)
    full[:, : T + W] = cr.ref_attach(bits, p)
    full[np.arange(frames), flips] ^= 1
    records = np.packbits(full, axis=1, bitorder="little")
    want_payload, want_pass, want_crc = cr.ref_check(full, p, T)
    n_bad = int(np.count_nonzero(want_pass == 0))
    assert n_bad == 2 + W and want_pass[2 + W:].all()                       # the padding flips pass
    counter = c.DeviceBuf(4).upload(np.zeros(1, np.uint32))
    for call in (1, 2):                                                     # the counter grows over calls without re-zeroing
        payload, passed, crc, failed = check_dev(c, chk, records, frames, counter=counter)
        assert np.array_equal(passed, want_pass) and np.array_equal(crc, want_crc)
        assert np.array_equal(payload, cr.pack_records(want_payload))
        assert failed == call * n_bad
    host = chk.run(records)
    assert np.array_equal(host[1], want_pass) and np.array_equal(host[2], want_crc) and chk.n_failed == n_bad
    for outputs in itertools.product((False, True), repeat=4):              # every combination of NULL outputs
        payload, passed, crc, failed = check_dev(c, chk, records, frames, outputs)
        assert payload is None or np.array_equal(payload, cr.pack_records(want_payload))
        assert passed is None or np.array_equal(passed, want_pass)
        assert crc is None or np.array_equal(crc, want_crc)
        assert failed is None or failed == n_bad


# ------------------------------------------------------------------ 4. lanes walk several frames
@pytest.mark.parametrize("W,T", [(16, 16), (16, 64 + 16)])                  # one-word and three-word checked records
def test_more_words_than_the_grid_has_lanes(c, W, T):
    p = cr.SHAPE_PARAMS[W]
    att, chk = nodes_of(c, p, T)
    words = (T + W + 31) // 32
    assert words == (1 if T == 16 else 3)
    for node in (att, chk):
        k = fields(node.kernel(10 ** 8))
        assert k["grid"] == k["max_grid"] and k["wg"] == cr.WG
        frames = k["grid"] * k["wg"] // words + 77
        kk = fields(node.kernel(frames))
        assert kk["words"] > kk["grid"] * kk["wg"] and kk["grid"] == kk["max_grid"]      # lanes walk several frames
        assert frames * kk["group"] > kk["grid"] * kk["wg"]
    bits = np.random.default_rng(T).integers(0, 2, (frames, T), dtype=np.uint8)
    want = cr.pack_records(cr.ref_attach(bits, p))
    got = attach_dev(c, att, cr.pack_records(bits), frames)
    assert np.array_equal(got, want)
    bad = np.arange(0, frames, 1001)
    got[bad, 0] ^= 1                                                        # the first payload bit of every 1001st frame
    payload, passed, crc, failed = check_dev(c, chk, got, frames)
    want_pass = np.ones(frames, np.int32)
    want_pass[bad] = 0
    bits[bad, 0] ^= 1
    assert np.array_equal(passed, want_pass) and failed == bad.size
    assert np.array_equal(crc, cr.ref_crc(bits, p)) and np.array_equal(payload, cr.pack_records(bits))


# ------------------------------------------------------------------ 5. host pointers, reuse, no frames, timers
def test_run_equals_run_dev_and_a_handle_is_stateless(c):
    p, T = cr.SHAPE_PARAMS[24], 2100
    att, chk = nodes_of(c, p, T)
    dirty, want, bits = round_trip(c, p, T, 3, 1, (att, chk))
    assert att.run(dirty).tobytes() == want.tobytes()
    broken = want.copy()
    broken[1, 5] ^= 0x10
    dev = check_dev(c, chk, broken, 3)
    host = chk.run(broken)
    assert all(np.array_equal(a, b) for a, b in zip(host, dev[:3])) and chk.n_failed == dev[3] == 1
    assert host[1].tolist() == [1, 0, 1]
    # other frames on the same handles equal fresh handles (round_trip compares with the reference, which a fresh handle equals)
    dirty2, want2, _ = round_trip(c, p, T, 2, 2, (att, chk))
    fresh_att, fresh_chk = nodes_of(c, p, T)
    assert att.run(dirty2).tobytes() == fresh_att.run(dirty2).tobytes() == want2.tobytes()
    assert all(np.array_equal(a, b) for a, b in zip(chk.run(want2), fresh_chk.run(want2)))
    # no frames
    att.run_dev(None, 0, None)
    chk.run_dev(None, 0, None, None, None, None)
    assert att.run(np.zeros((0, att.in_frame_bytes), np.uint8)).shape == (0, att.out_frame_bytes)
    empty = chk.run(np.zeros((0, chk.in_frame_bytes), np.uint8))
    assert empty[0].shape == (0, chk.out_frame_bytes) and empty[1].size == 0 and empty[2].size == 0 and chk.n_failed == 0
    # one positive time per launch, in either direction
    for node, call in ((att, lambda: att.run(dirty)), (chk, lambda: chk.run(want))):
        timer = c.KernelTimer(4).attach(node)
        call()
        call()
        ms = timer.read_ms()
        assert ms.size == 2 and np.all(ms > 0) and np.all(ms < 100)
        timer.close()


# ------------------------------------------------------------------ 6. the loop on the device
@pytest.mark.parametrize("point", [cr.LOOP_CLEAN, cr.LOOP_NOISY], ids=["clean", "noisy"])
def test_the_checked_loop_on_the_device(c, point):
    """PRNS payload -> CrcAttachNode (CRC24A) -> ConvEncoderNode -> RateMatchNode (3/4, 17 columns, PRNS scramble) -> QPSK ->
    AwgnNode (seeded) -> DeframeNode (LLR, one synthetic detection per frame) -> RateDematchNode -> ViterbiNode -> CrcCheckNode,
    nothing on the host in between: the receiver learns which frames are good from the device alone."""
    frames, T, p = cr.LOOP_FRAMES, cr.LOOP_T, cr.LOOP_CRC
    N, E = rr.LOOP_CODED, rr.LOOP_E
    sigma = cr.loop_sigma(point)
    scr_packed, scr = rr.loop_scramble()
    att, chk = nodes_of(c, p, T)
    enc = c.ConvEncoderNode(rr.LOOP_T)
    match = c.RateMatchNode(N, rr.LOOP_PATTERN, rr.LOOP_COLS, scramble=scr_packed)
    dematch = c.RateDematchNode(N, rr.LOOP_PATTERN, rr.LOOP_COLS, scramble=scr_packed)
    dec = c.ViterbiNode(rr.LOOP_T, qscale=point.qscale)
    assert att.in_frame_bytes == cr.LOOP_RECORD and att.out_frame_bytes == enc.in_frame_bytes == dec.out_frame_bytes == chk.in_frame_bytes
    n_sym = frames * rr.LOOP_SYMS
    d_payload = c.DeviceBuf(frames * cr.LOOP_RECORD).upload(np.full(frames * cr.LOOP_RECORD, 0xFF, np.uint8))
    d_frame, d_coded = c.DeviceBuf(frames * att.out_frame_bytes), c.DeviceBuf(frames * enc.out_frame_bytes)
    d_sent, d_tx, d_rx = c.DeviceBuf(frames * rr.LOOP_RECORD), c.DeviceBuf(4 * n_sym), c.DeviceBuf(8 * n_sym)
    prns = c.PrnsNode(*cr.LOOP_PRNS)
    for f in range(frames):                                                 # one stream, T bits to the start of every record
        prns.run_dev(T, d_payload.ptr + f * cr.LOOP_RECORD, packed=True)
    att.run_dev(d_payload.ptr, frames, d_frame.ptr)
    enc.run_dev(d_frame.ptr, frames, d_coded.ptr)
    match.run_dev(d_coded.ptr, frames, d_sent.ptr)
    assert c.lib().comms_qpsk_byte_mod_dev(d_sent.ptr, frames * rr.LOOP_RECORD, d_tx.ptr, 0, None) == c.COMMS_OK
    c.NoiseSource(cr.LOOP_SEED).set_input_format("i16", 1.0).awgn_dev(d_tx.ptr, n_sym, sigma, d_rx.ptr)
    deframe = c.DeframeNode(rr.LOOP_F, 0, 0).set_output_format("llr").set_llr_scale(0.5 / sigma ** 2)
    det = np.zeros(frames, c.FRAME_DETECTION_DTYPE)
    det["index"], det["corr_re"], det["metric"] = np.arange(frames) * rr.LOOP_SYMS, 1.0, 1.0
    d_llr, d_dem, d_bits = c.DeviceBuf(frames * 4 * E), c.DeviceBuf(frames * 4 * N), c.DeviceBuf(frames * dec.out_frame_bytes)
    assert deframe.run_dev(d_rx.ptr, n_sym, det, d_llr.ptr, frames) == frames
    dematch.run_dev(d_llr.ptr, frames, d_dem.ptr)
    dec.run_dev(d_dem.ptr, frames, d_bits.ptr)
    d_out, d_pass, d_crc = c.DeviceBuf(frames * chk.out_frame_bytes), c.DeviceBuf(4 * frames), c.DeviceBuf(4 * frames)
    d_failed = c.DeviceBuf(4).upload(np.zeros(1, np.uint32))
    chk.run_dev(d_bits.ptr, frames, d_out.ptr, d_pass.ptr, d_crc.ptr, d_failed.ptr)
    # what the host sees afterwards
    payload = cr.unpack_records(d_payload.download(np.uint8, frames * cr.LOOP_RECORD).reshape(frames, -1), T)
    assert np.array_equal(payload, cr.loop_payload())
    sent = cr.ref_attach(payload, p)
    assert np.array_equal(d_frame.download(np.uint8, frames * att.out_frame_bytes).reshape(frames, -1), cr.pack_records(sent))
    llr = d_llr.download(np.float32, frames * E).reshape(frames, -1)
    decoded = cr.unpack_records(d_bits.download(np.uint8, frames * dec.out_frame_bytes).reshape(frames, -1), rr.LOOP_T)
    want_bits, want_payload, want_pass, want_crc = cr.loop_decode(llr, point)
    assert np.array_equal(decoded, want_bits)                               # viterbi_ref on the downloaded LLRs
    passed = d_pass.download(np.int32, frames)
    failed = int(d_failed.download(np.uint32, 1)[0])
    same = np.all(decoded == sent, axis=1)
    print("Es/N0 %.1f dB: %d of %d frames pass, %d equal the sent frame, n_failed %d" % (point.esn0_db, passed.sum(), frames, same.sum(), failed))
    assert np.array_equal(passed, want_pass)                                # crc_ref on the decoded bits
    assert np.array_equal(d_crc.download(np.uint32, frames), want_crc)
    assert np.array_equal(d_out.download(np.uint8, frames * chk.out_frame_bytes).reshape(frames, -1), cr.pack_records(want_payload))
    assert np.array_equal(passed == 1, same)                                # the receiver's verdict is the truth, frame by frame
    assert failed == int(np.count_nonzero(passed == 0))
    if point == cr.LOOP_CLEAN:
        assert passed.all() and failed == 0
    else:
        assert frames // 4 <= failed <= frames - frames // 4                # both outcomes occur
    model = cr.loop_model(point)[2]
    assert np.max(np.abs(model - llr)) < 1e-4 * np.max(np.abs(model))       # test_crc_ref.py's model is this channel


# ------------------------------------------------------------------ 7. refusals
def test_refusals_leave_nothing_behind(c):
    lib = c.lib()
    # (width, poly, init, xorout, n_payload_bits)
    bad = [(0, 0, 0, 0, 8), (33, 0x04C11DB7, 0, 0, 8), (-1, 1, 0, 0, 8),
           (8, 0x107, 0, 0, 8), (8, 0x07, 0x100, 0, 8), (8, 0x07, 0, 0x100, 8), (1, 2, 0, 0, 8), (31, 1 << 31, 0, 0, 8),
           (8, 0x07, 0, 0, 0),
           (8, 0x07, 0, 0, (1 << 16) - 8 + 1), (32, 0x04C11DB7, 0, 0, (1 << 16) - 31), (1, 1, 0, 0, 1 << 16), (8, 0x07, 0, 0, 1 << 40)]
    for width, poly, init, xorout, T in bad:
        h = C.c_void_p(0xDEAD)
        assert lib.comms_crc_create(width, poly, init, xorout, T, 0, C.byref(h)) == c.COMMS_ERR_ARG, (width, poly, init, xorout, T)
        assert not h.value                                                 # no handle, nothing to destroy
    assert "2^16" in lib.comms_last_error().decode()
    assert lib.comms_crc_create(8, 0x07, 0, 0, 8, 0, None) == c.COMMS_ERR_ARG
    with pytest.raises(c.CommsError) as e:
        c.CrcAttachNode(8, 0x107, 0, 0, 8)
    assert e.value.code == c.COMMS_ERR_ARG
    for W in (1, 8, 32):                                                   # the limits themselves are allowed
        c.CrcCheckNode(W, 1, 0, 0, (1 << 16) - W)
    c.CrcAttachNode(32, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 1)
    p, T = cr.SHAPE_PARAMS[16], 70
    att, chk = nodes_of(c, p, T)
    pin, cod = att.in_frame_bytes, att.out_frame_bytes                      # 12 and 12 bytes
    buf = c.DeviceBuf(8192)
    for args in ((buf.ptr + 2, 1, buf.ptr + 4096), (buf.ptr, 1, buf.ptr + 4097), (None, 1, buf.ptr), (buf.ptr, 1, None),
                 (buf.ptr, 2, buf.ptr + 2 * pin - 4), (buf.ptr + 2 * cod - 4, 2, buf.ptr), (buf.ptr, 1, buf.ptr)):
        assert lib.comms_crc_attach_run_dev(att._h, args[0], args[1], args[2], None) == c.COMMS_ERR_ARG, args
    far = [buf.ptr + 1024 * k for k in (1, 2, 3, 4)]
    for k in range(4):                                                     # each output in turn: misaligned, overlapping
        for wrong in (far[k] + 2, buf.ptr + 4, buf.ptr):
            outs = list(far)
            outs[k] = wrong
            assert lib.comms_crc_check_run_dev(chk._h, buf.ptr, 2, outs[0], outs[1], outs[2], outs[3], None) == c.COMMS_ERR_ARG, (k, wrong - buf.ptr)
    for i, k in itertools.combinations(range(4), 2):                       # two outputs that overlap one another
        outs = list(far)
        outs[k] = outs[i]
        assert lib.comms_crc_check_run_dev(chk._h, buf.ptr, 2, outs[0], outs[1], outs[2], outs[3], None) == c.COMMS_ERR_ARG, (i, k)
    assert lib.comms_crc_check_run_dev(chk._h, buf.ptr + 1, 1, *far, None) == c.COMMS_ERR_ARG
    assert lib.comms_crc_check_run_dev(chk._h, None, 1, *far, None) == c.COMMS_ERR_ARG
    assert lib.comms_crc_check_run_dev(None, buf.ptr, 1, *far, None) == c.COMMS_ERR_ARG
    assert lib.comms_crc_attach_run_dev(None, buf.ptr, 1, far[0], None) == c.COMMS_ERR_ARG
    assert lib.comms_crc_attach_run(att._h, None, 1, None) == c.COMMS_ERR_ARG
    assert lib.comms_crc_check_run(chk._h, None, 1, None, None, None, None) == c.COMMS_ERR_ARG
    assert lib.comms_crc_payload_frame_bytes(None) == 0 and lib.comms_crc_coded_frame_bytes(None) == 0
    name = C.create_string_buffer(240)
    assert lib.comms_crc_get_kernel(att._h, 2, 1, name, 240) == c.COMMS_ERR_ARG
    assert lib.comms_crc_set_timer(None, None) == c.COMMS_ERR_ARG
    # adjacent records are not overlapping ones, and the handles still work after the refused calls
    assert lib.comms_crc_attach_run_dev(att._h, buf.ptr, 2, buf.ptr + 2 * pin, None) == c.COMMS_OK
    assert lib.comms_crc_check_run_dev(chk._h, buf.ptr, 2, buf.ptr + 2 * cod, None, None, None, None) == c.COMMS_OK
    round_trip(c, p, T, 2, 1, (att, chk))


# ------------------------------------------------------------------ 8. host graph
def test_host_graph_nodes(c):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "comms_rs_amd", "host"), "-s"], timeout=600)
    out = subprocess.run([os.path.join(ROOT, "comms_rs_amd", "lib", "test_crc_nodes_gpu")], capture_output=True,
                         text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all passed" in out.stdout
