"""GPU tests of the rate-matching nodes (comms_ratematch_*; ratematch_tx_kernel, ratematch_rx_kernel) against
tests/ratematch_ref.py.  Only bits and words move, so every record is compared for equality (LLRs as uint32);
tests/test_ratematch_ref.py checks the reference itself and pins the noisy point of the loop.  Run with -m gpu."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ratematch_ref as rr
import viterbi_ref as vr

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


def nodes_of(c, N, pattern, cols=0, perm=None, scr=None, record_llrs=0):
    packed = None if scr is None else rr.pack_bits(scr)
    return (c.RateMatchNode(N, pattern, cols, perm, packed), c.RateDematchNode(N, pattern, cols, perm, packed, record_llrs=record_llrs))


def run_dev_guarded(c, run_dev, data, frames, out_bytes):
    """run_dev on uploaded records into a 0xFF-filled buffer with a guard region behind it: the records as uint8 rows."""
    d_in = c.DeviceBuf(max(data.nbytes, 4)).upload(data)
    d_out = c.DeviceBuf(frames * out_bytes + GUARD).upload(np.full(frames * out_bytes + GUARD, 0xFF, np.uint8))
    run_dev(d_in.ptr, frames, d_out.ptr)
    raw = d_out.download(np.uint8, frames * out_bytes + GUARD)
    assert np.all(raw[frames * out_bytes:] == 0xFF), "the guard region was written"
    return raw[: frames * out_bytes].reshape(frames, out_bytes)


def check_tx(c, node, N, src, scr, frames, seed):
    """Random coded bits with every bit from N on set to 1 in the input records."""
    E = src.size
    assert node.n_tx_bits == E and node.in_frame_bytes == rr.record_bytes(N) and node.out_frame_bytes == rr.record_bytes(E)
    assert np.array_equal(node.map(), src)
    bits = np.random.default_rng(seed).integers(0, 2, (frames, N), dtype=np.uint8)
    dirty = rr.pack_records(bits) | ~rr.pack_records(np.ones((frames, N), np.uint8))
    want = rr.pack_records(rr.ref_tx(bits, src, scr))                      # padding bits and bytes 0
    got = run_dev_guarded(c, node.run_dev, dirty, frames, node.out_frame_bytes)
    assert np.array_equal(got, want), (N, E, frames, int(np.count_nonzero(rr.unpack_records(got, E) != rr.unpack_records(want, E))))
    return dirty, want


def check_rx(c, node, N, src, scr, frames, seed, record=None):
    """Records with NaN payloads, infinities, zeros and denormals in the used part, and NaN behind it where they are longer."""
    E = src.size
    record = E if record is None else record
    assert node.in_frame_bytes == 4 * record and node.out_frame_bytes == 4 * N
    words = rr.llr_words(frames, record, E, seed)
    want = rr.ref_rx(words, src, N, scr)
    got = run_dev_guarded(c, node.run_dev, words, frames, 4 * N).view(np.uint32)
    assert np.array_equal(got, want), (N, E, frames, int(np.count_nonzero(got != want)))
    return words, want


# ------------------------------------------------------------------ 1. + 2. every format, both directions, dirty input
@pytest.mark.parametrize("name", list(rr.PATTERNS))
def test_both_directions_are_the_reference_bit_for_bit(c, name):
    pattern = rr.PATTERNS[name]
    i = 0
    for N in rr.coded_lengths(pattern):
        E = rr.n_tx_bits(N, pattern)
        for cols, perm in rr.interleavers(E, N):
            i += 1
            frames = 1 + i % 3
            scr = rr.scramble_bits(E, N + i) if i % 2 else None
            src, _ = rr.build_map(N, pattern, cols, perm)
            wide = E + 5 if i % 4 == 0 else 0                              # receive records longer than E, NaN behind
            tx, rx = nodes_of(c, N, pattern, cols, perm, scr, wide)
            check_tx(c, tx, N, src, scr, frames, i)
            check_rx(c, rx, N, src, scr, frames, i, wide or E)
            k = tx.kernel(frames)
            assert k.startswith("ratematch_tx_kernel") and "table=lds" in k and fields(k)["seam"] == rr.LDS_SEAM, k
            k = rx.kernel(frames)
            assert k.startswith("ratematch_rx_kernel") and "table=lds" in k and fields(k)["values"] == frames * N, k


def test_scramble_on_every_interleaver_and_plain(c):
    """The parity of the case counter above couples scramble to some forms; here every form runs with and without it."""
    N, pattern = 140, rr.PATTERNS["3/4"]
    E = rr.n_tx_bits(N, pattern)
    for j, (cols, perm) in enumerate(rr.interleavers(E, 3)):
        for scr in (None, rr.scramble_bits(E, j)):
            src, _ = rr.build_map(N, pattern, cols, perm)
            tx, rx = nodes_of(c, N, pattern, cols, perm, scr)
            check_tx(c, tx, N, src, scr, 3, j)
            check_rx(c, rx, N, src, scr, 3, j)


def test_special_values_keep_their_bits(c):
    """Every special word at every scramble value: NaN payloads, +-inf, +-0.0 and denormals differ in the sign bit at most."""
    N = 2 * rr.SPECIAL.size
    scr = np.tile(np.array([0, 1], np.uint8), rr.SPECIAL.size)
    words = np.repeat(rr.SPECIAL, 2)[None, :].copy()
    src, _ = rr.build_map(N)
    _, rx = nodes_of(c, N, None, scr=scr)
    got = run_dev_guarded(c, rx.run_dev, words, 1, 4 * N).view(np.uint32)
    assert np.array_equal(got, words ^ (scr.astype(np.uint32) << 31)[None, :])
    assert np.array_equal(got, rr.ref_rx(words, src, N, scr))


# ------------------------------------------------------------------ 3. both table forms
def test_both_table_forms_at_the_seam(c):
    seam = fields(c.RateMatchNode(8).kernel(1))["seam"]
    assert seam == rr.LDS_SEAM
    p34 = rr.PATTERNS["3/4"]
    n_for_e = {E: next(N for N in range(E, 2 * E) if rr.n_tx_bits(N, p34) == E) for E in (seam, seam + 1)}
    # (N, pattern, table form on transmit (seam in E), on receive (seam in N))
    cases = [(seam, None, "lds", "lds"), (seam + 1, None, "global", "global"),
             (n_for_e[seam], p34, "lds", "global"), (n_for_e[seam + 1], p34, "global", "global")]
    for i, (N, pattern, tx_form, rx_form) in enumerate(cases):
        E = rr.n_tx_bits(N, pattern)
        scr = rr.scramble_bits(E, i)
        src, _ = rr.build_map(N, pattern, 17)
        tx, rx = nodes_of(c, N, pattern, 17, None, scr)
        for frames in (1, 3):
            check_tx(c, tx, N, src, scr, frames, i)
            check_rx(c, rx, N, src, scr, frames, i)
        kt, kr = tx.kernel(3), rx.kernel(3)
        assert "table=" + tx_form in kt and "table=" + rx_form in kr, (kt, kr)
        assert (fields(kt)["lds"] > 0) == (tx_form == "lds") and (fields(kr)["lds"] > 0) == (rx_form == "lds")
        assert fields(kt)["lds"] <= 4 * 32 * ((seam + 31) // 32) and fields(kr)["lds"] <= 4 * seam


def test_the_longest_frame(c):
    N, pattern = rr.MAX_CODED, rr.PATTERNS["7/8"]
    E = rr.n_tx_bits(N, pattern)
    perm = np.random.default_rng(1).permutation(E).astype(np.uint32)
    scr = rr.scramble_bits(E, 1)
    src, _ = rr.build_map(N, pattern, 0, perm)
    tx, rx = nodes_of(c, N, pattern, 0, perm, scr)
    check_tx(c, tx, N, src, scr, 1, 1)
    check_rx(c, rx, N, src, scr, 1, 1)
    assert "table=global" in tx.kernel(1) and fields(rx.kernel(1))["lds"] == 0
    # no pattern: E = N, the longest table on transmit
    src, _ = rr.build_map(N, None, 1000)
    tx, rx = nodes_of(c, N, None, 1000)
    check_tx(c, tx, N, src, None, 1, 2)
    check_rx(c, rx, N, src, None, 1, 2)


# ------------------------------------------------------------------ 4. lanes walk several items
def test_more_items_than_the_grid_has_lanes(c):
    N, pattern = 140, rr.PATTERNS["3/4"]                                    # E = 94: 3 words, two bits short of full
    E = rr.n_tx_bits(N, pattern)
    words = rr.record_bytes(E) // 4
    scr = rr.scramble_bits(E, 4)
    src, _ = rr.build_map(N, pattern, 17)
    tx, rx = nodes_of(c, N, pattern, 17, None, scr)
    k = fields(tx.kernel(10 ** 7))
    assert k["grid"] == k["max_grid"] and k["wg"] == rr.WG
    frames = k["grid"] * k["wg"] // words + 77
    assert fields(tx.kernel(frames))["words"] > k["grid"] * k["wg"]        # lanes walk several words
    check_tx(c, tx, N, src, scr, frames, 4)
    k = fields(rx.kernel(10 ** 7))
    assert k["grid"] == k["max_grid"]
    frames = k["grid"] * k["wg"] // N + 77
    assert fields(rx.kernel(frames))["values"] > k["grid"] * k["wg"]       # ... and several values
    check_rx(c, rx, N, src, scr, frames, 4)
    # the global form past its grid: a table of seam + 1 entries, more values than lanes
    N = rr.LDS_SEAM + 1
    src, _ = rr.build_map(N, None, 2)
    tx, rx = nodes_of(c, N, None, 2)
    frames = k["grid"] * k["wg"] // N + 3
    kk = fields(rx.kernel(frames))
    assert kk["values"] > kk["grid"] * kk["wg"] and kk["lds"] == 0
    check_rx(c, rx, N, src, None, frames, 5)
    check_tx(c, tx, N, src, None, 3, 5)


# ------------------------------------------------------------------ 5. host pointers, reuse, no frames, timers
def test_run_equals_run_dev_and_a_handle_is_stateless(c):
    N, pattern = 2012, rr.PATTERNS["5/6"]
    E = rr.n_tx_bits(N, pattern)
    scr = rr.scramble_bits(E, 8)
    src, _ = rr.build_map(N, pattern, 17)
    tx, rx = nodes_of(c, N, pattern, 17, None, scr, E + 3)
    dirty, want = check_tx(c, tx, N, src, scr, 3, 1)
    assert tx.run(dirty).tobytes() == want.tobytes()
    words, want_rx = check_rx(c, rx, N, src, scr, 3, 1, E + 3)
    assert rx.run(words.view(np.float32)).view(np.uint32).tobytes() == want_rx.tobytes()
    # other frames on the same handles equal fresh handles (check_* compare with the reference, which a fresh handle equals)
    check_tx(c, tx, N, src, scr, 2, 2)
    check_rx(c, rx, N, src, scr, 1, 2, E + 3)
    fresh_tx, fresh_rx = nodes_of(c, N, pattern, 17, None, scr, E + 3)
    dirty2, _ = check_tx(c, fresh_tx, N, src, scr, 2, 2)
    assert tx.run(dirty2).tobytes() == fresh_tx.run(dirty2).tobytes()
    words2 = rr.llr_words(2, E + 3, E, 9)
    assert rx.run(words2.view(np.float32)).tobytes() == fresh_rx.run(words2.view(np.float32)).tobytes()
    # no frames
    tx.run_dev(None, 0, None)
    rx.run_dev(None, 0, None)
    assert tx.run(np.zeros((0, tx.in_frame_bytes), np.uint8)).shape == (0, tx.out_frame_bytes)
    assert rx.run(np.zeros((0, E + 3), np.float32)).shape == (0, N)
    # one positive time per launch, in either direction
    for node, call in ((tx, lambda: tx.run(dirty)), (rx, lambda: rx.run(words.view(np.float32)))):
        timer = c.KernelTimer(4).attach(node)
        call()
        call()
        ms = timer.read_ms()
        assert ms.size == 2 and np.all(ms > 0) and np.all(ms < 100)
        timer.close()


# ------------------------------------------------------------------ 6. the loop on the device
def test_the_punctured_loop_on_the_device(c):
    """PRNS bits -> ConvEncoderNode -> RateMatchNode (3/4, 17 columns, PRNS scramble) -> QPSK -> AwgnNode (seeded) ->
    DeframeNode (LLR, one synthetic detection per frame) -> RateDematchNode -> ViterbiNode, nothing on the host in between."""
    frames, T, N, E = rr.LOOP_FRAMES, rr.LOOP_T, rr.LOOP_CODED, rr.LOOP_E
    mask, state, width = rr.LOOP_PRNS
    smask, sstate, swidth = rr.LOOP_SCRAMBLE_PRNS
    scr_packed = c.PrnsNode(smask, sstate, swidth).run_batch(E, packed=True)      # the sequence comes from the library's generator
    ref_packed, scr = rr.loop_scramble()
    assert np.array_equal(np.asarray(scr_packed, np.uint8)[: ref_packed.size], ref_packed)
    enc = c.ConvEncoderNode(T)
    match = c.RateMatchNode(N, rr.LOOP_PATTERN, rr.LOOP_COLS, scramble=ref_packed)
    dematch = c.RateDematchNode(N, rr.LOOP_PATTERN, rr.LOOP_COLS, scramble=ref_packed)
    assert match.in_frame_bytes == enc.out_frame_bytes and match.out_frame_bytes == rr.LOOP_RECORD and match.n_tx_bits == E
    n_sym = frames * rr.LOOP_SYMS
    d_info, d_coded, d_sent = c.DeviceBuf(frames * T // 8), c.DeviceBuf(frames * enc.out_frame_bytes), c.DeviceBuf(frames * rr.LOOP_RECORD)
    d_tx, d_rx = c.DeviceBuf(4 * n_sym), c.DeviceBuf(8 * n_sym)
    c.PrnsNode(mask, state, width).run_dev(frames * T, d_info.ptr, packed=True)
    enc.run_dev(d_info.ptr, frames, d_coded.ptr)
    match.run_dev(d_coded.ptr, frames, d_sent.ptr)
    assert c.lib().comms_qpsk_byte_mod_dev(d_sent.ptr, frames * rr.LOOP_RECORD, d_tx.ptr, 0, None) == c.COMMS_OK
    c.NoiseSource(rr.LOOP_SEED).set_input_format("i16", 1.0).awgn_dev(d_tx.ptr, n_sym, rr.LOOP_SIGMA, d_rx.ptr)
    deframe = c.DeframeNode(rr.LOOP_F, 0, 0).set_output_format("llr").set_llr_scale(rr.LOOP_LLR_SCALE)
    det = np.zeros(frames, c.FRAME_DETECTION_DTYPE)
    det["index"], det["corr_re"], det["metric"] = np.arange(frames) * rr.LOOP_SYMS, 1.0, 1.0
    assert deframe.frame_bytes() == dematch.in_frame_bytes == 4 * E
    d_llr, d_dem = c.DeviceBuf(frames * 4 * E), c.DeviceBuf(frames * 4 * N)
    assert deframe.run_dev(d_rx.ptr, n_sym, det, d_llr.ptr, frames) == frames
    dematch.run_dev(d_llr.ptr, frames, d_dem.ptr)
    dec = c.ViterbiNode(T, qscale=rr.LOOP_QSCALE)                           # record_llrs = 0: exactly n * steps
    assert dec.in_frame_bytes == dematch.out_frame_bytes
    d_bits = c.DeviceBuf(frames * dec.out_frame_bytes)
    dec.run_dev(d_dem.ptr, frames, d_bits.ptr)
    errs = c.bit_errors_dev(d_bits.ptr, d_info.ptr, frames * T)             # T is a multiple of 32: the records have no padding
    # what the host sees afterwards
    sent = vr.unpack_records(d_info.download(np.uint8, frames * T // 8).reshape(frames, -1), T)
    assert np.array_equal(sent, vr.loop_bits())
    coded = vr.ref_encode(sent, rr.LOOP_K, rr.LOOP_GENS, True)
    src, inv = rr.build_map(N, rr.LOOP_PATTERN, rr.LOOP_COLS)
    on_air = d_sent.download(np.uint8, frames * rr.LOOP_RECORD).reshape(frames, -1)
    assert np.array_equal(on_air, rr.pack_records(rr.ref_tx(coded, src, scr)))
    llr = d_llr.download(np.uint32, frames * E).reshape(frames, -1)
    dem = d_dem.download(np.uint32, frames * N).reshape(frames, -1)
    assert np.array_equal(dem, rr.ref_rx(llr, src, N, scr))
    got = vr.unpack_records(d_bits.download(np.uint8, frames * dec.out_frame_bytes).reshape(frames, -1), T)
    want, _ = vr.ref_decode(vr.ref_quantise(dem.view(np.float32), rr.LOOP_QSCALE), rr.LOOP_K, rr.LOOP_GENS, T, True)
    raw = int(np.count_nonzero((llr.view(np.float32) < 0) != (rr.ref_tx(coded, src, scr) == 1)))
    print("rate 3/4, Es/N0 %.1f dB: %d raw errors of %d transmitted bits, %d decoded errors of %d" % (rr.LOOP_ESN0_DB, raw, frames * E, errs, sent.size))
    assert np.array_equal(got, want)
    assert np.array_equal(got, sent) and errs == 0
    assert raw > 0
    # the model of tests/test_ratematch_ref.py is this channel: the same values but for rounding
    model = rr.loop_model()[2]
    assert np.max(np.abs(model - llr.view(np.float32))) < 1e-4 * np.max(np.abs(model))


# ------------------------------------------------------------------ 7. refusals
def test_refusals_leave_nothing_behind(c):
    lib = c.lib()
    u8 = lambda *v: (C.c_uint8 * len(v))(*v)                                # noqa: E731
    u32 = lambda *v: (C.c_uint32 * len(v))(*v)                              # noqa: E731
    p34 = u8(1, 1, 0, 1, 1, 0)
    long_pat = (C.c_uint8 * 257)(*([1] * 257))
    # (n_coded, pattern, pattern_len, cols, perm, record_llrs)
    bad = [(0, None, 0, 0, None, 0),                                       # N = 0
           ((3 << 16) + 1, None, 0, 0, None, 0),                           # N above 3 * 2^16
           (12, p34, 0, 0, None, 0),                                       # Lp = 0 with a pattern
           (12, None, 6, 0, None, 0),                                      # ... and a length without one
           (300, long_pat, 257, 0, None, 0),                               # Lp = 257
           (12, u8(1, 2, 0, 1), 4, 0, None, 0),                            # a pattern byte of 2
           (12, u8(0, 0, 0), 3, 0, None, 0),                               # all zero
           (2, u8(0, 0, 1), 3, 0, None, 0),                                # keeps no position below N
           (12, p34, 6, 9, None, 0),                                       # C > E = 8
           (12, p34, 6, 2, u32(0, 1, 2, 3, 4, 5, 6, 7), 0),                # perm together with cols
           (12, p34, 6, 0, u32(0, 1, 2, 3, 4, 5, 6, 6), 0),                # a repeat
           (12, p34, 6, 0, u32(0, 1, 2, 3, 4, 5, 6, 8), 0),                # a value >= E
           (12, p34, 6, 0, None, 7)]                                       # record_llrs < E
    for n_coded, pattern, lp, cols, perm, record in bad:
        h = C.c_void_p(0xDEAD)
        assert lib.comms_ratematch_create(n_coded, pattern, lp, cols, perm, None, record, 0, C.byref(h)) == c.COMMS_ERR_ARG, (n_coded, lp, cols, record)
        assert not h.value                                                 # no handle, nothing to destroy
    assert "record_llrs" in lib.comms_last_error().decode()
    assert lib.comms_ratematch_create(12, p34, 6, 0, None, None, 0, 0, None) == c.COMMS_ERR_ARG
    with pytest.raises(c.CommsError) as e:
        c.RateMatchNode(12, (1, 1, 0, 1, 1, 0), cols=9)
    assert e.value.code == c.COMMS_ERR_ARG
    with pytest.raises(ValueError):
        c.RateMatchNode(12, (1, 1, 0, 1, 1, 0), perm=np.arange(7))         # not one entry per transmitted bit
    c.RateMatchNode(3 << 16, cols=2)                                       # the limits themselves are allowed
    c.RateDematchNode(12, np.ones(256, np.uint8), cols=12, record_llrs=12)
    tx, rx = nodes_of(c, 140, rr.PATTERNS["3/4"], 17)
    fin, fout = tx.in_frame_bytes, tx.out_frame_bytes
    buf = c.DeviceBuf(8192)
    for args in ((buf.ptr + 2, 1, buf.ptr + 4096), (buf.ptr, 1, buf.ptr + 4097), (None, 1, buf.ptr), (buf.ptr, 1, None),
                 (buf.ptr, 2, buf.ptr + 2 * fin - 4), (buf.ptr + 2 * fout - 4, 2, buf.ptr), (buf.ptr, 1, buf.ptr)):
        assert lib.comms_ratematch_tx_run_dev(tx._h, args[0], args[1], args[2], None) == c.COMMS_ERR_ARG, args
    rin, rout = rx.in_frame_bytes, rx.out_frame_bytes
    for args in ((buf.ptr + 1, 1, buf.ptr + 4096), (buf.ptr, 1, buf.ptr + 4098), (None, 1, buf.ptr), (buf.ptr, 1, None),
                 (buf.ptr, 2, buf.ptr + 2 * rin - 4), (buf.ptr + 2 * rout - 4, 2, buf.ptr), (buf.ptr, 1, buf.ptr)):
        assert lib.comms_ratematch_rx_run_dev(rx._h, args[0], args[1], args[2], None) == c.COMMS_ERR_ARG, args
    assert lib.comms_ratematch_tx_run(tx._h, None, 1, None) == c.COMMS_ERR_ARG
    assert lib.comms_ratematch_rx_run(rx._h, None, 1, None) == c.COMMS_ERR_ARG
    assert lib.comms_ratematch_tx_run_dev(None, buf.ptr, 1, buf.ptr + 4096, None) == c.COMMS_ERR_ARG
    for size in ("n_tx_bits", "tx_in_frame_bytes", "tx_out_frame_bytes", "rx_in_frame_bytes", "rx_out_frame_bytes"):
        assert getattr(lib, "comms_ratematch_" + size)(None) == 0
    name = C.create_string_buffer(240)
    assert lib.comms_ratematch_get_kernel(tx._h, 2, 1, name, 240) == c.COMMS_ERR_ARG
    few = np.zeros(3, np.uint32)
    assert lib.comms_ratematch_get_map(tx._h, few.ctypes.data_as(C.c_void_p), 3) == c.COMMS_ERR_ARG
    # adjacent records are not overlapping ones, and the handles still work after the refused calls
    assert lib.comms_ratematch_tx_run_dev(tx._h, buf.ptr, 2, buf.ptr + 2 * fin, None) == c.COMMS_OK
    src, _ = rr.build_map(140, rr.PATTERNS["3/4"], 17)
    check_tx(c, tx, 140, src, None, 2, 1)
    check_rx(c, rx, 140, src, None, 2, 1)


# ------------------------------------------------------------------ 8. host graph
def test_host_graph_nodes(c):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "comms_rs_amd", "host"), "-s"], timeout=600)
    out = subprocess.run([os.path.join(ROOT, "comms_rs_amd", "lib", "test_ratematch_nodes_gpu")], capture_output=True,
                         text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all passed" in out.stdout
