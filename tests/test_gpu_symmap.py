"""GPU tests of the symbol mapper and the soft demapper (comms_symmap_*, comms_demap_*; symmap_kernel, demap_table_kernel,
demap_axis_kernel) against tests/symmap_ref.py, the brute-force definition of the header.  Every stage is an exact contract, so
every comparison is equality: symbols and bits as bytes, LLRs as uint32 with NaN matching NaN by position.
tests/test_symmap_ref.py checks the reference itself.  Run with -m gpu."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import symmap_ref as sr

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


def guarded(c, nbytes):
    """A 0xFF-filled device buffer of nbytes with a guard region behind it."""
    return c.DeviceBuf(nbytes + GUARD).upload(np.full(nbytes + GUARD, 0xFF, np.uint8))


def unguard(buf, nbytes):
    raw = buf.download(np.uint8, nbytes + GUARD)
    assert np.all(raw[nbytes:] == 0xFF), "the guard region was written"
    return raw[:nbytes]


def map_dev(c, node, records, frames):
    d_in = c.DeviceBuf(max(records.nbytes, 4)).upload(records)
    d_out = guarded(c, frames * node.out_frame_bytes)
    node.run_dev(d_in.ptr, frames, d_out.ptr)
    return unguard(d_out, frames * node.out_frame_bytes).view(np.complex64).reshape(frames, -1)


def demap_dev(c, node, z, frames):
    """run_dev into a guarded buffer; returns float32 (frames, F m) or uint8 (frames, record bytes)."""
    d_in = c.DeviceBuf(max(z.nbytes, 8)).upload(z)
    nbytes = frames * node.out_frame_bytes
    d_out = guarded(c, nbytes)
    node.run_dev(d_in.ptr, frames, d_out.ptr)
    raw = unguard(d_out, nbytes)
    return raw.view(np.float32).reshape(frames, -1) if node.format == "llr" else raw.reshape(frames, -1)


def same_bytes(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ 1. the mapper
@pytest.mark.parametrize("m", range(1, 9))
def test_mapper_equals_the_table_copy(c, m):
    """Fields straddle words at m = 3, 5, 6, 7; E = 1, 31, 33 and lengths that m does not divide; dirty padding bits; with and
    without a word and a gap; no frames, one, several."""
    table = sr.random_table(m, 40 + m)
    word = sr.noisy_points(sr.QPSK, 13, m)
    for i, E in enumerate((1, 31, 33, 32 * m + 1, 95 + m)):
        for P, G in ((0, 0), (13, 5)) if i % 2 else ((13, 0), (0, 5)):
            node = c.SymbolMapNode(m, table, E, word[:P] if P else None, G)
            F = -(-E // m)
            assert node.in_frame_bytes == sr.record_bytes(E) and node.out_frame_syms == P + F + G
            for frames in (1, 7):
                bits = np.random.default_rng(E + frames).integers(0, 2, (frames, E), dtype=np.uint8)
                want = sr.ref_map(bits, m, table, word[:P], G)
                got = map_dev(c, node, sr.dirty_records(bits, E), frames)
                assert same_bytes(got, want), (m, E, P, G, frames, np.argwhere(got != want)[:4])
            assert same_bytes(node.run(sr.dirty_records(bits, 3)), want)
            node.run_dev(None, 0, None)
            assert node.run(np.zeros((0, node.in_frame_bytes), np.uint8)).shape == (0, P + F + G)
    assert any(E % m for E in (1, 31, 33, 32 * m + 1, 95 + m)) or m == 1
    k = node.kernel(3)
    f = fields(k)
    assert k.startswith("symmap_kernel") and f["wg"] == sr.WG and f["bits"] == m and f["syms"] == 3 * node.out_frame_syms and f["lds"] == 2048, k


def test_mapper_default_tables_are_digital_rs(c):
    for m, table in ((1, sr.BPSK), (2, sr.QPSK)):
        bits = np.random.default_rng(m).integers(0, 2, (2, 37), dtype=np.uint8)
        assert same_bytes(c.SymbolMapNode(m, None, 37).run(sr.pack_records(bits)), sr.ref_map(bits, m, table))
    assert same_bytes(c.SymbolMapNode(4, c.qam_table(4), 37).run(sr.pack_records(bits)), sr.ref_map(bits, 4, sr.qam_table(4)))


def test_mapper_lanes_make_several_passes(c):
    m, E, P, G = 3, 100, 13, 5
    table, word = sr.psk_table(3), sr.noisy_points(sr.QPSK, P, 1)
    node = c.SymbolMapNode(m, table, E, word, G)
    k = fields(node.kernel(10 ** 7))
    assert k["grid"] == k["max_grid"] == sr.GRID_CAP
    frames = 2 * k["grid"] * k["wg"] // node.out_frame_syms + 77
    kk = fields(node.kernel(frames))
    assert kk["syms"] > 2 * kk["grid"] * kk["wg"] and kk["grid"] == kk["max_grid"]
    bits = np.random.default_rng(7).integers(0, 2, (frames, E), dtype=np.uint8)
    got = map_dev(c, node, sr.dirty_records(bits, 8), frames)
    assert same_bytes(got, sr.ref_map(bits, m, table, word, G))


# ------------------------------------------------------------------ 2. the demapper
def nodes_of(c, name, F):
    m, table, given, split = sr.table_of(name)
    return m, table, split, c.DemapNode(m, given, F), c.DemapNode(m, given, F, force_table=True)


@pytest.mark.parametrize("name", list(sr.tables()))
def test_demapper_equals_the_brute_force(c, name):
    """Both formats and both kernel forms on noisy table points plus the adversarial set, at the lengths that reach the word
    seams; the forced-table handle and the default one give the same bytes and name different forms where the table is
    separable; LLR signs agree with the hard bits; the format switches between calls on one handle."""
    for F in sr.demap_lengths(sr.table_of(name)[0]):
        m, table, split, node, forced = nodes_of(c, name, F)
        kd, kf = node.kernel(2), forced.kernel(2)
        assert "form=table" in kf and kf.startswith("demap_table_kernel<%d,llr>" % m), kf
        if split is None:
            assert kd == kf
        else:
            assert "form=axis" in kd and kd.startswith("demap_axis_kernel<%d,%d,llr>" % split), kd
            assert fields(kd)["points"] == (1 << split[0]) + (1 << split[1]) and fields(kf)["points"] == 1 << m
        assert node.in_frame_bytes == 8 * F
        for frames in (1, 3):
            z = sr.demap_input(table, frames * F, 1000 * F + frames)
            want_llr = sr.ref_llr_records(z, table, F, 0.37)
            want_bits = sr.ref_bits_records(z, table, F)
            for h in (node, forced):
                h.set_llr_scale(0.37)
                assert h.out_frame_bytes == 4 * F * m
                got_llr = demap_dev(c, h, z, frames)
                assert sr.same_floats(got_llr, want_llr), (name, F, frames, h.kernel(frames))
                h.set_output_format("bits")                                    # the same handle, the other format
                assert h.out_frame_bytes == sr.record_bytes(F * m) and ",bits>" in h.kernel(frames)
                got_bits = demap_dev(c, h, z, frames)
                assert same_bytes(got_bits, want_bits), (name, F, frames, h.kernel(frames), np.argwhere(got_bits != want_bits)[:4])
                h.set_output_format("llr")
                bit = sr.unpack_records(got_bits, F * m)
                assert np.all(bit[got_llr > 0] == 0) and np.all(bit[got_llr < 0] == 1)
        assert sr.same_floats(node.run(z), got_llr)
        node.run_dev(None, 0, None)
        assert node.run(np.zeros(0, np.complex64)).shape == (0, F * m)


@pytest.mark.parametrize("name", ["8psk", "16qam"])
def test_demapper_lanes_make_several_passes(c, name):
    F = 67
    m, table, split, node, forced = nodes_of(c, name, F)
    k = fields(node.kernel(10 ** 7))
    assert k["grid"] == k["max_grid"] == sr.GRID_CAP
    frames = k["grid"] * k["wg"] // F + 300
    z = np.resize(sr.demap_input(table, 50000, 5), frames * F)
    want_llr, want_bits = sr.ref_llr_records(z, table, F), sr.ref_bits_records(z, table, F)
    for h in (node, forced):
        kk = fields(h.kernel(frames))
        assert kk["items"] > kk["grid"] * kk["wg"] and kk["grid"] == kk["max_grid"]
        assert sr.same_floats(demap_dev(c, h, z, frames), want_llr)
        h.set_output_format("bits")
        kk = fields(h.kernel(frames))
        assert kk["items"] == 2 * frames and kk["lanes"] > kk["grid"] * kk["wg"]
        assert same_bytes(demap_dev(c, h, z, frames), want_bits)


def test_timers_and_refusals_at_run(c):
    lib = c.lib()
    node, mapper = c.DemapNode(4, sr.qam_table(4), 16), c.SymbolMapNode(4, sr.qam_table(4), 64)
    buf = c.DeviceBuf(8192)
    for args in ((buf.ptr + 4, 1, buf.ptr + 4096), (buf.ptr, 1, buf.ptr + 4096 + 8), (None, 1, buf.ptr), (buf.ptr, 1, None),
                 (buf.ptr, 1, buf.ptr), (buf.ptr, 2, buf.ptr + 128)):
        assert lib.comms_demap_run_dev(node._h, args[0], args[1], args[2], None) == c.COMMS_ERR_ARG, args
    for args in ((buf.ptr + 2, 1, buf.ptr + 4096), (buf.ptr, 1, buf.ptr + 4096 + 4), (None, 1, buf.ptr), (buf.ptr, 1, None), (buf.ptr, 1, buf.ptr)):
        assert lib.comms_symmap_run_dev(mapper._h, args[0], args[1], args[2], None) == c.COMMS_ERR_ARG, args
    assert lib.comms_demap_run_dev(None, buf.ptr, 1, buf.ptr + 4096, None) == c.COMMS_ERR_ARG
    assert lib.comms_symmap_run_dev(None, buf.ptr, 1, buf.ptr + 4096, None) == c.COMMS_ERR_ARG
    assert lib.comms_demap_set_output_format(node._h, c._lib.SYM_C32) == c.COMMS_ERR_ARG
    assert lib.comms_demap_set_llr_scale(node._h, C.c_float(float("inf"))) == c.COMMS_ERR_ARG
    assert lib.comms_demap_run_dev(node._h, buf.ptr, 2, buf.ptr + 256, None) == c.COMMS_OK      # adjacent is not overlapping
    z = sr.demap_input(sr.qam_table(4), 32, 1)
    bits = np.random.default_rng(1).integers(0, 2, (2, 64), dtype=np.uint8)
    for h, call in ((node, lambda: node.run(z)), (mapper, lambda: mapper.run(sr.pack_records(bits)))):
        timer = c.KernelTimer(4).attach(h)
        call()
        call()
        ms = timer.read_ms()
        assert ms.size == 2 and np.all(ms > 0) and np.all(ms < 100)
        timer.close()


# ------------------------------------------------------------------ 3. ties to the existing nodes
@pytest.mark.parametrize("m", [1, 2])
def test_at_one_and_two_bits_the_demapper_is_the_deframers_rule(c, m):
    """DemapNode on a DeframeNode's C32 records equals that deframer's LLR and BITS records and comms_sym_to_bits_dev on the same
    symbols, bit for bit."""
    F, frames, gap = 45, 6, 3
    table = sr.default_table(m)
    with np.errstate(invalid="ignore"):                                       # (the input holds NaN and infinite symbols)
        y = (sr.demap_input(table, frames * (F + gap), 3) * np.complex64(0.6 + 0.3j)).astype(np.complex64)
    det = np.zeros(frames, c.FRAME_DETECTION_DTYPE)
    det["index"], det["corr_re"], det["corr_im"], det["metric"] = np.arange(frames) * (F + gap), 0.8, -0.45, 1.0
    out = {}
    for fmt in ("c32", "llr", "bits"):
        d = c.DeframeNode(F, 0, 0, bits_per_sym=m, normalise=True, word_energy=1.3).set_output_format(fmt).set_llr_scale(1.7)
        out[fmt] = d.run(y, det)
        assert out[fmt].shape[0] == frames
    z = np.ascontiguousarray(out["c32"]).ravel()
    node = c.DemapNode(m, None, F).set_llr_scale(1.7)
    assert "form=axis" in node.kernel(1)
    assert sr.same_floats(demap_dev(c, node, z, frames), out["llr"])
    assert sr.same_floats(out["llr"], sr.ref_llr_records(z, table, F, 1.7))
    node.set_output_format("bits")
    got = demap_dev(c, node, z, frames)
    assert same_bytes(got, out["bits"])
    flat = c.DemapNode(m, None, frames * F).set_output_format("bits")      # any flat stream is one frame
    assert flat.run(z).tobytes()[: (frames * F * m + 7) // 8] == c.sym_to_bits(z, m).tobytes()


# ------------------------------------------------------------------ 4. round trip
@pytest.mark.parametrize("name", ["bpsk", "qpsk", "8psk", "16qam", "rand5", "64qam", "256qam"])
def test_demapped_mapper_output_is_the_input_bits(c, name):
    m, table, given, _ = sr.table_of(name)
    E, frames = 32 * m + 5, 4
    bits = np.random.default_rng(m).integers(0, 2, (frames, E), dtype=np.uint8)
    mapper = c.SymbolMapNode(m, given, E)
    F = mapper.out_frame_syms
    sym = mapper.run(sr.dirty_records(bits, 2))
    got = c.DemapNode(m, given, F).set_output_format("bits").run(sym)
    padded = np.zeros((frames, F * m), np.uint8)
    padded[:, :E] = bits
    assert same_bytes(got, sr.pack_records(padded))


# ------------------------------------------------------------------ 5. the coded link
def test_coded_link_over_16qam(c):
    """CRC-24 -> K = 7 encoder -> rate 3/4 matcher -> 16-QAM mapper with a 13-symbol word; noise and a rotation on the host;
    FrameSyncNode -> DeframeNode (C32, normalising) -> DemapNode -> RateDematchNode -> ViterbiNode -> CrcCheckNode.  Every
    intermediate record equals the same chain on the Python references."""
    f = sr.link_format()
    p, frames, P = f["p"], sr.LINK_FRAMES, sr.LINK_WORD.size
    payload, framed, coded, sent, sym = sr.link_transmit()
    att = c.CrcAttachNode(p.W, p.poly, p.init, p.xorout, sr.LINK_T)
    enc = c.ConvEncoderNode(f["info"])
    match = c.RateMatchNode(f["N"], f["pattern"])
    mapper = c.SymbolMapNode(sr.LINK_M, c.qam_table(sr.LINK_M), f["E"], sr.LINK_WORD, sr.LINK_GAP)
    assert match.n_tx_bits == f["E"] and mapper.in_frame_bytes == match.out_frame_bytes and mapper.out_frame_syms == f["rec"]
    d = [c.DeviceBuf(frames * n) for n in (att.in_frame_bytes, att.out_frame_bytes, enc.out_frame_bytes, match.out_frame_bytes,
                                           mapper.out_frame_bytes)]
    d[0].upload(sr.pack_records(payload))
    att.run_dev(d[0].ptr, frames, d[1].ptr)
    enc.run_dev(d[1].ptr, frames, d[2].ptr)
    match.run_dev(d[2].ptr, frames, d[3].ptr)
    mapper.run_dev(d[3].ptr, frames, d[4].ptr)
    for buf, want in zip(d[1:4], (framed, coded, sent)):
        assert same_bytes(buf.download(np.uint8, frames * sr.record_bytes(want.shape[1])).reshape(frames, -1), sr.pack_records(want))
    tx = d[4].download(np.complex64, frames * f["rec"]).reshape(frames, -1)
    assert same_bytes(tx, sym)
    y = sr.link_channel(tx)                                                  # host: the gain, the rotation, the seeded noise
    # receive
    sync = c.FrameSyncNode(sr.LINK_WORD, sr.LINK_THRESHOLD, sr.LINK_GUARD)
    deframe = c.DeframeNode(f["F"], P, sr.LINK_GUARD, normalise=True, word_energy=float(np.sum(np.abs(sr.LINK_WORD) ** 2)))
    demap = c.DemapNode(sr.LINK_M, c.qam_table(sr.LINK_M), f["F"]).set_llr_scale(0.5 / sr.LINK_SIGMA ** 2)
    dematch = c.RateDematchNode(f["N"], f["pattern"], record_llrs=f["F"] * sr.LINK_M)
    dec = c.ViterbiNode(f["info"], qscale=sr.LINK_QSCALE)
    chk = c.CrcCheckNode(p.W, p.poly, p.init, p.xorout, sr.LINK_T)
    d_y = c.DeviceBuf(y.nbytes).upload(y)
    dets = sync.run_dev(d_y.ptr, y.size, raw=True)
    assert [int(i) for i in dets["index"]] == [k * f["rec"] for k in range(frames)]
    d_z, d_llr = c.DeviceBuf(frames * 8 * f["F"]), c.DeviceBuf(frames * demap.out_frame_bytes)
    d_dem, d_bits = c.DeviceBuf(frames * 4 * f["N"]), c.DeviceBuf(frames * dec.out_frame_bytes)
    d_out, d_pass, d_crc = c.DeviceBuf(frames * chk.out_frame_bytes), c.DeviceBuf(4 * frames), c.DeviceBuf(4 * frames)
    d_failed = c.DeviceBuf(4).upload(np.zeros(1, np.uint32))
    assert deframe.run_dev(d_y.ptr, y.size, dets, d_z.ptr, frames) == frames
    demap.run_dev(d_z.ptr, frames, d_llr.ptr)
    dematch.run_dev(d_llr.ptr, frames, d_dem.ptr)
    dec.run_dev(d_dem.ptr, frames, d_bits.ptr)
    chk.run_dev(d_bits.ptr, frames, d_out.ptr, d_pass.ptr, d_crc.ptr, d_failed.ptr)
    z = d_z.download(np.complex64, frames * f["F"]).reshape(frames, -1)
    ideal = (y.reshape(frames, -1)[:, P: P + f["F"]].astype(np.complex128) / sr.LINK_GAIN)
    # the deframer brought the payload to the table's scale: what remains is the error of the 13-symbol channel estimate,
    # relative standard deviation sigma sqrt(2) / sqrt(Ep) = 0.042, on symbols of magnitude up to about 5.2 -- five of them
    assert np.max(np.abs(z - ideal)) < 5 * sr.LINK_SIGMA * np.sqrt(2.0 / np.sum(np.abs(sr.LINK_WORD) ** 2)) * 5.2
    want_llr, want_words, want_decoded, (want_payload, want_pass, want_crc) = sr.link_receive(z)
    assert sr.same_floats(d_llr.download(np.float32, want_llr.size).reshape(frames, -1), want_llr)
    assert same_bytes(d_dem.download(np.uint32, frames * f["N"]).reshape(frames, -1), want_words)
    got_bits = sr.unpack_records(d_bits.download(np.uint8, frames * dec.out_frame_bytes).reshape(frames, -1), f["info"])
    assert np.array_equal(got_bits, want_decoded)
    assert np.array_equal(d_pass.download(np.int32, frames), want_pass) and np.array_equal(d_crc.download(np.uint32, frames), want_crc)
    assert same_bytes(d_out.download(np.uint8, frames * chk.out_frame_bytes).reshape(frames, -1), sr.pack_records(want_payload))
    assert want_pass.all() and int(d_failed.download(np.uint32, 1)[0]) == 0 and np.array_equal(want_payload, payload)


# ------------------------------------------------------------------ 7. host graph
def test_host_graph_nodes(c):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "comms_rs_amd", "host"), "-s"], timeout=600)
    out = subprocess.run([os.path.join(ROOT, "comms_rs_amd", "lib", "test_symmap_nodes_gpu")], capture_output=True,
                         text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all passed" in out.stdout
