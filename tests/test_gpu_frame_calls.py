"""The call shell of the per-frame nodes (csrc/common.hpp: FrameCall, check_frame_call), one row per node and direction at the
node's smallest format and 3 frames, all through run_dev on DeviceBufs: n_frames = 0 with NULL pointers is a no-op; NULL
pointers, misaligned pointers and overlapping input and output records with n_frames = 3 are refused with COMMS_ERR_ARG and
launch nothing (a KernelTimer on the handle counts the launches); after every refusal a correct call on the same handle
returns the records of the node's own reference (tests/*_ref.py).  No call here passes an unmapped pointer.
test_frame_run_shell holds the host form, run(), of the same rows to the same references: any shape of whole records, no
frames, and an input that is no whole number of records."""
import collections

import numpy as np
import pytest

import crc_ref as cr
import ldpc_ref as lr
import ofdm_ref as orf
import ratematch_ref as rr
import symmap_ref as sm
import viterbi_ref as vr

pytestmark = pytest.mark.gpu
FRAMES = 3

# node: the handle; x: the input records (any dtype, FRAMES rows); out_bytes: per frame; aligns: (input, output) in bytes;
# same(raw): the output bytes (uint8, FRAMES * out_bytes) against the reference
Row = collections.namedtuple("Row", "node x out_bytes aligns same")


@pytest.fixture(scope="module")
def c():
    import comms_rs_amd as c

    assert c.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested (no CPU fallback)"
    return c


def exact(want):
    want = np.ascontiguousarray(want)
    return lambda raw: raw.tobytes() == want.tobytes()


def convenc(c):
    K, n, T = 3, 2, 5
    bits = np.random.default_rng(1).integers(0, 2, (FRAMES, T), dtype=np.uint8)
    node = c.ConvEncoderNode(T, K, vr.GENS[(K, n)])
    return Row(node, vr.pack_records(bits), node.out_frame_bytes, (4, 4), exact(vr.pack_records(vr.ref_encode(bits, K, vr.GENS[(K, n)], True))))


def viterbi(c):
    vc = vr.make_case(3, 2, True, 6, FRAMES, "noisy")
    _, llr, bits, _ = vr.case_data(vc)
    node = c.ViterbiNode(vc.T, vc.K, vc.gens, terminated=vc.terminated, record_llrs=vc.record_llrs, qscale=vc.qscale)
    return Row(node, np.ascontiguousarray(llr, np.float32), node.out_frame_bytes, (4, 4), exact(vr.pack_records(bits)))


LDPC_Z = 2
LDPC_B = lr.make_base(3, 5, LDPC_Z, 51)             # the smallest base matrix of the encoder's form: T = 4, N = 10 bits


def ldpcenc(c):
    bits = np.random.default_rng(8).integers(0, 2, (FRAMES, 2 * LDPC_Z), dtype=np.uint8)
    node = c.LdpcEncoderNode(LDPC_B, LDPC_Z)
    return Row(node, lr.pack_records(bits), node.out_frame_bytes, (4, 4), exact(lr.pack_records(lr.ref_encode(bits, LDPC_B, LDPC_Z))))


def ldpcdec(c):
    """LLRs of random codewords, one of them with a wrong bit; the statuses are the decoder's own output and not in the row"""
    rng = np.random.default_rng(9)
    coded = lr.ref_encode(rng.integers(0, 2, (FRAMES, 2 * LDPC_Z), dtype=np.uint8), LDPC_B, LDPC_Z)
    llr = ((1.0 - 2.0 * coded) * rng.uniform(2.0, 9.0, coded.shape)).astype(np.float32)
    llr[1, 3] *= -0.25
    bits, _ = lr.ref_decode(lr.ref_quantise(llr, 4.0), LDPC_B, LDPC_Z)
    node = c.LdpcDecoderNode(LDPC_B, LDPC_Z, qscale=4.0)
    return Row(node, llr, node.out_frame_bytes, (4, 4), exact(lr.pack_records(bits)))


RM_N, RM_PATTERN = 8, rr.PATTERNS["3/4"]           # 6 of 8 coded bits are transmitted


def ratematch_tx(c):
    src, _ = rr.build_map(RM_N, RM_PATTERN)
    bits = np.random.default_rng(2).integers(0, 2, (FRAMES, RM_N), dtype=np.uint8)
    node = c.RateMatchNode(RM_N, RM_PATTERN)
    return Row(node, rr.pack_records(bits), node.out_frame_bytes, (4, 4), exact(rr.pack_records(rr.ref_tx(bits, src))))


def ratematch_rx(c):
    src, _ = rr.build_map(RM_N, RM_PATTERN)
    llr = np.random.default_rng(3).standard_normal((FRAMES, src.size)).astype(np.float32)
    node = c.RateDematchNode(RM_N, RM_PATTERN)
    return Row(node, llr, node.out_frame_bytes, (4, 4), exact(rr.ref_rx(llr.view(np.uint32), src, RM_N)))


CRC_P, CRC_T = cr.SHAPE_PARAMS[8], 9               # CRC-8 over 9 payload bits


def crc_attach(c):
    bits, dirty = cr.dirty_payload(FRAMES, CRC_T, 4)
    node = c.CrcAttachNode(CRC_P.W, CRC_P.poly, CRC_P.init, CRC_P.xorout, CRC_T)
    return Row(node, dirty, node.out_frame_bytes, (4, 4), exact(cr.pack_records(cr.ref_attach(bits, CRC_P))))


def crc_check(c):
    """the payload output alone: the call of the shell's input / primary-output pair"""
    node = c.CrcCheckNode(CRC_P.W, CRC_P.poly, CRC_P.init, CRC_P.xorout, CRC_T)
    full = np.zeros((FRAMES, 8 * node.in_frame_bytes), np.uint8)
    full[:, : CRC_T + CRC_P.W] = cr.ref_attach(cr.dirty_payload(FRAMES, CRC_T, 5)[0], CRC_P)
    full[1, 3] ^= 1                                 # one failed frame: its payload is written all the same
    want_payload, want_pass, _ = cr.ref_check(full, CRC_P, CRC_T)
    assert want_pass.tolist() == [1, 0, 1]
    return Row(node, np.packbits(full, axis=1, bitorder="little"), node.out_frame_bytes, (4, 4), exact(cr.pack_records(want_payload)))


def symmap(c):
    E = 33
    bits = np.random.default_rng(6).integers(0, 2, (FRAMES, E), dtype=np.uint8)
    node = c.SymbolMapNode(1, None, E)
    return Row(node, sm.dirty_records(bits, 1), node.out_frame_bytes, (4, 8), exact(sm.ref_map(bits, 1, sm.table_of("bpsk")[1], None, 0)))


def demap(c, fmt):
    F, table = 3, sm.table_of("bpsk")[1]
    z = sm.demap_input(table, FRAMES * F, 7).reshape(FRAMES, F)
    node = c.DemapNode(1, None, F).set_output_format(fmt)
    if fmt == "bits":
        return Row(node, z, node.out_frame_bytes, (8, 16), exact(sm.ref_bits_records(z.ravel(), table, F)))
    want = sm.ref_llr_records(z.ravel(), table, F)
    return Row(node, z, node.out_frame_bytes, (8, 16), lambda raw: sm.same_floats(raw.view(np.float32).reshape(want.shape), want))


OFDM = orf.Format(64, 16, orf.map_80211a(), 1, 0)   # one data symbol, no training


def within(want, per, bound):
    def same(raw):
        err = float(orf.symbol_errors(raw.view(np.complex64).reshape(FRAMES, -1), want, per).max())
        print("worst symbol off by %.3e (bound %.3e)" % (err, bound))
        return err <= bound
    return same


def ofdm_mod(c):
    args, kw = OFDM.node_args()
    z = orf.data_values(OFDM, FRAMES)
    node = c.OfdmModNode(*args, **kw)
    return Row(node, z, node.out_frame_bytes, (8, 8), within(orf.ref_mod(OFDM, z), OFDM.sym_len, orf.FFT_BOUND))


def ofdm_demod(c):
    args, kw = OFDM.node_args()
    rx = orf.samples(OFDM, FRAMES)
    node = c.OfdmDemodNode(*args, **kw)
    return Row(node, rx, node.out_frame_bytes, (8, 8), within(orf.ref_demod(OFDM, rx), OFDM.D, orf.FFT_BOUND))


ROWS = {"convenc": convenc, "viterbi": viterbi, "ldpcenc": ldpcenc, "ldpcdec": ldpcdec, "ratematch-tx": ratematch_tx, "ratematch-rx": ratematch_rx, "crc-attach": crc_attach,
        "crc-check": crc_check, "symmap": symmap, "demap-llr": lambda c: demap(c, "llr"), "demap-bits": lambda c: demap(c, "bits"),
        "ofdm-mod": ofdm_mod, "ofdm-demod": ofdm_demod}


@pytest.mark.parametrize("name", sorted(ROWS))
def test_frame_call_shell(c, name):
    row = ROWS[name](c)
    node, x = row.node, np.ascontiguousarray(row.x)
    assert x.shape[0] == FRAMES and x.nbytes % FRAMES == 0
    in_b, out_b = x.nbytes, FRAMES * row.out_bytes
    # one buffer holds both ranges, 64 bytes of slack in front, between and behind: every pointer below is inside it
    buf = c.DeviceBuf(64 + in_b + 64 + out_b + 64 + max(in_b, out_b))
    d_in, d_out = buf.ptr + 64, buf.ptr + 64 + (in_b + 64 + 15) // 16 * 16
    timer = c.KernelTimer(32).attach(node)
    launched = 0

    def refused(*args):
        with pytest.raises(c.CommsError) as e:
            node.run_dev(*args)
        assert e.value.code == c.COMMS_ERR_ARG, (name, args, str(e.value))
        assert timer.read_ms().size == launched, (name, args)          # nothing was launched

    def correct():
        nonlocal launched
        stage = np.full(d_out - buf.ptr + out_b, 0xFF, np.uint8)
        stage[64: 64 + in_b] = x.view(np.uint8).ravel()
        buf.upload(stage)
        node.run_dev(d_in, FRAMES, d_out)
        raw = buf.download(np.uint8, stage.size)
        launched += 1
        assert timer.read_ms().size == launched, name
        assert raw[: 64].tolist() == [0xFF] * 64 and raw[64: 64 + in_b].tobytes() == x.tobytes(), name     # the input is as it was
        assert row.same(raw[d_out - buf.ptr:]), name

    node.run_dev(None, 0, None)                                        # no frames: OK, nothing to do
    assert timer.read_ms().size == 0
    correct()
    a_in, a_out = row.aligns
    bad = [(None, FRAMES, d_out), (d_in + 1, FRAMES, d_out)]           # NULL with frames to do; the input one byte off
    if name != "crc-check":                                            # (the check's payload is an output a caller may leave out)
        bad.append((d_in, FRAMES, None))
    if a_out > 4:
        bad.append((d_in, FRAMES, d_out + 4))                          # 4 bytes off where 8 or 16 are required
    else:
        bad.append((d_in, FRAMES, d_out + 1))
    step = max(a_in, a_out)                                            # overlapping ranges at legal alignments:
    bad.append((d_in, FRAMES, d_in + (in_b - 1) // step * step))       # the output starts inside the input records ...
    bad.append((d_out + (out_b - 1) // step * step, FRAMES, d_out))    # ... and the input inside the output records
    for args in bad:
        refused(*args)
        correct()


# the element type of run()'s records where it is not uint8
OUT_DTYPES = {"ratematch-rx": np.float32, "demap-llr": np.float32, "symmap": np.complex64, "ofdm-mod": np.complex64, "ofdm-demod": np.complex64}


@pytest.mark.parametrize("name", sorted(ROWS))
def test_frame_run_shell(c, name):
    """The host form: run() on the row's records in their (FRAMES, record) shape and flat gives the reference; no frames give
    the empty 2-D array of the node's output type and an input one element short of whole records is a ValueError, neither
    with a launch."""
    row = ROWS[name](c)
    node, x = row.node, np.ascontiguousarray(row.x)
    assert node.in_frame_bytes * FRAMES == x.nbytes and node.out_frame_bytes == row.out_bytes
    timer = c.KernelTimer(8).attach(node)

    def primary(got):
        return got[0] if isinstance(got, tuple) else got

    dtype = np.dtype(OUT_DTYPES.get(name, np.uint8))
    out = primary(node.run(x))
    assert timer.read_ms().size == 1
    assert out.dtype == dtype and out.shape == (FRAMES, row.out_bytes // dtype.itemsize), (name, out.dtype, out.shape)
    assert row.same(np.ascontiguousarray(out).view(np.uint8).ravel()), name
    flat = primary(node.run(x.ravel()))
    assert timer.read_ms().size == 2
    assert flat.dtype == out.dtype and flat.tobytes() == out.tobytes(), name
    none = primary(node.run(x[:0]))
    assert none.shape == (0, row.out_bytes // dtype.itemsize) and none.dtype == dtype, (name, none.shape, none.dtype)
    with pytest.raises(ValueError):
        node.run(x.ravel()[:-1])
    assert timer.read_ms().size == 2, name                             # neither launched anything
