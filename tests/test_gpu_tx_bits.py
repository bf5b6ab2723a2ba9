"""GPU tests of the transmit front end: the PRNS source (bit-exact against tests/tx_ref.py), the digital.rs
modulators (bit-exact against their known answers), and the pulse shaper's packed-bit input (bit-identical to
the same node fed the mapped Complex<f32> symbols), end to end against the oracle chain.  Run with -m gpu."""
import json
import os
import subprocess

import numpy as np
import pytest

import oracle
import tx_ref as t

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

TOL = 1e-5
MAX32 = 0xD04FBB5A  # maximal 32-bit mask (tests/test_tx_ref.py::test_a_maximal_32_bit_mask)
MASKS = {8: 0xB8, 16: 0xB400, 32: MAX32, 64: 0xD800000000000000}
STATES = {8: 0x01, 16: 0xACE1, 32: 0x12345678, 64: 0x0123456789ABCDEF}

BPSK_EX = np.array([-1, 1], np.complex64)                              # 2b - 1 (single_thread_bpsk.rs:29-32)
QPSK_EX = np.array([-1 - 1j, 1 - 1j, -1 + 1j, 1 + 1j], np.complex64)   # (2x - 1, 2y - 1) (single_thread_qpsk.rs:29-35)
BPSK_DEF = np.array([1, -1], np.complex64)                             # digital.rs bpsk_bit_mod
QPSK_DEF = np.array([1 + 1j, -1 + 1j, 1 - 1j, -1 - 1j], np.complex64)  # digital.rs qpsk_bit_mod


@pytest.fixture(scope="module")
def c():
    import comms_rs_amd as c

    assert c.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested (no CPU fallback)"
    return c


@pytest.fixture(scope="module")
def dkats():
    with open(os.path.join(ROOT, "tests", "golden", "digital_kats.json")) as f:
        return json.load(f)


# ------------------------------------------------------------------ PRNS
@pytest.mark.parametrize("w", t.WIDTHS)
@pytest.mark.parametrize("packed", [False, True])
def test_prns_bit_exact(c, w, packed):
    for n in (1, 7, 8, 63, 64, 65, 4095, (1 << 20) + 3):
        node = c.PrnsNode(MASKS[w], STATES[w], w)
        got = node.run_batch(n, packed=packed)
        want = t.prns_packed(MASKS[w], STATES[w], n, w)
        assert np.array_equal(got, want if packed else t.unpack(want, n)), (w, n)
        assert node.state == t.Jump(MASKS[w], w).skip(STATES[w], n)


@pytest.mark.parametrize("w", t.WIDTHS)
def test_prns_2p28_bits(c, w):
    n = 1 << 28
    node = c.PrnsNode(MASKS[w], STATES[w], w)
    want = t.prns_packed(MASKS[w], STATES[w], n, w, streams=1 << 16)
    assert np.array_equal(node.run_batch(n, packed=True), want)
    if w == 64:
        node.state = STATES[w]
        assert np.array_equal(node.run_batch(n), t.unpack(want, n))


def test_prns_reference_node_semantics(c, kats):
    k = kats["prbs7"]
    node = c.PrnsNode(k["poly_mask"], k["state"])
    assert [node.run() for _ in range(len(k["expected"]))] == k["expected"]
    assert c.PrnsNode(0xC0, 0xFF).run() == 1  # prns.rs:59-62


@pytest.mark.parametrize("w", t.WIDTHS)
def test_prns_calls_concatenate_and_state_is_exact(c, w):
    j = t.Jump(MASKS[w], w)
    lens = [1, 5, 64, 3, 100, 127, 4096, 999, 65, 70000]
    total = sum(lens)
    want = t.unpack(t.prns_packed(MASKS[w], STATES[w], total, w), total)
    node = c.PrnsNode(MASKS[w], STATES[w], w)
    got, done = [], 0
    for i, n in enumerate(lens):  # the two output formats in turn
        got.append(t.unpack(node.run_batch(n, packed=True), n) if i & 1 else node.run_batch(n))
        done += n
        assert node.state == j.skip(STATES[w], done)
    assert np.array_equal(np.concatenate(got), want)
    # set_state then restore
    saved = node.state
    node.state = STATES[w]
    assert np.array_equal(node.run_batch(300), want[:300])
    node.state = saved
    tail = t.unpack(t.prns_packed(MASKS[w], saved, 50, w), 50)
    assert np.array_equal(node.run_batch(50), tail)
    # skip(n) then run == the tail of one run
    node = c.PrnsNode(MASKS[w], STATES[w], w)
    node.skip(12345)
    assert np.array_equal(node.run_batch(total - 12345), want[12345:])


def test_prns_skip_full_period_and_ranks(c):
    node = c.PrnsNode(MAX32, 0x1234567, 32)
    node.skip((1 << 32) - 1)
    assert node.state == 0x1234567
    # two "ranks": rank r starts at skip(r * n); their outputs concatenate to one node's
    n = 100003
    one = c.PrnsNode(0xC0, 0x01).run_batch(2 * n)
    r0 = c.PrnsNode(0xC0, 0x01).run_batch(n)
    r1 = c.PrnsNode(0xC0, 0x01).skip(n).run_batch(n)
    assert np.array_equal(np.concatenate([r0, r1]), one)


def test_prns_run_dev(c):
    n = (1 << 16) + 9
    want = t.prns_packed(0xB8, 0x01, n, 8)
    node = c.PrnsNode(0xB8, 0x01)
    buf = c.DeviceBuf(n)
    node.run_dev(n, buf.ptr, packed=True, stream=0)
    assert np.array_equal(buf.download(np.uint8, (n + 7) // 8), want)
    node.state = 0x01
    node.run_dev(n, buf.ptr, packed=False, stream=0)
    assert np.array_equal(buf.download(np.uint8, n), t.unpack(want, n))
    from comms_rs_amd._lib import lib

    assert lib().comms_prns_run_dev(node._h, 8, 7, buf.ptr, None) == c.COMMS_ERR_ARG  # unknown format
    assert lib().comms_prns_set_state(node._h, 0x100) == c.COMMS_ERR_ARG              # wider than W


# ------------------------------------------------------------------ modulators
def test_modulators_known_answers(c, dkats):
    for v, want in dkats["bpsk_bit"]["cases"]:
        assert c.bpsk_bit_mod([v]).tolist() == [want]
    for v, want in dkats["qpsk_bit"]["cases"]:
        assert c.qpsk_bit_mod([v]).tolist() == [want]
    for b, want in dkats["bpsk_byte"]["cases"]:
        assert c.bpsk_byte_mod([b]).tolist() == want
    for b, want in dkats["qpsk_byte"]["cases"]:
        assert c.qpsk_byte_mod([b]).tolist() == want


def test_modulators_random_bytes(c):
    x = np.random.default_rng(5).integers(0, 256, 1 << 20, dtype=np.uint8)
    assert np.array_equal(c.bpsk_byte_mod(x), t.bpsk_byte_mod(x))
    assert np.array_equal(c.qpsk_byte_mod(x), t.qpsk_byte_mod(x))
    assert np.array_equal(c.bpsk_bit_mod(x & 1), t.BPSK[x & 1])
    assert np.array_equal(c.qpsk_bit_mod(x & 3), t.QPSK[x & 3])


def test_bit_modulators_device_entries_write_zero_for_out_of_range(c):
    from comms_rs_amd._lib import lib

    x = np.array([0, 1, 2, 3, 4, 200], np.uint8)
    din, dout = c.DeviceBuf(64), c.DeviceBuf(64)
    din.upload(x)
    assert lib().comms_bpsk_bit_mod_dev(din.ptr, x.size, dout.ptr, 0, None) == 0
    got = dout.download(np.int16, 2 * x.size).reshape(-1, 2)
    assert got.tolist() == [[1, 0], [-1, 0], [0, 0], [0, 0], [0, 0], [0, 0]]
    assert lib().comms_qpsk_bit_mod_dev(din.ptr, x.size, dout.ptr, 0, None) == 0
    got = dout.download(np.int16, 2 * x.size).reshape(-1, 2)
    assert got.tolist() == [[1, 1], [-1, 1], [1, -1], [-1, -1], [0, 0], [0, 0]]
    with pytest.raises(c.CommsError):  # the host entry refuses it
        c.qpsk_bit_mod(x)


# ------------------------------------------------------------------ pulse shaper, packed-bit input
def _taps(rng, n, real):
    h = rng.standard_normal(n) + (0 if real else 1j * rng.standard_normal(n))
    return (h / n).astype(np.complex64)


CASES = [(sps, nt) for sps in (2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 32) for nt in (4 * sps - 1,)] + [(7, 29), (2, 301)]


@pytest.mark.parametrize("sps,n_taps", CASES)
@pytest.mark.parametrize("real", [True, False])
@pytest.mark.parametrize("mix", [False, True])
@pytest.mark.parametrize("i16", [False, True])
def test_pulse_bits_bit_identical_to_mapped_symbols(c, sps, n_taps, real, mix, i16):
    rng = np.random.default_rng(sps * 1000 + n_taps + 2 * real + 4 * mix + 8 * i16)
    taps = _taps(rng, n_taps, real)
    k = 1 + int(real)  # every (sps, k, table) combination: k from `real`, the examples' tables with i16 output
    cons = (BPSK_EX if k == 1 else QPSK_EX) if i16 else None
    table = cons if cons is not None else (BPSK_DEF if k == 1 else QPSK_DEF)
    a, b = c.PulseNode(taps, sps), c.PulseNode(taps, sps)
    for node in (a, b):
        if mix:
            node.set_mixer(2 * np.pi * 0.0123, 0.3)
        if i16:
            node.set_output_format("i16", 8192.0)
    a.set_input_format("bits", k, cons)
    # several calls, n_sym not a multiple of 8 / k, a switch to c32 symbols and back in between
    for n_sym in (1001, 37, 5, 2048):
        packed = rng.integers(0, 256, (n_sym * k + 7) // 8, dtype=np.uint8)
        sym = t.map_bits(packed, n_sym, k, table)
        got, want = a.run_bits(packed, n_sym), b.run(sym)
        assert np.array_equal(got.view(np.int32) if i16 else got.view(np.uint64),
                              want.view(np.int32) if i16 else want.view(np.uint64)), n_sym
        if n_sym == 37:
            a.set_input_format("c32")
            s2 = (rng.standard_normal(77) + 1j * rng.standard_normal(77)).astype(np.complex64)
            assert np.array_equal(a.run(s2).view(np.int32 if i16 else np.uint64), b.run(s2).view(np.int32 if i16 else np.uint64))
            a.set_input_format("bits", k, cons)


def test_pulse_bits_device_entry_and_refusals(c):
    from comms_rs_amd._lib import lib

    taps = c.rrc_taps(63, 4.0, 0.25)
    a, b = c.PulseNode(taps, 4).set_input_format("bits", 2), c.PulseNode(taps, 4)
    n_sym = 4099
    packed = np.random.default_rng(1).integers(0, 256, (2 * n_sym + 7) // 8, dtype=np.uint8)
    din, dout = c.DeviceBuf(packed.size), c.DeviceBuf(n_sym * 4 * 8)
    din.upload(packed)
    a.run_dev(din.ptr, n_sym, dout.ptr, stream=0)
    got = dout.download(np.complex64, n_sym * 4)
    assert np.array_equal(got.view(np.uint64), b.run(t.map_bits(packed, n_sym, 2, QPSK_DEF)).view(np.uint64))
    for fmt, k in ((1, 3), (1, 0), (1, 8), (2, 1), (-1, 1)):
        assert lib().comms_pulse_set_input_format(a._h, fmt, k, None) == c.COMMS_ERR_ARG, (fmt, k)


def test_pulse_bits_host_entry_across_chunks(c):
    # a call long enough for the host entry's large-transfer route.  (Its chunked pipeline needs both directions to carry
    # a real share of the bytes; a packed-bit call's output is >= 64 times its input, so it runs in one piece, while
    # the c32 node it is compared with is pipelined.)
    taps = c.rrc_taps(63, 4.0, 0.25)
    for k in (1, 2):
        a, b = c.PulseNode(taps, 4).set_input_format("bits", k), c.PulseNode(taps, 4)
        a.set_output_format("i16", 8192.0)
        b.set_output_format("i16", 8192.0)
        n_sym = (1 << 22) + 13
        packed = np.random.default_rng(k).integers(0, 256, (n_sym * k + 7) // 8, dtype=np.uint8)
        got = a.run_bits(packed, n_sym)
        want = b.run(t.map_bits(packed, n_sym, k, BPSK_DEF if k == 1 else QPSK_DEF))
        assert np.array_equal(got, want)


# ------------------------------------------------------------------ end to end
def _fir_close(got, want, taps, x):
    d = np.abs(got.astype(np.complex128) - want.astype(np.complex128))
    bound = TOL * np.sum(np.abs(taps)) * max(np.max(np.abs(x)), 1e-30)
    assert d.max(initial=0.0) <= bound, (d.max(), bound)
    nrm = np.linalg.norm(want.astype(np.complex128))
    if nrm > 0:
        assert np.linalg.norm(d) / nrm <= TOL


def test_config1_chain_from_prns_bits(c):
    """BASELINE config 1 (PRBS -> BPSK 2b-1 -> 63-tap RRC x4 -> mixer) at full size, with the source on the device and
    the symbols read as packed bits: against the oracle chain of test_gpu_parity.py's config 1 test."""
    n_sym = 262144
    bits, _ = oracle.prns_u8(0xC0, 0x01, n_sym)
    sym = (bits.astype(np.float32) * 2.0 - 1.0).astype(np.complex64)
    taps = oracle.rrc_taps(63, 4.0, 0.25)
    dphase = 2 * np.pi * 0.1
    want = oracle.Mixer(0.0, dphase).mix(oracle.pulse(sym, taps, 4, oracle.default_state(taps)))
    packed = c.PrnsNode(0xC0, 0x01).run_batch(n_sym, packed=True)
    assert np.array_equal(t.unpack(packed, n_sym), bits)
    node = c.PulseNode(c.rrc_taps(63, 4.0, 0.25), 4).set_mixer(dphase).set_input_format("bits", 1, BPSK_EX)
    got = node.run_bits(packed, n_sym)
    assert got.size == 1 << 20
    _fir_close(got, want, taps, sym)


def test_qpsk_example_chain_i16(c):
    """examples/single_thread_qpsk.rs: bits -> (2x-1, 2y-1) -> 32-tap RRC x4 -> (8192 y) as i16."""
    n_sym = 1 << 16
    packed = c.PrnsNode(MAX32, 0xCAFE, 32).run_batch(2 * n_sym, packed=True)
    sym = t.map_bits(packed, n_sym, 2, QPSK_EX)
    taps = oracle.rrc_taps(32, 4.0, 0.25)
    want = oracle.iq_c32_to_i16(oracle.pulse(sym, taps, 4, oracle.default_state(taps)), 8192.0)
    node = c.PulseNode(c.rrc_taps(32, 4.0, 0.25), 4).set_input_format("bits", 2, QPSK_EX).set_output_format("i16", 8192.0)
    got = node.run_bits(packed, n_sym)
    want = np.asarray(want, np.int32).reshape(got.shape)
    bound = 1 + 8192.0 * TOL * np.sum(np.abs(taps)) * np.sqrt(2)
    assert np.max(np.abs(got.astype(np.int32) - want)) <= bound


# ------------------------------------------------------------------ C++ node in a graph
def test_cpp_prns_node_in_a_graph():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "comms_rs_amd", "host"), "-s"], timeout=600)
    out = subprocess.run([os.path.join(ROOT, "comms_rs_amd", "lib", "test_tx_nodes_gpu")], capture_output=True,
                         text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all passed" in out.stdout
