"""GPU tests of the receive end's hard decisions: comms_sym_to_bits bit-exact against tests/rx_ref.py; the chain's bits
output (comms_chain_set_output_format) bit for bit equal to rx_ref applied to the same chain's Complex<f32> output, for every
chain kind; a PRNS -> pulse shaper -> i16 -> chain -> bits loopback with zero bit errors, proven by an ISI bound; and
comms_bit_errors against numpy.  Run with -m gpu."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rx_ref as r
import tx_ref as t

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

CANARY = 0xA5
QPSK_CUSTOM = np.array([0.3 + 0.1j, -0.2 + 0.25j, 0.15 - 0.3j, -0.05 - 0.02j], np.complex64)
BPSK_CUSTOM = np.array([0.1 - 0.2j, -0.05 + 0.4j], np.complex64)


@pytest.fixture(scope="module")
def c():
    import comms_rs_amd as c

    assert c.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested (no CPU fallback)"
    return c


def _tables(k):
    return [None, r.BPSK_EX if k == 1 else r.QPSK_EX, BPSK_CUSTOM if k == 1 else QPSK_CUSTOM]


def _ref_bits(y, k, table):
    return r.sym_to_bits(y, k, table)


def _edge_symbols(n, seed):
    """Symbols with ties, signed zeros, subnormals, NaN / Inf and points on the decision lines, the rest random."""
    rng = np.random.default_rng(seed)
    y = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    f = np.float32
    special = np.array([0, -0.0, 1e-45, -1e-45, -1e-40, np.nan, np.inf, -np.inf, 0.5, -0.5, 1.0, -1.0, 3e38, -3e38,
                        0.1, 0.125, -0.05, 2.0 ** -26], f)
    m = rng.random(n) < 0.5
    re = np.where(m, special[rng.integers(0, special.size, n)], y.real).astype(f)
    im = np.where(rng.random(n) < 0.5, special[rng.integers(0, special.size, n)], y.imag).astype(f)
    out = np.empty(n, np.complex64)
    out.real, out.imag = re, im
    return out


# ------------------------------------------------------------------ sym_to_bits
@pytest.mark.parametrize("k", [1, 2])
def test_sym_to_bits_host_bit_exact(c, k):
    for n in (1, 7, 8, 9, 63, 64, 65, 1000, 65537):
        y = _edge_symbols(n, n * k)
        for table in _tables(k):
            got = c.sym_to_bits(y, k, table)
            assert np.array_equal(got, _ref_bits(y, k, table)), (n, table)


@pytest.mark.parametrize("k", [1, 2])
def test_sym_to_bits_long_and_device_entry(c, k):
    import torch

    n = (1 << 24) + 3
    y = _edge_symbols(n, 7 + k)
    want = _ref_bits(y, k, None)
    assert np.array_equal(c.sym_to_bits(y, k), want)
    yd = torch.from_numpy(y.view(np.float32)).to("cuda:0")
    for n_sym in (1, 7, 8, 9, 63, 64, 65, n):
        nb = (n_sym * k + 7) // 8
        out = torch.full((nb + 64,), CANARY, dtype=torch.uint8, device="cuda:0")
        c.sym_to_bits_dev(yd.data_ptr(), n_sym, k, out.data_ptr())
        got = out.cpu().numpy()
        assert np.array_equal(got[:nb], _ref_bits(y[:n_sym], k, None)), n_sym
        assert np.all(got[nb:] == CANARY), n_sym
    # unaligned (8-byte, not 16-byte) symbols take the narrow loads
    out = torch.full((1024,), CANARY, dtype=torch.uint8, device="cuda:0")
    c.sym_to_bits_dev(yd.data_ptr() + 8, 1001, k, out.data_ptr())
    nb = (1001 * k + 7) // 8
    got = out.cpu().numpy()
    assert np.array_equal(got[:nb], _ref_bits(y[1:1002], k, None)) and np.all(got[nb:] == CANARY)


def test_sym_to_bits_refusals(c):
    from comms_rs_amd._lib import lib

    y = np.zeros(64, np.complex64)
    out = np.zeros(64, np.uint8)
    for k in (0, 3, -1, 8):
        assert lib().comms_sym_to_bits(y.ctypes.data, 64, k, None, out.ctypes.data, 0) == c.COMMS_ERR_ARG, k
    import torch

    yd = torch.zeros(128, dtype=torch.complex64, device="cuda:0")
    od = torch.zeros(128, dtype=torch.uint8, device="cuda:0")
    assert lib().comms_sym_to_bits_dev(yd.data_ptr(), 64, 1, None, od.data_ptr() + 1, 0, None) == c.COMMS_ERR_ARG
    assert lib().comms_sym_to_bits_dev(yd.data_ptr() + 4, 64, 1, None, od.data_ptr(), 0, None) == c.COMMS_ERR_ARG


# ------------------------------------------------------------------ chain bits == rx_ref(chain c32)
def _x(c, n, fmt, seed):
    x = c.synth_iq(n, seed * 7919)
    if fmt == "c32":
        return x
    if fmt == "i16":
        return c.iq_c32_to_i16(x, 8192.0)
    return np.clip(np.round(x.view(np.float32) * 127.5 + 127.5), 0, 255).astype(np.uint8).reshape(-1, 2)


def _pair(c, make, fmt, k, table):
    a, b = make(), make()
    scale = 1.0 / 8192 if fmt == "i16" else 1.0
    a.set_input_format(fmt, scale)
    b.set_input_format(fmt, scale)
    b.set_output_format("bits", k, table)
    return a, b


def _check_calls(c, a, b, lens, fmt, k, table, seed, kernel=None):
    """Per call: b's bits == rx_ref(a's c32), a and b fed the same stream."""
    pos = 0
    for i, n in enumerate(lens):
        x = _x(c, n, fmt, seed + i)
        y = a.run(x)
        got = b.run(x)
        assert got.dtype == np.uint8 and got.size == (y.size * k + 7) // 8
        assert np.array_equal(got, _ref_bits(y, k, table)), (i, n, pos)
        if kernel is not None:
            assert b.kernel == kernel, (b.kernel, kernel)
        pos += n


# (taps, rate, ChainNode kwargs, the kernel reported after the run)
KINDS = [
    ("rrc63", 4, dict(), "time"),                      # Decim (config 1's receive filter)
    ("rrc63", 4, dict(kernel="freq"), "freq"),         # Os1024
    ("rrc63", 4, dict(kernel="poly"), "poly"),         # Poly8
    ("rrc63", 17, dict(), "time_any"),                 # DecimAny (rate 17)
    ("129", 8, dict(), "poly"),                        # Decim handed to fir_poly8_kernel
    ("300", 5, dict(), "freq"),                        # Os4096Dec (300 taps)
    ("2000", 5, dict(), "freq"),                       # Os16kDec
    ("rrc63", 4, dict(unfused=True), "unfused"),       # Series (mixer in front) / SeriesPost (mixer after)
]


def _taps(c, name):
    if name == "rrc63":
        return c.rrc_taps(63, 4.0, 0.25)
    n = int(name)
    return c.rrc_taps(n, 8.0, 0.35)


@pytest.mark.parametrize("kind", range(len(KINDS)))
@pytest.mark.parametrize("after", [False, True])
@pytest.mark.parametrize("k", [1, 2])
def test_chain_bits_every_kind(c, kind, after, k):
    name, rate, kw, kernel = KINDS[kind]
    taps = _taps(c, name)
    dphase = 2 * np.pi * 0.0371
    for fmt, table in (("c32", None), ("i16", _tables(k)[1])):
        a, b = _pair(c, lambda: c.ChainNode(dphase, 0.3, taps, rate, False, mixer_after_fir=after, **kw), fmt, k, table)
        lens = [rate * (8 * 517 + 3), rate * 5, rate * (8 * 4096 + 1)]  # multiples of R, not of 8R
        if name == "129":
            lens = [rate * (1 << 17) + rate * 3, rate * ((1 << 17) + 5)]  # long enough for the polyphase hand-over
        _check_calls(c, a, b, lens, fmt, k, table, seed=kind, kernel=kernel)


@pytest.mark.parametrize("rate", [2, 3, 4, 5, 6, 8, 10, 12, 16])
@pytest.mark.parametrize("after", [False, True])
def test_chain_bits_decim_rates(c, rate, after):
    taps = c.rrc_taps(8 * rate + 1 if rate <= 4 else 2 * rate + 1, float(rate), 0.3)
    dphase = 2 * np.pi * 0.013
    for fmt, k in (("c32", 1), ("i16", 2), ("u8", 1)):
        a, b = _pair(c, lambda: c.ChainNode(dphase, 1.1, taps, rate, False, mixer_after_fir=after, kernel="time"), fmt, k, None)
        _check_calls(c, a, b, [rate * 1003, rate * 9, rate * (3 * 4096 + 7)], fmt, k, None, seed=rate, kernel="time")


def test_chain_switch_formats_mid_stream(c):
    taps = c.rrc_taps(63, 4.0, 0.25)
    dphase = 2 * np.pi * 0.021
    for kw in (dict(), dict(kernel="freq"), dict(unfused=True)):
        a = c.ChainNode(dphase, 0.0, taps, 4, False, **kw)
        b = c.ChainNode(dphase, 0.0, taps, 4, False, **kw)
        for i, (n, fmt) in enumerate([(4 * 1001, "bits"), (4 * 333, "c32"), (4 * 8195, "bits"), (4 * 77, "bits"), (4 * 99, "c32")]):
            x = c.synth_iq(n, 1000 * i)
            y = a.run(x)
            if fmt == "bits":
                b.set_output_format("bits", 2)
                assert np.array_equal(b.run(x), _ref_bits(y, 2, None)), (kw, i)
            else:
                b.set_output_format("c32")
                assert np.array_equal(b.run(x).view(np.uint64), y.view(np.uint64)), (kw, i)


def test_chain_checkpoint_across_bits_call(c):
    taps = c.rrc_taps(63, 4.0, 0.25)
    n_taps = taps.size
    dphase = 2 * np.pi * 0.047
    for kw in (dict(), dict(kernel="freq"), dict(unfused=True), dict(mixer_after_fir=True)):
        a = c.ChainNode(dphase, 0.2, taps, 4, False, **kw)
        b = c.ChainNode(dphase, 0.2, taps, 4, False, **kw).set_output_format("bits", 1)
        x1, x2 = c.synth_iq(4 * 5003, 1), c.synth_iq(4 * 2001, 2)
        a.run(x1)
        b.run(x1)
        state, phase = b.fir_state(n_taps), b.phase
        fresh = c.ChainNode(dphase, 0.0, taps, 4, False, **kw).set_output_format("bits", 1)
        fresh.phase = phase
        fresh.set_fir_state(state)
        y2 = a.run(x2)
        assert np.array_equal(fresh.run(x2), _ref_bits(y2, 1, None)), kw
        assert np.array_equal(b.run(x2), _ref_bits(y2, 1, None)), kw


def test_chain_host_entry_equals_device_entry(c):
    import torch

    taps = c.rrc_taps(63, 4.0, 0.25)
    dphase = 2 * np.pi * 0.09
    # short (pinned staging), past the zero-copy limit, and long (device scratch)
    for n in (4 * 9, 4 * 3001, 4 * ((1 << 20) + 5), 4 * ((1 << 22) + 3)):
        for k in (1, 2):
            h = c.ChainNode(dphase, 0.0, taps, 4, False).set_output_format("bits", k)
            d = c.ChainNode(dphase, 0.0, taps, 4, False).set_output_format("bits", k)
            h.set_input_format("i16", 1.0 / 8192)
            d.set_input_format("i16", 1.0 / 8192)
            x = _x(c, n, "i16", n)
            got = h.run(x)
            nb = d.out_bytes(n)
            xd = torch.from_numpy(x).to("cuda:0")
            out = torch.full((nb + 64,), CANARY, dtype=torch.uint8, device="cuda:0")
            d.run_dev(xd.data_ptr(), n, out.data_ptr(), stream=0)
            o = out.cpu().numpy()
            assert np.array_equal(o[:nb], got), (n, k)
            assert np.all(o[nb:] == CANARY), (n, k)


def test_chain_bits_canary_every_kind(c):
    import torch

    for name, rate, kw, _ in KINDS:
        taps = _taps(c, name)
        node = c.ChainNode(0.1, 0.0, taps, rate, False, **kw).set_output_format("bits", 1)
        n = rate * (8 * 1000 + 5)
        xd = torch.from_numpy(c.synth_iq(n, 3).view(np.float32)).to("cuda:0")
        nb = node.out_bytes(n)
        out = torch.full((nb + 64,), CANARY, dtype=torch.uint8, device="cuda:0")
        node.run_dev(xd.data_ptr(), n, out.data_ptr(), stream=0)
        o = out.cpu().numpy()
        assert o[nb - 1] >> 5 == 0, (name, kw)  # 8000 + 5 bits: the last byte's top three bits are zero
        assert np.all(o[nb:] == CANARY), (name, kw)


def test_chain_bits_refusals(c):
    import torch
    from comms_rs_amd._lib import lib

    taps = c.rrc_taps(63, 4.0, 0.25)
    fm = c.ChainNode(0.1, 0.0, taps, 4, True)
    with pytest.raises(c.CommsError):
        fm.set_output_format("bits", 1)
    node = c.ChainNode(0.1, 0.0, taps, 4, False)
    for k in (0, 3):
        assert lib().comms_chain_set_output_format(node._h, 1, k, None) == c.COMMS_ERR_ARG
    assert lib().comms_chain_set_output_format(node._h, 7, 1, None) == c.COMMS_ERR_ARG
    node.set_output_format("bits", 1)
    xd = torch.zeros(4096, dtype=torch.complex64, device="cuda:0")
    od = torch.zeros(256, dtype=torch.uint8, device="cuda:0")
    for off in (1, 2, 3):
        assert lib().comms_chain_run_dev(node._h, C.c_void_p(xd.data_ptr()), 4096, C.c_void_p(od.data_ptr() + off), None) == c.COMMS_ERR_ARG
    assert lib().comms_chain_run_dev(node._h, C.c_void_p(xd.data_ptr()), 4096, C.c_void_p(od.data_ptr() + 4), None) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ loopback
MASK32, STATE32 = 0xD04FBB5A, 0x2468ACE1


def _isi_margin(h, sps, peak, scale):
    """Worst-case per-axis margin of the sampled combined response (tx RRC * rx RRC) for unit-amplitude axes: |peak| minus
    the off-peak sum and the i16 quantisation error (|e| < 1/scale per component, through the receive filter and the
    unmixing rotation)."""
    g = np.convolve(h.astype(np.float64), h.astype(np.float64))
    idx = peak + sps * np.arange(-(peak // sps), (g.size - 1 - peak) // sps + 1)
    off = np.sum(np.abs(g[idx[idx != peak]]))
    quant = np.sqrt(2.0) * np.sum(np.abs(h)) / scale
    return abs(g[peak]) - off - quant - 1e-3 * abs(g[peak])


def _loopback(c, k, sps, taps, n_sym, shift=0):
    h = np.real(taps).astype(np.float64)
    n = taps.size
    assert np.all(np.imag(taps) == 0)
    dphase = 2 * np.pi * 0.0173
    amp = np.sqrt(2.0) if k == 2 else 1.0
    scale = float(np.floor(32767.0 / (np.sum(np.abs(h)) * amp * 1.01)))
    assert np.sum(np.abs(h)) * amp * scale < 32767  # no saturation of the i16 wire format
    peak = n - 1 + shift  # the combined response's peak, in receiver samples
    assert peak % sps == 0
    delay = peak // sps
    assert _isi_margin(h, sps, peak - shift, scale) > 0  # every decision is right whatever the bits: zero errors is a theorem
    bits = c.PrnsNode(MASK32, STATE32, 32).run_batch(n_sym * k, packed=True)
    tx = c.PulseNode(taps, sps).set_input_format("bits", k).set_mixer(dphase).set_output_format("i16", scale)
    # the receiver unmixes with the transmitter's phase of the sample it sees: shifted by `shift` samples
    rx = c.ChainNode(-dphase, dphase * shift, taps, sps, False)
    rx.set_input_format("i16", 1.0 / scale).set_output_format("bits", k)
    # several calls on both sides, cut differently
    tx_calls = [n_sym // 4 - 24, n_sym // 4 + 24, n_sym // 2]
    rx_out, pending, pos = [], np.zeros((shift, 2), np.int16), 0
    rx_chunk = 32 * sps * 3001
    for m in tx_calls:
        assert (pos * k) % 8 == 0
        samples = tx.run_bits(bits[pos * k // 8:(pos + m) * k // 8 + 1], m)
        pos += m
        pending = np.concatenate([pending, samples])
        while pending.shape[0] >= rx_chunk:
            rx_out.append(rx.run(pending[:rx_chunk]))
            pending = pending[rx_chunk:]
    tail = pending.shape[0] // (32 * sps) * (32 * sps)
    if tail:
        rx_out.append(rx.run(pending[:tail]))
    got = np.concatenate(rx_out)
    n_rx = got.size * 8 // k
    n_cmp = n_rx - delay
    assert n_cmp > n_sym // 2
    assert (delay * k) % 8 == 0
    want = bits
    errors = c.bit_errors(got[delay * k // 8:], want, n_cmp * k)
    assert errors == 0, errors
    assert np.array_equal(t.unpack(got[delay * k // 8:], n_cmp * k), t.unpack(want, n_cmp * k))
    return rx.kernel


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("sps", [4, 8])
def test_loopback_zero_errors(c, k, sps):
    taps = c.rrc_taps(8 * sps + 1, float(sps), 0.35)
    _loopback(c, k, sps, taps, 1 << 24)


@pytest.mark.parametrize("k", [1, 2])
def test_loopback_examples_rrc32(c, k):
    # rrc_taps(32, 4, 0.25): even length, the combined response peaks at 31, between two symbol instants.  The receiver
    # sees the transmitted stream one sample late (one zero sample in front), so that the peak falls on sample 32 = 8 symbols.
    _loopback(c, k, 4, c.rrc_taps(32, 4.0, 0.25), 1 << 20, shift=1)


# ------------------------------------------------------------------ bit errors
def test_bit_errors_against_numpy(c):
    rng = np.random.default_rng(5)
    raw_a = rng.integers(0, 256, 70000, dtype=np.uint8)
    raw_b = rng.integers(0, 256, 70000, dtype=np.uint8)
    for n_bits in (1, 7, 9, 127, 129, 1001, 8 * 65537 + 5, 8 * 69990 + 3):
        for off in (0, 1, 3):  # unaligned host buffers
            a, b = raw_a[off:], raw_b[3 - off:]
            assert c.bit_errors(a, b, n_bits) == r.bit_errors(a, b, n_bits), (n_bits, off)
    # bits beyond n_bits in the last byte are ignored
    assert c.bit_errors(np.array([0xF0], np.uint8), np.array([0x0F], np.uint8), 4) == 4


def test_bit_errors_injected_and_2p30(c):
    import torch

    n_bits = 1 << 30
    rng = np.random.default_rng(9)
    a = rng.integers(0, 256, n_bits // 8, dtype=np.uint8)
    b = a.copy()
    flips = np.unique(rng.integers(0, n_bits, 4097))
    np.bitwise_xor.at(b, flips // 8, (1 << (flips % 8)).astype(np.uint8))
    assert c.bit_errors(a, b, n_bits) == flips.size
    assert c.bit_errors(a, a, n_bits) == 0
    da, db = torch.from_numpy(a).to("cuda:0"), torch.from_numpy(b).to("cuda:0")
    assert c.bit_errors_dev(da.data_ptr(), db.data_ptr(), n_bits) == flips.size
    # a count past the first flips only
    m = int(flips[100])
    assert c.bit_errors_dev(da.data_ptr(), db.data_ptr(), m) == 100
    assert c.bit_errors_dev(da.data_ptr() + 1, db.data_ptr() + 1, n_bits - 8) == int(np.count_nonzero(flips >= 8))


# ------------------------------------------------------------------ C++ graph
def test_cpp_rx_loopback_graph():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "comms_rs_amd", "host"), "-s"], timeout=600)
    out = subprocess.run([os.path.join(ROOT, "comms_rs_amd", "lib", "test_rx_nodes_gpu")], capture_output=True,
                         text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all passed" in out.stdout
