"""GPU tests of the seeded noise source and the AWGN node (comms_noise_*, comms_awgn_*) against tests/noise_ref.py:
bits bit-exact, uniform within one ulp, normals and AWGN within the accuracy the header states, the cut / shard / skip
rules bit for bit, the refusals, and a whole BPSK / QPSK link on the device whose error count is compared with the
reference link's.  Run with -m gpu."""
import ctypes as C
import math

import numpy as np
import pytest

import noise_ref as nr

pytestmark = pytest.mark.gpu

CANARY = 0xA5
SEED, STREAM = 0x1234567887654321, 0x00000003FFFFFFFF  # both halves of key and counter in use
ACC = 2.0 ** -17  # |z - z_ref| <= ACC * max(1, |z_ref|)
TOL = 1e-5        # the chain's parity tolerance (tests/test_gpu_parity.py)


@pytest.fixture(scope="module")
def c():
    import comms_rs_amd as c

    assert c.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested (no CPU fallback)"
    return c


def _lib():
    from comms_rs_amd._lib import lib

    return lib()


class _Guarded:
    """A device buffer of `nbytes` with canary bytes behind it."""

    def __init__(self, c, nbytes, pad=64):
        self.nbytes, self.pad = nbytes, pad
        self.buf = c.DeviceBuf(nbytes + pad)
        self.buf.upload(np.full(nbytes + pad, CANARY, np.uint8))
        self.ptr = self.buf.ptr

    def read(self, dtype, count):
        raw = self.buf.download(np.uint8, self.nbytes + self.pad)
        assert np.all(raw[self.nbytes:] == CANARY), "bytes behind the output were written"
        return raw[:count * np.dtype(dtype).itemsize].view(dtype).copy()


# ------------------------------------------------------------------ bits
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("entry", ["host", "dev"])
def test_bits_bit_exact(c, packed, entry):
    for n in (1, 31, 32, 33, 1000, (1 << 24) + 3):
        for pos in (0, 5):
            src = c.NoiseSource(SEED, STREAM)
            src.pos = pos
            want = nr.Source(SEED, STREAM, pos).bits(n, packed=packed)
            if entry == "host":
                got = src.bits(n, packed=packed)
            else:
                g = _Guarded(c, want.size)
                src.bits_dev(n, g.ptr, packed=packed)
                got = g.read(np.uint8, want.size)
            assert np.array_equal(got, want), (n, pos)
            assert src.pos == pos + (n + 31) // 32


# ------------------------------------------------------------------ uniform
def _ulp(x):
    x = np.abs(np.asarray(x, np.float32))
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


@pytest.mark.parametrize("entry", ["host", "dev"])
def test_uniform_within_one_ulp_and_in_range(c, entry):
    f32 = np.float32
    one_up = float(np.nextafter(f32(1.0), f32(2.0)))
    for lo, hi in ((0.0, 1.0), (-3.5, 2.25), (1.0, one_up), (-3e38, 3e38), (100.0, 100.5)):
        for n, pos in ((1, 0), (5, 3), (1001, 2), ((1 << 22) + 1, 0)):
            src = c.NoiseSource(SEED, STREAM)
            src.pos = pos
            exact, _ = nr.Source(SEED, STREAM, pos).uniform(n, lo, hi)
            if entry == "host":
                got = src.uniform(n, lo, hi)
            else:
                g = _Guarded(c, 4 * n)
                src.uniform_dev(n, g.ptr, lo, hi)
                got = g.read(np.float32, n)
            assert src.pos == pos + n
            assert np.all(got >= f32(lo)) and np.all(got < f32(hi)), (lo, hi, n)
            err = np.abs(got.astype(np.float64) - exact)
            assert np.all(err <= _ulp(got)), (lo, hi, n, float(np.max(err / _ulp(got))))


# ------------------------------------------------------------------ normals
@pytest.mark.parametrize("f64", [False, True])
def test_normals_accuracy_2p24(c, f64):
    n = 1 << 24
    dt = np.float64 if f64 else np.float32
    z_ref = nr.Source(12345, 7).normal(n)
    scale_ref = np.maximum(1.0, np.abs(z_ref))
    got = c.NoiseSource(12345, 7).normal(n, dtype=dt)
    assert got.dtype == dt
    err = np.abs(got.astype(np.float64) - z_ref) / scale_ref
    print("normal %s: max |z - z_ref| / max(1, |z_ref|) = %.3e (bound %.3e), max |z| = %.4f"
          % (dt.__name__, err.max(), ACC, np.abs(got).max()))
    assert err.max() <= ACC
    assert np.abs(got).max() <= math.sqrt(48.0 * math.log(2.0)) * (1 + ACC)
    # scaled: the bound times sd
    sd = 2.5
    got = c.NoiseSource(12345, 7).normal(1 << 20, 0.0, sd, dtype=dt)
    assert np.max(np.abs(got.astype(np.float64) - sd * z_ref[:1 << 20]) / scale_ref[:1 << 20]) <= sd * ACC
    # with a mean: the f32 output is rounded once more (half an ulp of the value, 2^-24 relative); the f64 output is not
    mu, sd = -1.25, 0.75
    got = c.NoiseSource(12345, 7).normal(1 << 20, mu, sd, dtype=dt).astype(np.float64)
    want = mu + sd * z_ref[:1 << 20]
    rounding = 0.0 if f64 else 2.0 ** -24 * np.abs(want)
    assert np.all(np.abs(got - want) <= sd * ACC * scale_ref[:1 << 20] + rounding)
    # the f64 form is the f32 z widened
    if f64:
        z32 = c.NoiseSource(12345, 7).normal(4096)
        assert np.array_equal(c.NoiseSource(12345, 7).normal(4096, dtype=np.float64), z32.astype(np.float64))


def test_normals_device_entries(c):
    for f64 in (False, True):
        dt = np.float64 if f64 else np.float32
        for n, pos in ((1, 0), (2, 1), (7, 3), (1001, 6)):
            src = c.NoiseSource(SEED, STREAM)
            src.pos = pos
            g = _Guarded(c, n * np.dtype(dt).itemsize)
            src.normal_dev(n, g.ptr, 0.0, 1.0, f64=f64)
            got = g.read(dt, n)
            z_ref = nr.Source(SEED, STREAM, pos).normal(n)
            assert np.all(np.abs(got - z_ref) <= ACC * np.maximum(1.0, np.abs(z_ref))), (f64, n, pos)
            assert src.pos == pos + n


# ------------------------------------------------------------------ AWGN
def _awgn_check(got, x_in, sigma, g_ref):
    want = x_in.astype(np.complex128) + sigma * g_ref
    for part in ("real", "imag"):
        w, z = getattr(want, part), getattr(g_ref, part)
        bound = sigma * ACC * np.maximum(1.0, np.abs(z)) + 2.0 ** -23 * np.abs(w)
        err = np.abs(getattr(got, part).astype(np.float64) - w)
        assert np.all(err <= bound), (part, float(np.max(err - bound)))


def _signal(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


@pytest.mark.parametrize("fmt", ["c32", "i16"])
@pytest.mark.parametrize("in_place", [False, True])
def test_awgn_against_the_reference(c, fmt, in_place):
    scale = 1.0 / 2746.0
    for n in (1, 2, 3, 1001, (1 << 22) + 1):
        for pos in (0, 3):
            g_ref = nr.Source(SEED, STREAM, pos).complex_normal(n)
            for sigma in (0.7, 0.0):
                if fmt == "i16":
                    raw = np.random.default_rng(n).integers(-32768, 32768, (n, 2), dtype=np.int16)
                    x32 = raw.astype(np.float32) * np.float32(scale)
                    x_in = (x32[:, 0] + 1j * x32[:, 1]).astype(np.complex64)
                else:
                    raw = x_in = _signal(n, n)
                src = c.NoiseSource(SEED, STREAM)
                src.pos = pos
                src.set_input_format(fmt, scale)
                if in_place and fmt == "c32":
                    g = _Guarded(c, 8 * n)
                    g.buf.upload(raw)
                    src.awgn_dev(g.ptr, n, sigma, g.ptr)
                    got = g.read(np.complex64, n)
                elif in_place:
                    # the i16 node has no in-place form (4 bytes in, 8 out): the call is refused and nothing moves
                    d = c.DeviceBuf(8 * n)
                    assert _lib().comms_awgn_run_dev(src._h, d.ptr, n, sigma, d.ptr, None) == c.COMMS_ERR_ARG
                    assert src.pos == pos
                    continue
                elif n == 1001:
                    din, g = c.DeviceBuf(raw.nbytes), _Guarded(c, 8 * n)
                    din.upload(raw)
                    src.awgn_dev(din.ptr, n, sigma, g.ptr)
                    got = g.read(np.complex64, n)
                else:
                    got = src.awgn(raw, sigma)
                assert src.pos == ((pos + 1) & ~1) + 2 * n
                if sigma == 0.0:
                    assert np.array_equal(got.view(np.uint64), x_in.view(np.uint64)), (n, pos)
                else:
                    _awgn_check(got, x_in, sigma, g_ref)


def test_awgn_i16_is_the_conversion_followed_by_the_node(c):
    n, scale = 70001, 1.0 / 1942.0
    raw = np.random.default_rng(2).integers(-32768, 32768, (n, 2), dtype=np.int16)
    a = c.NoiseSource(SEED, 1).set_input_format("i16", scale).awgn(raw, 0.3)
    b = c.NoiseSource(SEED, 1).awgn(c.iq_i16_to_c32(raw, scale), 0.3)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    # a 4-byte aligned device input (not 8): same bits
    din, dout = c.DeviceBuf(4 * n + 16), c.DeviceBuf(8 * n)
    din.upload(raw, offset=4)
    src = c.NoiseSource(SEED, 1).set_input_format("i16", scale)
    src.awgn_dev(din.ptr + 4, n, 0.3, dout.ptr)
    assert np.array_equal(dout.download(np.complex64, n).view(np.uint64), a.view(np.uint64))


# ------------------------------------------------------------------ bit-for-bit self-consistency
def _cuts(rng, total, k, step=1):
    inner = np.sort(rng.choice(np.arange(1, total // step), k, replace=False)) * step
    return np.diff(np.concatenate([[0], inner, [total]]))


def test_cut_streams_equal_the_uncut_stream(c):
    rng = np.random.default_rng(11)
    total = 100003
    x = _signal(total, 4)
    whole = c.NoiseSource(SEED, 2).awgn(x, 0.5)
    src, parts, at = c.NoiseSource(SEED, 2), [], 0
    for m in _cuts(rng, total, 9):
        parts.append(src.awgn(x[at:at + m], 0.5))
        at += m
    assert np.array_equal(np.concatenate(parts).view(np.uint64), whole.view(np.uint64))
    for kind, dt in (("normal", np.float32), ("normal", np.float64), ("uniform", np.float32)):
        draw = (lambda s, m: s.normal(m, 0.5, 2.0, dtype=dt)) if kind == "normal" else (lambda s, m: s.uniform(m, -1.0, 3.0))
        whole = draw(c.NoiseSource(SEED, 2), total)
        src = c.NoiseSource(SEED, 2)
        lens = _cuts(rng, total, 9)
        assert any(int(v) % 2 for v in np.cumsum(lens)[:-1])  # odd boundaries: a pair is split between two calls
        assert np.array_equal(np.concatenate([draw(src, int(m)) for m in lens]), whole), kind
    for packed in (False, True):
        whole = c.NoiseSource(SEED, 2).bits(32 * 5000, packed=packed)
        src = c.NoiseSource(SEED, 2)
        parts = [src.bits(int(m), packed=packed) for m in _cuts(rng, 32 * 5000, 6, step=32)]
        assert np.array_equal(np.concatenate(parts), whole)


def test_host_entry_equals_device_entry_across_the_host_paths(c):
    # zero-copy staging up to 1 MiB each way, device scratch above, the chunked pipeline from 64 MiB in + out
    for n in (1000, (1 << 17) - 1, (1 << 17) + 1, 1 << 20, (1 << 22) - 3, (1 << 22) + 5):
        x = _signal(n, n)
        host = c.NoiseSource(SEED, 9).awgn(x, 1.25)
        din, dout = c.DeviceBuf(8 * n), c.DeviceBuf(8 * n)
        din.upload(x)
        c.NoiseSource(SEED, 9).awgn_dev(din.ptr, n, 1.25, dout.ptr)
        assert np.array_equal(dout.download(np.complex64, n).view(np.uint64), host.view(np.uint64)), n
    for n in (1000, (1 << 18) + 1, (1 << 22) + 3):
        d = c.DeviceBuf(8 * n)
        src = c.NoiseSource(SEED, 9)
        src.normal_dev(n, d.ptr)
        assert np.array_equal(d.download(np.float32, n), c.NoiseSource(SEED, 9).normal(n))
        src.normal_dev(n, d.ptr, f64=True)
        assert np.array_equal(d.download(np.float64, n), c.NoiseSource(SEED, 9).skip(n).normal(n, dtype=np.float64))
        src.uniform_dev(n, d.ptr)
        assert np.array_equal(d.download(np.float32, n), c.NoiseSource(SEED, 9).skip(2 * n).uniform(n))


def test_shards_skip_and_streams(c):
    n, a = 50001, 20001
    x = _signal(n, 1)
    p0 = 6
    src = c.NoiseSource(SEED, 4)
    src.pos = p0
    whole = src.awgn(x, 0.9)
    # two shards, each a handle of its own started with set_pos(p0 + 2 a)
    s0, s1 = c.NoiseSource(SEED, 4), c.NoiseSource(SEED, 4)
    s0.pos, s1.pos = p0, p0 + 2 * a
    both = np.concatenate([s0.awgn(x[:a], 0.9), s1.awgn(x[a:], 0.9)])
    assert np.array_equal(both.view(np.uint64), whole.view(np.uint64))
    # skip(n) equals drawing and discarding, for every kind
    s0, s1 = c.NoiseSource(SEED, 4), c.NoiseSource(SEED, 4)
    s0.normal(12345), s0.bits(77), s0.uniform(3), s0.awgn(x[:10], 1.0)
    s1.skip(12345).skip(3).skip(3)
    s1.skip(1 + 20)  # 12351 is odd: the complex draw first moves to 12352
    assert s0.pos == s1.pos == 12372
    assert np.array_equal(s0.normal(100), s1.normal(100))
    # the position wraps modulo 2^64
    s0.pos = (1 << 64) - 2
    got = s0.normal(6)
    assert s0.pos == 4
    z_ref = np.concatenate([nr.Source(SEED, 4, (1 << 64) - 2).normal(2), nr.Source(SEED, 4, 0).normal(4)])
    assert np.all(np.abs(got - z_ref) <= ACC * np.maximum(1.0, np.abs(z_ref)))
    # a passed stream and COMMS_STREAM_HANDLE give the same output
    from comms_rs_amd._lib import STREAM_HANDLE

    st = C.c_void_p()
    assert _lib().comms_stream_create(0, C.byref(st)) == 0
    din, d1, d2 = c.DeviceBuf(8 * n), c.DeviceBuf(8 * n), c.DeviceBuf(8 * n)
    din.upload(x)
    s0, s1 = c.NoiseSource(SEED, 4), c.NoiseSource(SEED, 4)
    s0.awgn_dev(din.ptr, n, 0.9, d1.ptr, stream=st.value)
    assert _lib().comms_stream_synchronize(0, st) == 0
    s1.awgn_dev(din.ptr, n, 0.9, d2.ptr, stream=STREAM_HANDLE)
    s1.awgn(x[:1], 0.0)  # a host call on the handle's stream: synchronises it
    assert np.array_equal(d1.download(np.uint64, n), d2.download(np.uint64, n))
    assert _lib().comms_stream_destroy(0, st) == 0
    # different `stream` values of the source differ, and so do different seeds
    base = c.NoiseSource(SEED, 4).normal(4096)
    assert not np.array_equal(base, c.NoiseSource(SEED, 5).normal(4096))
    assert not np.array_equal(base, c.NoiseSource(SEED + 1, 4).normal(4096))
    assert abs(np.corrcoef(base, c.NoiseSource(SEED, 5).normal(4096))[0, 1]) < 0.1


# ------------------------------------------------------------------ refusals
def test_refusals_leave_the_position_alone(c):
    L = _lib()
    src = c.NoiseSource(SEED, 0)
    src.pos = 41
    d = c.DeviceBuf(4096)
    inf, nan = float("inf"), float("nan")
    E = c.COMMS_ERR_ARG
    assert L.comms_noise_bits_run_dev(src._h, 64, 7, d.ptr, None) == E
    assert L.comms_noise_bits_run_dev(src._h, 64, 0, d.ptr + 8, None) == E
    assert L.comms_noise_bits_run_dev(src._h, 64, 0, None, None) == E
    host = np.zeros(64, np.float64)
    assert L.comms_noise_bits_run(src._h, 64, 2, host.ctypes.data) == E
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (0.0, inf), (-inf, 0.0), (nan, 1.0), (0.0, nan)):
        assert L.comms_noise_uniform_run_dev(src._h, 8, lo, hi, d.ptr, None) == E, (lo, hi)
        assert L.comms_noise_uniform_run(src._h, 8, lo, hi, host.ctypes.data) == E, (lo, hi)
    assert L.comms_noise_uniform_run_dev(src._h, 8, 0.0, 1.0, d.ptr + 4, None) == E
    for mu, sd in ((0.0, -1.0), (0.0, inf), (0.0, nan), (nan, 1.0), (inf, 1.0)):
        assert L.comms_noise_normal_run_dev(src._h, 8, mu, sd, d.ptr, None) == E, (mu, sd)
        assert L.comms_noise_normal_f64_run_dev(src._h, 8, mu, sd, d.ptr, None) == E, (mu, sd)
        assert L.comms_noise_normal_run(src._h, 8, mu, sd, host.ctypes.data) == E, (mu, sd)
        assert L.comms_noise_normal_f64_run(src._h, 8, mu, sd, host.ctypes.data) == E, (mu, sd)
    assert L.comms_noise_normal_run_dev(src._h, 8, 0.0, 1.0, d.ptr + 4, None) == E
    assert L.comms_noise_normal_f64_run_dev(src._h, 8, 0.0, 1.0, d.ptr + 8, None) == E
    for sigma in (-0.5, inf, nan):
        assert L.comms_awgn_run_dev(src._h, d.ptr, 8, sigma, d.ptr, None) == E, sigma
        assert L.comms_awgn_run(src._h, host.ctypes.data, 4, sigma, host.ctypes.data) == E, sigma
    assert L.comms_awgn_run_dev(src._h, d.ptr + 8, 8, 1.0, d.ptr + 1024, None) == E   # c32 input: 16-byte aligned
    assert L.comms_awgn_run_dev(src._h, d.ptr, 8, 1.0, d.ptr + 1032, None) == E
    assert L.comms_awgn_run_dev(src._h, d.ptr, 8, 1.0, d.ptr + 16, None) == E         # partial overlap
    assert L.comms_awgn_run_dev(src._h, None, 8, 1.0, d.ptr, None) == E
    for fmt in (2, 3, -1):
        assert L.comms_awgn_set_input_format(src._h, fmt, 1.0) == E
    assert L.comms_awgn_set_input_format(src._h, 1, inf) == E
    assert L.comms_awgn_set_input_format(src._h, 1, 0.5) == 0
    assert L.comms_awgn_run_dev(src._h, d.ptr + 2, 8, 1.0, d.ptr + 1024, None) == E   # i16 input: 4-byte aligned
    assert src.pos == 41
    # n == 0 is a no-op, position included (no move to an even word either)
    assert L.comms_awgn_run_dev(src._h, None, 0, 1.0, None, None) == 0
    assert L.comms_noise_bits_run_dev(src._h, 0, 0, None, None) == 0
    assert L.comms_noise_normal_run(src._h, 0, 0.0, 1.0, None) == 0
    assert src.pos == 41
    with pytest.raises(ValueError):
        src.set_input_format("u8")


# ------------------------------------------------------------------ the link, all on the device
MASK32, STATE32 = 0xD04FBB5A, 0x12345678  # a maximal 32-bit PRNS mask (tests/test_tx_ref.py)


def link_setup(c, k):
    taps = c.rrc_taps(nr.LINK_TAPS, float(nr.LINK_SPS), nr.LINK_BETA)
    h = taps.real.astype(np.float64)
    return taps, h, nr.link_scale(h, k)


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("sigma", nr.LINK_SIGMAS + (0.0,))
def test_link_error_count_against_the_reference_link(c, k, sigma):
    """PRNS -> pulse shaper (packed-bit input, i16 output) -> AWGN (i16 input) -> chain (bits output) -> comms_bit_errors,
    every buffer on the device.  The reference link (noise_ref.sample_link) runs from the same wire samples with the
    reference's noise; E_ref is its error count and m the number of its decision variables within delta of the threshold,
    the only ones the device may decide differently: |E_gpu - E_ref| <= m, with m <= 1e-3 of the symbols and m < E_ref / 4
    (tests/test_noise_ref.py checks the same condition for these noise levels without a GPU)."""
    n_sym = 1 << 18
    LINK_SPS = nr.LINK_SPS
    n = n_sym * LINK_SPS
    taps, h, scale = link_setup(c, k)
    delay = (nr.LINK_TAPS - 1) // LINK_SPS
    n_bytes = n_sym * k // 8
    dbits, dwire, drx, dout = c.DeviceBuf(n_bytes), c.DeviceBuf(4 * n), c.DeviceBuf(8 * n), c.DeviceBuf(n_bytes)
    c.PrnsNode(MASK32, STATE32, 32).run_dev(n_sym * k, dbits.ptr, packed=True)
    tx = c.PulseNode(taps, LINK_SPS).set_input_format("bits", k).set_output_format("i16", scale)
    tx.run_dev(dbits.ptr, n_sym, dwire.ptr)
    rx_scale = float(np.float32(1.0 / scale))
    chan = c.NoiseSource(SEED, 100 + k).set_input_format("i16", rx_scale)
    chan.awgn_dev(dwire.ptr, n, sigma, drx.ptr)
    rx = c.ChainNode(0.0, 0.0, taps, LINK_SPS, False).set_output_format("bits", k)
    rx.run_dev(drx.ptr, n, dout.ptr)
    n_cmp = (n_sym - delay) * k
    assert (delay * k) % 8 == 0
    e_gpu = c.bit_errors_dev(dout.ptr + delay * k // 8, dbits.ptr, n_cmp)
    if sigma == 0.0:
        assert e_gpu == 0
        return
    bits = np.unpackbits(dbits.download(np.uint8, n_bytes), bitorder="little")
    wire = dwire.download(np.int16, 2 * n).reshape(-1, 2)
    noise = nr.Source(SEED, 100 + k).complex_normal(n)
    e_ref, n_ref, d = nr.sample_link(bits, k, h, LINK_SPS, scale, sigma, noise, wire=wire, rx_scale=rx_scale)
    assert n_ref == n_cmp
    rx_max = float(np.max(np.abs(wire))) * rx_scale + sigma * max(np.max(np.abs(noise.real)), np.max(np.abs(noise.imag)))
    delta = nr.link_delta(h, sigma, noise, rx_max, ACC, TOL)
    m = int(np.count_nonzero(np.abs(d) < delta))
    print("k=%d sigma=%.2f: E_gpu=%d E_ref=%d of %d bits, m=%d (delta %.3e)" % (k, sigma, e_gpu, e_ref, n_cmp, m, delta))
    assert m <= 1e-3 * n_sym and m < e_ref / 4
    assert abs(e_gpu - e_ref) <= m
