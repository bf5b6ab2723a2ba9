"""RealFirDecimNode (comms_rfir_*): FIR + decimator over a real f32 stream, against the reference graph it stands for --
Convert2Node -> BatchFirNode<f32>(Complex(h, 0), state) -> Convert3Node -> DecimateNode<f32>(R) (examples/fm_radio.rs:98-152)
-- restated with the oracle's nodes: oracle.decimate(oracle.batch_fir(complex(x), complex(h), state).real, R), call by call.
Bounds: the project's f32 FIR bound max|d| <= 1e-5 sum|taps| max|x| (TOL of tests/test_gpu_parity.py), nothing new."""
import json
import os
import subprocess

import numpy as np
import pytest

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

TOL = 1e-5


@pytest.fixture(scope="module")
def c():
    import comms_rs_amd as c

    assert c.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested (no CPU fallback)"
    return c


def fm_radio_taps():
    """The 63 taps examples/fm_radio.rs:30-52 ships (tests/golden/reference_kats.json), as f32."""
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_kats.json")))["fm_radio_taps"]
    taps = np.asarray(g["taps_re"], np.float32)
    assert taps.size == g["n_taps"] == 63 and g["dec_rate"] == 5
    return taps


def make_taps(rng, n_taps):
    return fm_radio_taps() if n_taps == 63 else rng.uniform(-1, 1, n_taps).astype(np.float32)


def ref_fir(x, taps, state):
    """The reference's three middle nodes: complex cast, batch_fir (state: complex64, newest first, updated), .re"""
    return oracle.batch_fir(x.astype(np.complex64), taps.astype(np.complex64), state, norotate=True).real.copy()


def ref_state(taps, state=None):
    return oracle.default_state(taps.astype(np.complex64)) if state is None else np.ascontiguousarray(state, np.float32).astype(np.complex64)


def close(got, want, taps, x, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bound = TOL * float(np.sum(np.abs(taps))) * max(float(np.max(np.abs(x), initial=0.0)), 1e-30)
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert d.max(initial=0.0) <= bound, (what, float(d.max()), bound, int(np.argmax(d)))


def out_len(n, rate):
    return n if rate <= 1 else -(-n // rate)


def run_dev(c, node, x):
    """The device entry on device buffers (legacy stream), downloaded."""
    n = x.size
    m = node.out_len(n)
    din, dout = c.DeviceBuf(max(4 * n, 4)).upload(x), c.DeviceBuf(max(4 * m, 4))
    node.run_dev(din.ptr, n, dout.ptr)
    return dout.download(np.float32, m)


# ------------------------------------------------------------------ 1. parity grid
GRID_TAPS = [1, 2, 5, 31, 63, 64, 127, 255, 257]
GRID_RATES = [0, 1, 2, 3, 5, 8, 13, 64]


@pytest.mark.parametrize("n_taps", GRID_TAPS)
def test_parity_grid(c, n_taps):
    rng = np.random.default_rng(1000 + n_taps)
    taps = make_taps(rng, n_taps)
    filtered = {}  # the FIR's output does not depend on the rate: one oracle run per length
    for rate in GRID_RATES:
        lens = [1] + ([rate - 1] if rate - 1 > 0 else []) + ([rate] if rate > 0 else []) + [4097, 262125, (1 << 20) + 3]
        for n in lens:
            if n not in filtered:
                x = rng.uniform(-1, 1, n).astype(np.float32)
                filtered[n] = (x, ref_fir(x, taps, ref_state(taps)))
            x, y = filtered[n]
            want = oracle.decimate(y, rate)
            node = c.RealFirDecimNode(taps, rate)
            assert "rfir_decim" in node.kernel(n), (rate, n, node.kernel(n))
            got = node.run(x)
            assert got.shape == (out_len(n, rate),)
            close(got, want, taps, x, (n_taps, rate, n))


# ------------------------------------------------------------------ 2. beyond the kernel's range: the series
@pytest.mark.parametrize("n_taps,rate", [(258, 5), (511, 4), (1025, 8), (63, 100)])
def test_series_beyond_the_kernels_range(c, n_taps, rate):
    rng = np.random.default_rng(2000 + n_taps)
    taps = make_taps(rng, n_taps)
    node = c.RealFirDecimNode(taps, rate)
    st = ref_state(taps)
    for n in (4097, 100003):
        x = rng.uniform(-1, 1, n).astype(np.float32)
        k = node.kernel(n)
        assert "series" in k and "rfir_decim" not in k, k
        close(node.run(x), oracle.decimate(ref_fir(x, taps, st), rate), taps, x, (n_taps, rate, n))


# ------------------------------------------------------------------ 3. state across ragged calls
@pytest.mark.parametrize("n_taps,rate", [(63, 5), (127, 8), (255, 4), (31, 1), (257, 64), (5, 13), (511, 4)])
def test_state_across_ragged_calls(c, n_taps, rate):
    rng = np.random.default_rng(3000 + n_taps)
    taps = make_taps(rng, n_taps)
    node = c.RealFirDecimNode(taps, rate)
    st = ref_state(taps)
    for n in (1, 7, 4096, 33, 100001, 2, 1):
        x = rng.uniform(-1, 1, n).astype(np.float32)
        close(node.run(x), oracle.decimate(ref_fir(x, taps, st), rate), taps, x, (n_taps, rate, n))
    assert np.array_equal(node.get_state(min(n_taps, 16)), st.real[:min(n_taps, 16)])  # newest first, as the reference keeps it


# ------------------------------------------------------------------ 4. cut invariance, bit for bit
@pytest.mark.parametrize("n_taps,rate", [(63, 5), (127, 8), (255, 4), (31, 1), (257, 64), (64, 13), (2, 3)])
def test_cut_invariance_bit_for_bit(c, n_taps, rate):
    rng = np.random.default_rng(4000 + n_taps)
    taps = make_taps(rng, n_taps)
    units = 40000
    x = rng.uniform(-1, 1, units * rate).astype(np.float32)
    whole = c.RealFirDecimNode(taps, rate).run(x)
    many = sorted(set(int(v) for v in rng.integers(1, units, 60)))
    for cuts in ([units // 2], [1, units - 1], [units // 3, units // 3 + 1283], many):
        node = c.RealFirDecimNode(taps, rate)
        edges = [0] + [u * rate for u in cuts] + [x.size]
        got = np.concatenate([node.run(x[a:b]) for a, b in zip(edges[:-1], edges[1:])])
        assert np.array_equal(got, whole), (n_taps, rate, cuts[:4])


# ------------------------------------------------------------------ 5. checkpoint / shard hooks
@pytest.mark.parametrize("n_taps,rate", [(63, 5), (255, 4), (511, 4)])
def test_checkpoint_and_shard_hooks(c, n_taps, rate):
    rng = np.random.default_rng(5000 + n_taps)
    taps = make_taps(rng, n_taps)
    half = 12000 * rate
    x = rng.uniform(-1, 1, 2 * half).astype(np.float32)
    one = c.RealFirDecimNode(taps, rate)
    a, b = one.run(x[:half]), one.run(x[half:])
    # checkpoint: the state after a call, into a fresh node
    first = c.RealFirDecimNode(taps, rate)
    assert np.array_equal(first.run(x[:half]), a)
    saved = first.get_state(n_taps)
    assert np.array_equal(saved, x[:half][::-1][:n_taps])
    fresh = c.RealFirDecimNode(taps, rate)
    fresh.set_state(saved)
    assert np.array_equal(fresh.run(x[half:]), b)
    # shard: the second half on a node created with the halo (the last n_taps samples of the first half, newest first)
    second = c.RealFirDecimNode(taps, rate, state=x[:half][::-1][:n_taps].copy())
    assert np.array_equal(second.run(x[half:]), b)
    uncut = c.RealFirDecimNode(taps, rate)
    if "rfir_decim" in uncut.kernel(x.size):
        assert np.array_equal(np.concatenate([a, b]), uncut.run(x))
    else:  # the series filters in the frequency domain: where its segments fall depends on the call, so both forms are
        #    held to the f32 FIR bound against the reference instead
        want = oracle.decimate(ref_fir(x, taps, ref_state(taps)), rate)
        close(np.concatenate([a, b]), want, taps, x, "series, two calls")
        close(uncut.run(x), want, taps, x, "series, one call")


@pytest.mark.parametrize("n_taps,n_state,rate", [(63, 10, 5), (127, 1, 8), (31, 40, 2), (300, 258, 3)])
def test_user_state_shorter_than_the_taps_truncates(c, n_taps, n_state, rate):
    """zip(taps, state) (fir.rs:53): only min(n_taps, n_state) taps take part"""
    rng = np.random.default_rng(5500 + n_taps)
    taps = make_taps(rng, n_taps)
    state = rng.uniform(-1, 1, n_state).astype(np.float32)
    node = c.RealFirDecimNode(taps, rate, state=state)
    st = ref_state(taps, state)
    for n in (777, 5000):
        x = rng.uniform(-1, 1, n).astype(np.float32)
        close(node.run(x), oracle.decimate(ref_fir(x, taps, st), rate), taps, x, (n_taps, n_state, rate, n))


# ------------------------------------------------------------------ 6. host entry == device entry
@pytest.mark.parametrize("n_taps,rate,n", [(63, 5, 10000), (63, 5, 262125), (127, 8, 3 << 20), (63, 1, 1 << 24), (511, 4, 50001)])
def test_host_entry_equals_device_entry(c, n_taps, rate, n):
    """Short calls run on zero-copy staging, longer ones through device scratch; (63, 1, 2^24) moves 64 MiB each way, which
    the host entry cuts into pipelined chunks of whole units -- at rate >= 5 the output is too small a share for that
    and the call is a single shot.  All of them: the bits of run_dev."""
    rng = np.random.default_rng(6000 + n_taps + rate)
    taps = make_taps(rng, n_taps)
    x = rng.uniform(-1, 1, n).astype(np.float32)
    host = c.RealFirDecimNode(taps, rate).run(x)
    dev = run_dev(c, c.RealFirDecimNode(taps, rate), x)
    assert host.shape == (out_len(n, rate),) and np.array_equal(host, dev)


# ------------------------------------------------------------------ 7. the literal example in two launches
def fm_stream(n, first=0):
    idx = np.arange(first, first + n, dtype=np.float64)
    phase = -2 * np.pi * 0.05 * idx + 8.0 * np.cos(2 * np.pi * idx / 4096)
    return np.exp(1j * phase).astype(np.complex64)


def circ(d):
    d = np.abs(d)
    return np.minimum(d, 2 * np.pi - d)


def test_fm_radio_example_in_two_launches(c):
    """examples/fm_radio.rs:144-152 as ChainNode (u8 bytes -> 63 taps -> /5 -> FM demod) -> RealFirDecimNode (63 taps, /5), on
    the input and against the expected values of test_fm_radio_example_chain (tests/test_gpu_parity.py), with its bounds:
    angles by circular error x min(|y[j]|, |y[j-1]|) <= 4 TOL sum|taps| (and a flat 1e-4 rad where the magnitude is above
    0.5, behind the first filter's start-up); audio outputs by convolve(angle bound, |taps|)[::5] + TOL sum|taps| pi."""
    t32 = fm_radio_taps()
    taps = t32.astype(np.complex64)
    n = 262125
    x = fm_stream(n)
    u8 = np.clip(np.round(np.stack([x.real, x.imag], axis=1) * 127.5 + 127.5), 0, 255).astype(np.uint8)
    xin = oracle.iq_u8_to_c32(u8)
    scale = float(np.sum(np.abs(taps)))
    skip = taps.size // 5 + 1
    wy = oracle.decimate(oracle.batch_fir(xin, taps, oracle.default_state(taps), norotate=True), 5)
    w = oracle.FM().demod(wy)
    w2 = oracle.decimate(oracle.batch_fir(w.astype(np.complex64), taps, oracle.default_state(taps), norotate=True).real.copy(), 5)
    mag = np.minimum(np.abs(wy), np.abs(np.concatenate([[1.0], wy[:-1]]))).astype(np.float64)

    front = c.ChainNode(0.0, 0.0, taps, 5, True)
    front.set_input_format("u8")
    audio = c.RealFirDecimNode(t32, 5)
    assert "rfir_decim" in audio.kernel(n // 5)
    gf = front.run(u8)
    d = circ(gf.astype(np.float64) - w)
    worst = int(np.argmax(d * mag))
    assert gf.shape == w.shape and d[worst] * mag[worst] <= 4 * TOL * scale, (worst, d[worst], mag[worst])
    ok = mag > 0.5
    ok[:skip] = False
    assert float(np.max(d[ok])) <= 1e-4
    angle_bound = np.minimum(4 * TOL * scale / np.maximum(mag, 1e-30), np.pi)
    bound = (np.convolve(angle_bound, np.abs(t32).astype(np.float64))[:angle_bound.size] + TOL * scale * np.pi)[::5]
    g2 = audio.run(gf)
    assert g2.shape == w2.shape == (-(-(-(-n // 5)) // 5),)
    dd = np.abs(g2.astype(np.float64) - w2)
    worst = int(np.argmax(dd / bound))
    assert dd[worst] <= bound[worst], (worst, dd[worst], bound[worst])
    # on the device, the two launches back to back on one stream, the angles never leaving it
    m1, m2 = n // 5, -(-(n // 5) // 5)
    din, dmid, dout = c.DeviceBuf(u8.size).upload(u8), c.DeviceBuf(4 * m1), c.DeviceBuf(4 * m2)
    front2 = c.ChainNode(0.0, 0.0, taps, 5, True)
    front2.set_input_format("u8")
    audio2 = c.RealFirDecimNode(t32, 5)
    front2.run_dev(din.ptr, n, dmid.ptr)
    audio2.run_dev(dmid.ptr, m1, dout.ptr)
    assert np.array_equal(dout.download(np.float32, m2), g2)


# ------------------------------------------------------------------ 8. arguments
def test_arguments(c):
    import ctypes as C

    from comms_rs_amd import _lib

    lib = _lib.lib()
    t = np.ones(4, np.float32)
    h = C.c_void_p()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.comms_rfir_create(p(t), 0, None, 0, 5, 0, C.byref(h)) == 1 and not h          # n_taps == 0
    assert lib.comms_rfir_create(None, 4, None, 0, 5, 0, C.byref(h)) == 1 and not h          # NULL taps
    assert lib.comms_rfir_create(p(t), 4, p(t), 0, 5, 0, C.byref(h)) == 1 and not h          # empty user state
    assert lib.comms_rfir_create(p(t), 4, None, 0, 5, 0, None) == 1                         # NULL out
    with pytest.raises(c.CommsError) as e:
        c.RealFirDecimNode(np.zeros(0, np.float32), 5)
    assert e.value.code == 1
    with pytest.raises(c.CommsError) as e:
        c.RealFirDecimNode(t, 5, state=np.zeros(0, np.float32))
    assert e.value.code == 1
    for taps, rate in ((t, 5), (np.ones(300, np.float32), 5)):
        node = c.RealFirDecimNode(taps, rate, state=np.arange(1, taps.size + 1, dtype=np.float32))
        before = node.get_state(taps.size)
        assert node.run(np.zeros(0, np.float32)).shape == (0,)                               # n == 0: OK, nothing written
        assert lib.comms_rfir_run_dev(node._h, None, 0, None, None) == 0
        assert np.array_equal(node.get_state(taps.size), before)                             #   ... and the state stays
        assert lib.comms_rfir_run_dev(node._h, None, 8, None, None) == 1                     # NULL device pointers
        assert lib.comms_rfir_run(node._h, None, 8, None) == 1
        assert lib.comms_rfir_run_dev(None, None, 0, None, None) == 1                        # NULL handle
        assert lib.comms_rfir_get_state(node._h, None, 1) == 1
        assert lib.comms_rfir_get_state(node._h, p(before), taps.size + 1) == 1              # more than the taps
        assert lib.comms_rfir_set_state(node._h, p(before), taps.size - 1) == 1              # not exactly the taps
        assert lib.comms_rfir_get_kernel(node._h, 8, None, 0) == 1
        buf = c.DeviceBuf(64)
        assert lib.comms_rfir_run_dev(node._h, buf.ptr, 8, buf.ptr, None) == 1               # in place
        assert lib.comms_rfir_run_dev(node._h, buf.ptr + 2, 4, buf.ptr + 32, None) == 1      # misaligned
    assert lib.comms_rfir_destroy(None) == 0
    assert lib.comms_rfir_set_timer(None, None) == 1


def test_kernel_timer_brackets_the_launch(c):
    rng = np.random.default_rng(8)
    x = rng.uniform(-1, 1, 1 << 20).astype(np.float32)
    for taps in (fm_radio_taps(), rng.uniform(-1, 1, 300).astype(np.float32)):
        node = c.RealFirDecimNode(taps, 5)
        timer = c.KernelTimer(8).attach(node)
        for _ in range(3):
            node.run(x)
        ms = timer.read_ms()
        assert ms.size == 3 and np.all(ms > 0) and np.all(ms < 100)
        node.set_timer(None)
        node.run(x)
        assert timer.read_ms().size == 3
        timer.close()


# ------------------------------------------------------------------ the C++ graph: the literal example as two nodes
def test_cpp_real_nodes_graph():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "comms_rs_amd", "host"), "-s"], timeout=600)
    out = subprocess.run([os.path.join(ROOT, "comms_rs_amd", "lib", "test_real_nodes_gpu")], capture_output=True,
                         text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all passed" in out.stdout
