"""ResampleNode (comms_resample_*): upsample by L, FIR, decimate by M over an f32 or Complex<f32> stream -- one launch
(resample_kernel) or, beyond its range, the reference's nodes in series -- against tests/resample_ref.py, the float64
polyphase formula that tests/test_resample_ref.py pins to the oracle's composition, and for one case of each dtype against
that composition directly.  Bound: the project's f32 FIR bound max|d| <= 1e-5 sum|taps| max|x| (TOL of
tests/test_gpu_parity.py), x being the samples the outputs are made of (the call's and the history's)."""
import json
import os
import subprocess

import numpy as np
import pytest

import oracle
from resample_ref import ResampleRef, close, out_len, state_len, unit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.complex64]


@pytest.fixture(scope="module")
def c():
    import comms_rs_amd as c

    assert c.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested (no CPU fallback)"
    return c


def rand(rng, n, dtype):
    if np.dtype(dtype).kind == "c":
        return (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(dtype)
    return rng.uniform(-1, 1, n).astype(dtype)


def make_taps(rng, n_taps):
    return rng.uniform(-1, 1, n_taps).astype(np.float32)


def run_dev(c, node, x):
    """The device entry on device buffers (legacy stream), downloaded."""
    n, m, e = x.size, node.out_len(x.size), x.dtype.itemsize
    din, dout = c.DeviceBuf(max(e * n, e)).upload(x), c.DeviceBuf(max(e * m, e))
    node.run_dev(din.ptr, n, dout.ptr)
    return dout.download(x.dtype, m)


def oracle_series(x, taps, L, M, state):
    u = oracle.upsample(x, L)
    y = oracle.batch_fir(u.astype(np.complex64), taps.astype(np.complex64), state, norotate=True)
    return oracle.decimate(y if x.dtype.kind == "c" else y.real.copy(), M)


# ------------------------------------------------------------------ 1. parity grid
# the issue's list, then two of this kernel's own corners: a table that stays in global memory (complex, one phase of 6144
# taps) and the smallest tiles (32 outputs of 64 input samples each beside 1536 taps per phase)
GRID = [(3, 2, 64), (2, 3, 63), (147, 152, 3528), (147, 152, 1000), (160, 147, 1601), (5, 5, 33), (1, 5, 63), (4, 1, 32), (7, 3, 5),
        (0, 0, 9), (6, 4, 13), (256, 1, 2048), (1, 64, 257), (64, 256, 1025), (1, 3, 6144), (4, 256, 6144)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L,M,N", GRID)
def test_parity_grid(c, L, M, N, dtype):
    rng = np.random.default_rng(1000 + 7 * L + 3 * M + N)
    taps = make_taps(rng, N)
    u = unit(L, M)
    for n in sorted({1, max(u - 1, 1), u, 4097, 20011}):
        x = rand(rng, n, dtype)
        node = c.ResampleNode(taps, L, M, dtype)
        assert "resample_kernel" in node.kernel(n), (L, M, N, n, node.kernel(n))
        got = node.run(x)
        assert got.shape == (node.out_len(n),) == (out_len(n, L, M),) and got.dtype == dtype
        ref = ResampleRef(taps, L, M, dtype)
        want = ref.run(x)
        close(got, want, taps, ref.x_max, (L, M, N, n))
        if N <= max(L, 1):   # phases without a tap: exactly 0.0
            j = np.arange(got.size)
            assert np.all(got[(j * max(M, 1)) % max(L, 1) >= N] == 0)
    if (L, M, N) == (1, 3, 6144):
        assert ("global" in node.kernel(n)) == (np.dtype(dtype).kind == "c"), node.kernel(n)


@pytest.mark.parametrize("L,M,N,n,dtype", [(3, 2, 64, 20011, np.float32), (147, 152, 1000, 4097, np.complex64)])
def test_parity_with_the_oracle_composition(c, L, M, N, n, dtype):
    """The GPU path against the reference's three nodes themselves, not through resample_ref: two calls, state carried."""
    rng = np.random.default_rng(1500 + L)
    taps = make_taps(rng, N)
    node = c.ResampleNode(taps, L, M, dtype)
    state = oracle.default_state(taps.astype(np.complex64))
    x_max = 0.0
    for k in (n, 777):
        x = rand(rng, k, dtype)
        x_max = max(x_max, float(np.max(np.abs(x))))
        assert "resample_kernel" in node.kernel(k)
        close(node.run(x), oracle_series(x, taps, L, M, state), taps, x_max, (L, M, N, k))
    Q = node.state_len()
    mapped = state[L - 1::L][:Q]
    assert np.array_equal(node.get_state(), mapped if np.dtype(dtype).kind == "c" else mapped.real)


# ------------------------------------------------------------------ 2. beyond the kernel's range: the series
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L,M,N,n", [(300, 7, 1200, 4097), (3, 2, 40000, 3000), (1, 100, 63, 20011)])
def test_series_beyond_the_kernels_range(c, L, M, N, n, dtype):
    rng = np.random.default_rng(2000 + L + N)
    taps = make_taps(rng, N)
    node = c.ResampleNode(taps, L, M, dtype)
    ref = ResampleRef(taps, L, M, dtype)
    for k in (n, 1001):
        x = rand(rng, k, dtype)
        name = node.kernel(k)
        assert "series" in name and "resample_kernel" not in name, name
        got = node.run(x)
        assert got.shape == (out_len(k, L, M),)
        close(got, ref.run(x), taps, ref.x_max, (L, M, N, k))


# ------------------------------------------------------------------ 3. state across ragged calls
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L,M,N", [(147, 152, 3528), (3, 2, 64), (2, 3, 63), (1, 5, 63), (4, 1, 32), (300, 7, 1200), (7, 3, 5)])
def test_state_across_ragged_calls(c, L, M, N, dtype):
    rng = np.random.default_rng(3000 + L + N)
    taps = make_taps(rng, N)
    node = c.ResampleNode(taps, L, M, dtype)
    ref = ResampleRef(taps, L, M, dtype)
    Q = state_len(N, L)
    assert node.state_len() == Q
    seen = np.zeros(Q, dtype)
    for n in (1, 7, 4096, 33, 10001, 2, 1):
        x = rand(rng, n, dtype)
        got = node.run(x)
        close(got, ref.run(x), taps, ref.x_max, (L, M, N, n))
        seen = np.concatenate([seen, x])[-Q:] if Q else seen
        if Q == 0:   # no state: the call is what a fresh node gives, bit for bit
            assert np.array_equal(got, c.ResampleNode(taps, L, M, dtype).run(x))
    assert np.array_equal(node.get_state(Q), seen[::-1])   # the last Q inputs, newest first
    assert (Q == 0) == ((L, M, N) == (7, 3, 5))


# ------------------------------------------------------------------ 4. cut invariance, bit for bit
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L,M,N", [(147, 152, 3528), (3, 2, 64), (2, 3, 63), (6, 4, 13), (64, 256, 1025)])
def test_cut_invariance_bit_for_bit(c, L, M, N, dtype):
    rng = np.random.default_rng(4000 + L + N)
    taps = make_taps(rng, N)
    units, u = 4000, unit(L, M)
    x = rand(rng, units * u, dtype)
    node = c.ResampleNode(taps, L, M, dtype)
    assert "resample_kernel" in node.kernel(x.size)
    whole = node.run(x)
    many = sorted(set(int(v) for v in rng.integers(1, units, 40)))
    for cuts in ([units // 2], [1, units - 1], many):
        node = c.ResampleNode(taps, L, M, dtype)
        edges = [0] + [k * u for k in cuts] + [x.size]
        got = np.concatenate([node.run(x[a:b]) for a, b in zip(edges[:-1], edges[1:])])
        assert np.array_equal(got, whole), (L, M, N, cuts[:4])


# ------------------------------------------------------------------ 5. checkpoint / shard hooks
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L,M,N", [(147, 152, 3528), (3, 2, 64), (300, 7, 1200)])
def test_checkpoint_and_shard_hooks(c, L, M, N, dtype):
    rng = np.random.default_rng(5000 + L + N)
    taps = make_taps(rng, N)
    half = 30 * unit(L, M)
    x = rand(rng, 2 * half, dtype)
    Q = state_len(N, L)
    one = c.ResampleNode(taps, L, M, dtype)
    a, b = one.run(x[:half]), one.run(x[half:])
    first = c.ResampleNode(taps, L, M, dtype)
    first.run(x[:half])
    saved = first.get_state()
    assert np.array_equal(saved, x[:half][::-1][:Q])
    fresh = c.ResampleNode(taps, L, M, dtype)
    fresh.set_state(saved)
    assert np.array_equal(fresh.get_state(), saved)
    got = fresh.run(x[half:])
    if "resample_kernel" in one.kernel(half):
        assert np.array_equal(got, b)
        assert np.array_equal(np.concatenate([a, b]), c.ResampleNode(taps, L, M, dtype).run(x))
    else:   # the series filters in the frequency domain, its segments fall where the call does: within the bound
        ref = ResampleRef(taps, L, M, dtype)
        ref.run(x[:half])
        want = ref.run(x[half:])
        close(got, want, taps, ref.x_max, "series, restored")
        close(b, want, taps, ref.x_max, "series, carried")


# ------------------------------------------------------------------ 6. host entry == device entry
@pytest.mark.parametrize("L,M,N,n,dtype", [(147, 152, 3528, 10000, np.float32), (3, 2, 64, 10000, np.complex64),
                                             (3, 2, 64, 1 << 23, np.complex64), (300, 7, 1200, 10000, np.float32)])
def test_host_entry_equals_device_entry(c, L, M, N, n, dtype):
    """Short calls run on zero-copy staging, longer ones through device scratch; (3, 2, 64) complex at 2^23 samples moves
    64 MiB in and 96 MiB out, which the host entry cuts into pipelined chunks of whole units of M / gcd input samples."""
    rng = np.random.default_rng(6000 + L)
    taps = make_taps(rng, N)
    x = rand(rng, n, dtype)
    host = c.ResampleNode(taps, L, M, dtype).run(x)
    dev = run_dev(c, c.ResampleNode(taps, L, M, dtype), x)
    assert host.shape == (out_len(n, L, M),) and np.array_equal(host, dev)


# ------------------------------------------------------------------ 7. arguments
def test_arguments(c):
    import ctypes as C

    from comms_rs_amd import _lib

    lib = _lib.lib()
    t = np.ones(4, np.float32)
    h = C.c_void_p()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.comms_resample_create(p(t), 0, 3, 2, 4, 0, C.byref(h)) == 1 and not h          # n_taps == 0
    assert lib.comms_resample_create(None, 4, 3, 2, 4, 0, C.byref(h)) == 1 and not h          # NULL taps
    assert lib.comms_resample_create(p(t), 4, 3, 2, 2, 0, C.byref(h)) == 1 and not h          # elem neither 4 nor 8
    assert lib.comms_resample_create(p(t), 4, 3, 2, 4, 0, None) == 1                         # NULL out
    with pytest.raises(c.CommsError) as e:
        c.ResampleNode(np.zeros(0, np.float32), 3, 2)
    assert e.value.code == 1
    rng = np.random.default_rng(7)
    for L, M, N, dtype in ((3, 2, 64, np.float32), (3, 2, 64, np.complex64), (300, 7, 1200, np.float32), (300, 7, 1200, np.complex64)):
        e = np.dtype(dtype).itemsize
        node = c.ResampleNode(make_taps(rng, N), L, M, dtype)
        Q = node.state_len()
        assert Q == (N - 1) // L and Q >= 3
        node.set_state(rand(rng, Q, dtype))
        before = node.get_state()
        assert node.run(np.zeros(0, dtype)).shape == (0,)                                     # n == 0: OK, nothing written
        assert lib.comms_resample_run_dev(node._h, None, 0, None, None) == 0
        assert lib.comms_resample_run(node._h, None, 0, None) == 0
        assert np.array_equal(node.get_state(), before)                                       #   ... and the state stays
        assert lib.comms_resample_run_dev(node._h, None, 8, None, None) == 1                  # NULL device pointers
        assert lib.comms_resample_run(node._h, None, 8, None) == 1
        assert lib.comms_resample_run_dev(None, None, 0, None, None) == 1                     # NULL handle
        assert lib.comms_resample_get_state(node._h, None, 1) == 1
        assert lib.comms_resample_get_state(node._h, p(before), Q + 1) == 1                   # more than the state
        assert np.array_equal(node.get_state(2), before[:2])                                  # fewer: the newest
        assert lib.comms_resample_set_state(node._h, p(before), Q - 1) == 1                   # not exactly the state
        assert lib.comms_resample_set_state(node._h, p(before), Q + 1) == 1
        assert lib.comms_resample_get_kernel(node._h, 8, None, 0) == 1
        buf = c.DeviceBuf(256)
        assert lib.comms_resample_run_dev(node._h, buf.ptr, 8, buf.ptr, None) == 1            # in place
        assert lib.comms_resample_run_dev(node._h, buf.ptr, 8, buf.ptr + e * 4, None) == 1    # overlapping
        assert lib.comms_resample_run_dev(node._h, buf.ptr + e // 2, 2, buf.ptr + 128, None) == 1   # misaligned
        assert lib.comms_resample_run_dev(node._h, buf.ptr, 1 << 62, buf.ptr + 128, None) == 1      # n * up overflows
        assert np.array_equal(node.get_state(), before)                                       # refused calls change nothing
    assert lib.comms_resample_destroy(None) == 0
    assert lib.comms_resample_set_timer(None, None) == 1


# ------------------------------------------------------------------ 8. timer
@pytest.mark.parametrize("L,M,N", [(147, 152, 3528), (300, 7, 1200)])
def test_kernel_timer_brackets_the_launch(c, L, M, N):
    rng = np.random.default_rng(8)
    x = rand(rng, 1 << 14, np.float32)
    node = c.ResampleNode(make_taps(rng, N), L, M)
    timer = c.KernelTimer(8).attach(node)
    for _ in range(3):
        node.run(x)
    ms = timer.read_ms()
    assert ms.size == 3 and np.all(ms > 0) and np.all(ms < 100)
    node.set_timer(None)
    node.run(x)
    assert timer.read_ms().size == 3
    timer.close()


# ------------------------------------------------------------------ 9. the example's missing stage
def test_fm_radio_audio_to_the_sound_cards_rate(c):
    """examples/fm_radio.rs:57,146-154: 1 140 000 samples/s, two decimators by 5, 45 600 Hz of audio into a 44 100 Hz sink --
    the stage the example leaves open is 147/152.  Front end as test_fm_radio_example_in_two_launches
    (tests/test_gpu_real_chain.py) builds it: ChainNode on u8 input -> RealFirDecimNode; then ResampleNode."""
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_kats.json")))["fm_radio_taps"]
    t32 = np.asarray(g["taps_re"], np.float32)
    taps = t32.astype(np.complex64)
    n = 262125
    idx = np.arange(n, dtype=np.float64)
    xs = np.exp(1j * (-2 * np.pi * 0.05 * idx + 8.0 * np.cos(2 * np.pi * idx / 4096))).astype(np.complex64)
    u8 = np.clip(np.round(np.stack([xs.real, xs.imag], axis=1) * 127.5 + 127.5), 0, 255).astype(np.uint8)
    L, M = 147, 152
    # windowed sinc, 24 taps per phase: cutoff at the OUTPUT's Nyquist, 22 050 Hz = 0.5 / 152 of the upsampled rate
    # (147 x 45 600 Hz); gain 147 at DC, which makes up for the 146 stuffed zeros per sample
    k = np.arange(L * 24) - (L * 24 - 1) / 2.0
    lowpass = (L * (1.0 / M) * np.sinc(k / M) * np.hamming(L * 24)).astype(np.float32)
    assert abs(float(np.sum(lowpass.astype(np.float64))) / L - 1.0) < 1e-3

    front = c.ChainNode(0.0, 0.0, taps, 5, True)
    front.set_input_format("u8")
    audio = c.RealFirDecimNode(t32, 5)
    rs = c.ResampleNode(lowpass, L, M)
    m1, m2 = n // 5, -(-(n // 5) // 5)
    m3 = -(-m2 * L // M)
    assert "resample_kernel" in rs.kernel(m2)
    mid = audio.run(front.run(u8))          # the GPU's own 45 600 Hz audio
    got = rs.run(mid)
    assert mid.shape == (m2,) and got.shape == (m3,) == (rs.out_len(m2),)
    ref = ResampleRef(lowpass, L, M)
    close(got, ref.run(mid), lowpass, ref.x_max, "fm_radio audio")
    # on the device: three launches back to back on one stream, nothing leaving it in between
    din, d1, d2, d3 = c.DeviceBuf(u8.size).upload(u8), c.DeviceBuf(4 * m1), c.DeviceBuf(4 * m2), c.DeviceBuf(4 * m3)
    front2 = c.ChainNode(0.0, 0.0, taps, 5, True)
    front2.set_input_format("u8")
    audio2, rs2 = c.RealFirDecimNode(t32, 5), c.ResampleNode(lowpass, L, M)
    front2.run_dev(din.ptr, n, d1.ptr)
    audio2.run_dev(d1.ptr, m1, d2.ptr)
    rs2.run_dev(d2.ptr, m2, d3.ptr)
    assert np.array_equal(d3.download(np.float32, m3), got)


# ------------------------------------------------------------------ 10. the C++ graph
def test_cpp_resample_nodes_graph():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "comms_rs_amd", "host"), "-s"], timeout=600)
    out = subprocess.run([os.path.join(ROOT, "comms_rs_amd", "lib", "test_resample_nodes_gpu")], capture_output=True,
                         text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all passed" in out.stdout
