"""CPU check of tests/channelizer_ref.py, the float64 polyphase filter bank the GPU channelizer tests compare with: against M
instances of tests/chain_ref.ChainRef (mixer in front, dphase = -2 pi k / M, phase 0; both are f64: 1e-10 sum|h| max|x|), and
for one case against the oracle's own nodes in series -- Mixer(0, -2 pi k / M).mix -> batch_fir -> decimate per channel, in
f32, within the chain's bound -- with a ragged second call.  Also what of comms_channelizer_* needs no device: the two length
helpers, the argument checks that come before the device, and the no-CPU-fallback rule."""
import ctypes as C
import math

import numpy as np
import pytest

import oracle
from chain_ref import ChainRef, out_bound
from channelizer_ref import ChannelizerRef, check, out_len, state_len

CASES = [(4, 4, 13), (8, 3, 8), (16, 8, 70), (12, 5, 25), (1, 2, 5)]


def rand(rng, n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


@pytest.mark.parametrize("M,D,N", CASES)
def test_channelizer_ref_is_m_chain_refs(M, D, N):
    rng = np.random.default_rng(100 * M + 10 * D + N)
    taps = rng.uniform(-1, 1, N).astype(np.float32)
    ref = ChannelizerRef(taps, M, D)
    frm = ChannelizerRef(taps, M, D, "frame")
    chains = [ChainRef(taps.astype(np.complex64), D, -2 * math.pi * k / M, 0.0, False, False) for k in range(M)]
    x_max = 0.0
    for n in (7 * D, 12 * D):
        x = rand(rng, n)
        x_max = max(x_max, float(np.max(np.abs(x))))
        got = ref.run(x)
        assert got.shape == (M, out_len(n, D)) == (M, n // D)
        assert np.array_equal(frm.run(x), got.T)
        tol = 1e-10 * float(np.sum(np.abs(taps))) * x_max
        for k in range(M):
            want = chains[k].run(x)[1]
            assert np.max(np.abs(got[k] - want)) <= tol, (M, D, N, n, k, float(np.max(np.abs(got[k] - want))), tol)
    assert ref.phase() == (19 * D) % M
    assert np.array_equal(ref.state(), chains[0].state(N - 1).astype(np.complex64))


def test_channelizer_ref_matches_the_oracle_composition():
    """The reference's three nodes per channel, themselves: f32, so within the chain's bound; the second call is ragged."""
    M, D, N = 8, 3, 21
    rng = np.random.default_rng(11)
    taps = rng.uniform(-1, 1, N).astype(np.float32)
    ref = ChannelizerRef(taps, M, D)
    mixers = [oracle.Mixer(0.0, -2 * math.pi * k / M) for k in range(M)]
    states = [oracle.default_state(taps.astype(np.complex64)) for _ in range(M)]
    for n in (30, 41, 1, 17):
        x = rand(rng, n)
        got = ref.run(x)
        assert got.shape == (M, -(-n // D))
        want = np.stack([oracle.decimate(oracle.batch_fir(mixers[k].mix(x), taps.astype(np.complex64), states[k], norotate=True), D)
                         for k in range(M)])
        check(want, got, ref, (M, D, N, n))
    assert ref.t == 89 and ref.phase() == 89 % M


def test_cuts_at_multiples_of_the_rate_are_neutral_and_state_hooks_restore():
    rng = np.random.default_rng(5)
    for M, D, N in [(8, 3, 21), (4, 4, 13), (12, 5, 25)]:
        taps = rng.uniform(-1, 1, N).astype(np.float32)
        x = rand(rng, 9 * D)
        whole = ChannelizerRef(taps, M, D).run(x)
        cut = ChannelizerRef(taps, M, D)
        a, b = cut.run(x[:2 * D]), cut.run(x[2 * D:])
        assert np.allclose(np.concatenate([a, b], axis=1), whole, rtol=0, atol=1e-12)
        first = ChannelizerRef(taps, M, D)
        first.run(x[:2 * D])
        fresh = ChannelizerRef(taps, M, D)
        fresh.set_state(first.state())
        fresh.set_phase(first.phase() + 5 * M)
        assert np.allclose(fresh.run(x[2 * D:]), b, rtol=0, atol=1e-12)


def stockham_layer(src, M, R, Ns, tw):
    """One layer of channelizer_kernel's transform (chz_layer<R> in csrc/channelizer.hip), index for index."""
    per, tstep = M // R, M // (Ns * R)
    dst = np.zeros(M, np.complex128)
    for j in range(per):
        k = j & (Ns - 1)
        v = [src[j + r * per] * (tw[r * k * tstep] if Ns > 1 else 1.0) for r in range(R)]
        base = (j - k) * R + k
        for m in range(R):
            dst[base + m * Ns] = sum(v[r] * np.exp(2j * np.pi * r * m / R) for r in range(R))
    return dst


@pytest.mark.parametrize("M", [2, 4, 8, 16, 32, 64, 128, 256, 512, 1024])
def test_the_kernels_transform_layers_are_an_inverse_dft(M):
    """The layer sequence the kernel runs -- radix 4 while 4 Ns <= M, then one radix-2 layer -- with its read, twiddle and
    write indices: natural order in, natural order out, the unnormalised inverse DFT; every twiddle index inside the table."""
    rng = np.random.default_rng(M)
    x = rng.standard_normal(M) + 1j * rng.standard_normal(M)
    tw = np.exp(2j * np.pi * np.arange(M) / M)
    s, Ns = x.copy(), 1
    while Ns * 4 <= M:
        s = stockham_layer(s, M, 4, Ns, tw)
        Ns *= 4
    if Ns < M:
        s = stockham_layer(s, M, 2, Ns, tw)
    assert np.max(np.abs(s - np.fft.ifft(x) * M)) <= 1e-12 * M


# ------------------------------------------------------------------ the library without a device
@pytest.fixture(scope="module")
def c():
    import __graft_entry__ as g

    g.build()
    import comms_rs_amd as c

    return c


def test_length_helpers(c):
    from comms_rs_amd import _lib

    lib = _lib.lib()
    m = C.c_size_t(12345)
    for down in (0, 1, 2, 3, 8, 1025, 4096):
        for n in (0, 1, 5, 17, 40, 4097, 20011, 1 << 26):
            assert lib.comms_channelizer_out_len(n, down, C.byref(m)) == 0 and m.value == out_len(n, down), (down, n)
    assert out_len(17, 0) == out_len(17, 1) == 17 and out_len(17, 3) == 6
    for N in (1, 2, 13, 16384):
        assert lib.comms_channelizer_state_len(N, C.byref(m)) == 0 and m.value == state_len(N) == N - 1
    assert lib.comms_channelizer_out_len(6, 3, None) == 1          # NULL out
    assert lib.comms_channelizer_state_len(6, None) == 1
    assert lib.comms_channelizer_state_len(0, C.byref(m)) == 1     # no taps, no state
    assert _lib.CHANNELIZER_CHANNEL_MAJOR == 0 and _lib.CHANNELIZER_FRAME_MAJOR == 1


def test_arguments_are_checked_before_the_device(c):
    from comms_rs_amd import _lib

    lib = _lib.lib()
    t = np.ones(4, np.float32)
    p = t.ctypes.data_as(C.c_void_p)
    h = C.c_void_p()
    assert lib.comms_channelizer_create(p, 0, 4, 2, 0, 0, C.byref(h)) == 1 and not h      # n_taps == 0
    assert lib.comms_channelizer_create(None, 4, 4, 2, 0, 0, C.byref(h)) == 1 and not h   # NULL taps
    assert lib.comms_channelizer_create(p, 4, 0, 2, 0, 0, C.byref(h)) == 1 and not h      # channels == 0
    assert lib.comms_channelizer_create(p, 4, 4, 2, 0, 0, None) == 1                      # NULL out
    for layout in (-1, 2, 8):
        assert lib.comms_channelizer_create(p, 4, 4, 2, layout, 0, C.byref(h)) == 1 and not h
    assert lib.comms_channelizer_create(p, 4, 1025, 2, 0, 0, C.byref(h)) == 1 and not h   # more channels than the series takes
    assert lib.comms_channelizer_create(p, 4, 2048, 2, 1, 0, C.byref(h)) == 1 and not h
    with pytest.raises(c.CommsError) as e:
        c.ChannelizerNode(np.zeros(0, np.float32), 4, 2)
    assert e.value.code == 1
    with pytest.raises(ValueError):
        c.ChannelizerNode(t, 4, 2, layout="rows")
    assert lib.comms_channelizer_destroy(None) == 0
    assert lib.comms_channelizer_set_timer(None, None) == 1
    assert lib.comms_channelizer_run_dev(None, None, 0, None, None) == 1                  # NULL handle
    assert lib.comms_channelizer_run(None, None, 0, None) == 1
    assert lib.comms_channelizer_get_state(None, None, 0) == 1
    assert lib.comms_channelizer_set_state(None, None, 0) == 1
    assert lib.comms_channelizer_get_phase(None, None) == 1
    assert lib.comms_channelizer_set_phase(None, 0) == 1
    assert lib.comms_channelizer_get_kernel(None, 8, None, 0) == 1


def test_channelizer_has_no_cpu_fallback(c):
    if c.device_count() > 0:
        pytest.skip("GPU present")
    for make in (lambda: c.ChannelizerNode(np.ones(64, np.float32), 16, 8),
                 lambda: c.ChannelizerNode(np.ones(64, np.float32), 16, 8, layout="frame"),
                 lambda: c.ChannelizerNode(np.ones(25, np.float32), 12, 5),          # the series forms
                 lambda: c.ChannelizerNode(np.ones(5, np.float32), 1, 2)):
        with pytest.raises(c.CommsError) as e:
            make()
        assert e.value.code == 2
        assert "no CPU fallback" in str(e.value) or "HIP" in str(e.value)
