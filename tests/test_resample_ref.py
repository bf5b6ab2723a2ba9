"""CPU check of tests/resample_ref.py, the float64 polyphase reference the GPU resampler tests compare with, against the
oracle's nodes in series -- oracle.decimate(oracle.batch_fir(oracle.upsample(x, L), taps, state), M), with the .real detour
for f32 -- call by call: values within the project's f32 FIR bound, output lengths, and the state mapping
state[L-1::L][:Q] == history newest first, exactly.  Also what of comms_resample_* needs no device: the two length
helpers, the argument checks that come before the device, and the no-CPU-fallback rule."""
import ctypes as C

import numpy as np
import pytest

import oracle
from resample_ref import ResampleRef, close, out_len, state_len, unit

CASES = [(3, 2, 10), (2, 3, 7), (147, 152, 300), (5, 5, 11), (1, 4, 9), (4, 1, 9), (7, 3, 5), (0, 0, 4), (6, 4, 13), (3, 7, 1)]
CALLS = (1, 5, 0, 17, 2, 40)


def rand(rng, n, dtype):
    if np.dtype(dtype).kind == "c":
        return (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(dtype)
    return rng.uniform(-1, 1, n).astype(dtype)


def oracle_call(x, taps, L, M, state):
    """The reference's three nodes on one batch; `state` (complex64, len(taps), newest first) is updated in place."""
    u = oracle.upsample(x, L)
    y = oracle.batch_fir(u.astype(np.complex64), taps.astype(np.complex64), state, norotate=True)
    if x.dtype.kind != "c":
        y = y.real.copy()
    return oracle.decimate(y, M)


@pytest.mark.parametrize("dtype", [np.float32, np.complex64])
@pytest.mark.parametrize("L,M,N", CASES)
def test_resample_ref_matches_the_oracle_composition(L, M, N, dtype):
    rng = np.random.default_rng(100 * L + 10 * M + N)
    taps = rng.uniform(-1, 1, N).astype(np.float32)
    ref = ResampleRef(taps, L, M, dtype)
    Le = max(L, 1)
    Q = state_len(N, L)
    assert ref.Q == Q == (N - 1) // Le
    state = oracle.default_state(taps.astype(np.complex64))
    seen = np.zeros(0, dtype)
    for n in CALLS:
        x = rand(rng, n, dtype)
        want = oracle_call(x, taps, L, M, state)
        got = ref.run(x)
        assert got.shape == want.shape == (out_len(n, L, M),) == (-(-n * Le // max(M, 1)),)
        close(want, got, taps, ref.x_max, (L, M, N, n))
        seen = np.concatenate([seen, x])
        # the history is the last Q inputs, and sits at entries L-1, 2L-1, ... of the reference's state
        hist = ref.state()
        newest_first = np.concatenate([np.zeros(Q, dtype), seen])[::-1][:Q]
        assert np.array_equal(hist, newest_first)
        mapped = state[Le - 1::Le][:Q]
        assert mapped.size == Q
        if np.dtype(dtype).kind == "c":
            assert np.array_equal(mapped, hist)
        else:
            assert np.array_equal(mapped.real, hist) and np.all(mapped.imag == 0)


def test_empty_phases_are_exact_zeros_and_cuts_at_units_are_neutral():
    rng = np.random.default_rng(5)
    taps = rng.uniform(-1, 1, 5).astype(np.float32)
    x = rand(rng, 40, np.float32)
    y = ResampleRef(taps, 7, 3, np.float32).run(x)
    j = np.arange(y.size)
    assert np.all(y[(j * 3) % 7 >= 5] == 0.0) and np.all(y[(j * 3) % 7 < 5] != 0.0)
    for L, M, N in [(147, 152, 300), (6, 4, 13), (2, 3, 7)]:
        taps = rng.uniform(-1, 1, N).astype(np.float32)
        u = unit(L, M)
        x = rand(rng, 9 * u, np.complex64)
        whole = ResampleRef(taps, L, M, np.complex64).run(x)
        cut = ResampleRef(taps, L, M, np.complex64)
        parts = np.concatenate([cut.run(x[:2 * u]), cut.run(x[2 * u:3 * u]), cut.run(x[3 * u:])])
        assert np.array_equal(parts, whole)   # the same products in the same order


def test_state_hooks_of_the_reference():
    rng = np.random.default_rng(6)
    taps = rng.uniform(-1, 1, 13).astype(np.float32)
    x = rand(rng, 60, np.float32)
    one = ResampleRef(taps, 6, 4)
    a, b = one.run(x[:20]), one.run(x[20:])
    first = ResampleRef(taps, 6, 4)
    first.run(x[:20])
    fresh = ResampleRef(taps, 6, 4)
    fresh.set_state(first.state())
    assert np.array_equal(fresh.run(x[20:]), b) and a.size == 30


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
    for L, M, N in CASES + [(147, 152, 3528), (300, 7, 1200), (1, 100, 63)]:
        for n in (0, 1, 5, 17, 40, 4097, 20011, 1 << 26):
            assert lib.comms_resample_out_len(n, L, M, C.byref(m)) == 0 and m.value == out_len(n, L, M), (L, M, n)
        assert lib.comms_resample_state_len(N, L, C.byref(m)) == 0 and m.value == state_len(N, L), (L, N)
    assert lib.comms_resample_out_len(6, 3, 2, None) == 1          # NULL out
    assert lib.comms_resample_state_len(6, 3, None) == 1
    assert lib.comms_resample_state_len(0, 3, C.byref(m)) == 1     # no taps, no state
    assert lib.comms_resample_out_len(1 << 62, 147, 152, C.byref(m)) == 1   # n * up overflows
    assert _lib.RESAMPLE_F32 == 4 and _lib.RESAMPLE_C32 == 8


def test_arguments_are_checked_before_the_device(c):
    from comms_rs_amd import _lib

    lib = _lib.lib()
    t = np.ones(4, np.float32)
    p = t.ctypes.data_as(C.c_void_p)
    h = C.c_void_p()
    assert lib.comms_resample_create(p, 0, 3, 2, 4, 0, C.byref(h)) == 1 and not h      # n_taps == 0
    assert lib.comms_resample_create(None, 4, 3, 2, 4, 0, C.byref(h)) == 1 and not h   # NULL taps
    assert lib.comms_resample_create(p, 4, 3, 2, 4, 0, None) == 1                      # NULL out
    for elem in (0, 1, 2, 5, 16):
        assert lib.comms_resample_create(p, 4, 3, 2, elem, 0, C.byref(h)) == 1 and not h
    with pytest.raises(c.CommsError) as e:
        c.ResampleNode(np.zeros(0, np.float32), 3, 2)
    assert e.value.code == 1
    with pytest.raises(TypeError):
        c.ResampleNode(t, 3, 2, dtype=np.float64)
    assert lib.comms_resample_destroy(None) == 0
    assert lib.comms_resample_set_timer(None, None) == 1
    assert lib.comms_resample_run_dev(None, None, 0, None, None) == 1                  # NULL handle
    assert lib.comms_resample_get_state(None, None, 0) == 1
    assert lib.comms_resample_set_state(None, None, 0) == 1
    assert lib.comms_resample_get_kernel(None, 8, None, 0) == 1


def test_resampler_has_no_cpu_fallback(c):
    if c.device_count() > 0:
        pytest.skip("GPU present")
    for make in (lambda: c.ResampleNode(np.ones(3528, np.float32), 147, 152),
                 lambda: c.ResampleNode(np.ones(64, np.float32), 3, 2, dtype=np.complex64),
                 lambda: c.ResampleNode(np.ones(1200, np.float32), 300, 7)):               # the series form
        with pytest.raises(c.CommsError) as e:
            make()
        assert e.value.code == 2
        assert "no CPU fallback" in str(e.value) or "HIP" in str(e.value)
