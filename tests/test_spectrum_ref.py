"""tests/spectrum_ref.py held to the contract of include/comms_hip.h ("spectrum estimator") without a GPU, and the host side of
the library: the window design and the argument checks of comms_spectrum_create, which come before the device is touched."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spectrum_ref as ref  # noqa: E402


@pytest.fixture(scope="module")
def c():
    import __graft_entry__ as g

    g.build()
    import comms_rs_amd as c

    return c


# ---- the reference -------------------------------------------------------------------------------------------------------------
def test_reference_against_a_direct_dft_matrix():
    n, hop, avg = 64, 24, 3
    x = ref.signal(64 + 8 * hop + 5, 1)
    w = ref.window("hamming", n)
    k = np.arange(n)
    F = np.exp(-2j * np.pi * np.outer(k, k) / n)
    rows = []
    for r in range(3):
        acc = np.zeros(n)
        for s in range(r * avg, r * avg + avg):
            X = F @ (w * x[s * hop: s * hop + n].astype(np.complex128))
            acc += np.abs(X) ** 2
        rows.append(0.25 * acc)
    got = ref.ref_rows(x, w, hop, avg, 0.25)
    assert got.shape == (3, n)
    assert np.max(np.abs(got - np.array(rows))) <= 1e-9 * np.max(got)


@pytest.mark.parametrize("n", ref.SIZES)
def test_parseval(n):
    x = ref.signal(5 * n, 2)
    w = ref.window("hann", n)
    p = ref.segment_powers(x, w, n // 2)
    for s in range(p.shape[0]):
        y = w * x[s * (n // 2): s * (n // 2) + n].astype(np.complex128)
        assert abs(p[s].sum() - n * np.sum(np.abs(y) ** 2)) <= 1e-10 * p[s].sum()


def test_centred_order_is_fftshift():
    n = 128
    x = ref.signal(6 * n, 3)
    w = ref.window("blackman", n)
    nat, cen = ref.ref_rows(x, w, n, 2, 1.0), ref.ref_rows(x, w, n, 2, 1.0, "centred")
    assert np.array_equal(cen, np.fft.fftshift(nat, axes=1))
    c = np.arange(n)
    assert np.array_equal(cen[:, c], nat[:, (c + n // 2) % n])   # column c holds bin (c + N / 2) mod N


def test_out_len_against_enumeration():
    checked = 0
    for n_fft in (64, 128):
        for hop in (1, 7, n_fft // 2, n_fft, n_fft + 5, 3 * n_fft):
            for avg in (1, 2, 3, 32, 33):
                for T in (0, 1, n_fft - 1, n_fft, n_fft + hop - 1, n_fft + hop, 5 * n_fft + 3, 977):
                    for n in (0, 1, 5, n_fft - 1, n_fft, n_fft + 1, hop * avg, hop * avg + n_fft, 4001):
                        assert ref.out_len(T, n, n_fft, hop, avg) == ref.brute_out_len(T, n, n_fft, hop, avg), (n_fft, hop, avg, T, n)
                        checked += 1
    assert checked == 2 * 6 * 5 * 8 * 9
    # calls shorter than N add up to the uncut stream
    n_fft, hop, avg = 64, 24, 2
    assert sum(ref.out_len(T, 50, n_fft, hop, avg) for T in range(0, 1000, 50)) == ref.out_len(0, 1000, n_fft, hop, avg) > 0


def test_case_table():
    cases = ref.cases()
    assert len(cases) == 5 * 4 + 1 and (64, 1) in cases
    assert max(ref.n_samples(n, h, k) for n, h in cases for k in ref.AVGS) < 4e5
    for n, h in cases:
        for k in ref.AVGS:
            ns = ref.n_samples(n, h, k)
            if h == 1:   # (the tail of seven samples is seven segments more)
                assert ref.out_len(0, ns, n, h, k) >= 3
                continue
            assert ref.out_len(0, ns, n, h, k) in (3, 4)
            assert (ns - n) % h != 0                                   # ends inside a segment
            assert k == 1 or ref.segments_before(ns, n, h) % k != 0    # ... and inside a row


# ---- the library's host side ------------------------------------------------------------------------------------------------------
def _ulp_distance(a, b):
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


@pytest.mark.parametrize("kind", ["rect", "hann", "hamming", "blackman"])
def test_window_taps_against_numpy(c, kind):
    for n in (1, 2, 64, 100, 1024):
        got = c.window_taps(kind, n)
        want = ref.window(kind, n).astype(np.float32)
        assert got.dtype == np.float32 and got.shape == (n,)
        near_zero = np.abs(want) < 1e-6   # (blackman's first value is 0 up to the rounding of its coefficients)
        assert np.all(_ulp_distance(got[~near_zero], want[~near_zero]) <= 1), (kind, n)
        assert np.all(np.abs(got[near_zero].astype(np.float64) - ref.window(kind, n)[near_zero]) <= 1e-15), (kind, n)
    if kind == "hann":
        assert c.window_taps(kind, 64)[0] == 0.0 and c.window_taps(kind, 64)[32] == 1.0   # periodic: the peak is at N / 2
    with pytest.raises(c.CommsError) as e:
        c.window_taps(7, 8)
    assert e.value.code == c.COMMS_ERR_ARG


def test_create_argument_errors_come_before_the_device(c):
    from comms_rs_amd._lib import lib

    w = np.ones(2048, np.float32)
    bad = np.ones(64, np.float32)
    bad[17] = np.nan

    def create(n_fft=64, window=w, hop=32, avg=1, scale=1.0, order=0, out=True):
        h = C.c_void_p()
        st = lib().comms_spectrum_create(n_fft, window.ctypes.data_as(C.c_void_p), hop, avg, scale, order, 0, C.byref(h) if out else None)
        assert not h
        return st

    for kw in (dict(n_fft=32), dict(n_fft=96), dict(n_fft=2048), dict(hop=0), dict(avg=0), dict(window=bad), dict(scale=0.0),
               dict(scale=float("inf")), dict(order=2), dict(out=False), dict(hop=(1 << 20) + 1), dict(avg=(1 << 24) + 1),
               dict(scale=float("nan")), dict(scale=-1.0)):
        assert create(**kw) == c.COMMS_ERR_ARG, kw
    n = C.c_size_t()
    assert lib().comms_spectrum_state_len(64, C.byref(n)) == c.COMMS_OK and n.value == 63
    assert lib().comms_spectrum_state_len(96, C.byref(n)) == c.COMMS_ERR_ARG
