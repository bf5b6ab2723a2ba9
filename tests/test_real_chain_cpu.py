"""The real FIR + decimator node (comms_rfir_*) where no GPU is needed: host arithmetic and the no-fallback rule."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def c():
    import __graft_entry__ as g

    g.build()
    import comms_rs_amd as c

    return c


def test_rfir_out_len_matches_the_reference_decimator(c, kats):
    """comms_rfir_out_len against the reference's own DecimateNode cases (src/util/resample_node.rs:140-155 and the
    doctest): rates 0 / 1 / 2 / 3 / 100."""
    from comms_rs_amd import _lib

    cases = kats["decimate"]["cases"]
    assert sorted(k["rate"] for k in cases) == [0, 1, 2, 3, 100]
    for k in cases:
        m = C.c_size_t(12345)
        assert _lib.lib().comms_rfir_out_len(len(k["input"]), k["rate"], C.byref(m)) == 0
        assert m.value == len(k["expected"]), k
    assert _lib.lib().comms_rfir_out_len(6, 2, None) == 1  # NULL out_len
    m = C.c_size_t(1)
    assert _lib.lib().comms_rfir_out_len(0, 5, C.byref(m)) == 0 and m.value == 0


def test_real_fir_has_no_cpu_fallback(c):
    if c.device_count() > 0:
        pytest.skip("GPU present")
    for make in (lambda: c.RealFirDecimNode(np.ones(63, np.float32), 5),
                 lambda: c.RealFirDecimNode(np.ones(300, np.float32), 5),                 # the series form
                 lambda: c.RealFirDecimNode(np.ones(4, np.float32), 0, state=np.ones(2, np.float32))):
        with pytest.raises(c.CommsError) as e:
            make()
        assert e.value.code == 2
        assert "no CPU fallback" in str(e.value) or "HIP" in str(e.value)


def test_real_fir_arguments_are_checked_before_the_device(c):
    """n_taps == 0 and an empty user state are COMMS_ERR_ARG (the reference panics) with or without a device"""
    for make in (lambda: c.RealFirDecimNode(np.zeros(0, np.float32), 5),
                 lambda: c.RealFirDecimNode(np.ones(4, np.float32), 5, state=np.zeros(0, np.float32))):
        with pytest.raises(c.CommsError) as e:
            make()
        assert e.value.code == 1
