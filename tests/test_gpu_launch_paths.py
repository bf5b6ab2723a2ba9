"""The one kernel launch path of the C library (comms::launch_kernel, csrc/common.hpp): LDS opt-in per (kernel, device),
the launch -- with an event pair (hipExtLaunchKernelGGL) or plain -- and the launch check.  Every comparison here is bit
for bit: the same kernel on the same input.  Run with -m gpu.

The chain node reports the kind its last call ran on ("time", "poly": ChainNode.kernel), not the kernel's name: the two
time-domain forms (fir_decim_wave_kernel, fir_decim_kernel) both report "time".  Their batch sizes follow run_decim's rule
(fir_decim.hip): the wave-private form takes a batch whose tiles of 128 outputs spread evenly over the 4096 single-wave
workgroups of the chip (4096 tiles: yes; 4097 tiles: two per wave for one tile more, no) -- the sizes
tests/test_gpu_chain_handover.py uses for the same purpose."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def c():
    import comms_rs_amd

    assert comms_rs_amd.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested (no CPU fallback)"
    return comms_rs_amd


def _same_bits(a, b):
    import torch

    return torch.equal(torch.view_as_real(a).view(torch.int32), torch.view_as_real(b).view(torch.int32))


def _lp(n_taps, cutoff=0.1):
    k = np.arange(n_taps) - (n_taps - 1) / 2
    return (cutoff * np.sinc(cutoff * k) * np.hamming(n_taps)).astype(np.float32).astype(np.complex64)


def _fir(c, n, name):
    def make():
        node = c.BatchFirNode(_lp(255))
        assert node.kernel_for(n) == name, (node.kernel_for(n), name)
        return node

    return make, n, n, lambda node: None


def _chain(c, n_taps, rate, n, kind):
    def make():
        return c.ChainNode(0.2, 0.3, _lp(n_taps, 0.4 / rate), rate, False)

    def after(node):
        assert node.kernel == kind, (node.kernel, kind)

    return make, n, n // rate, after


def _poly8_smallest_n(c):
    """The smallest batch (a multiple of the rate) that the 129-tap rate-8 chain reports on fir_poly8_kernel."""
    import torch

    probe = c.ChainNode(0.2, 0.3, _lp(129, 0.05), 8, False)
    x = torch.zeros(1 << 12, dtype=torch.complex64, device="cuda:0")
    y = torch.empty(1 << 9, dtype=torch.complex64, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    for n in range(8, (1 << 12) + 1, 8):
        probe.run_dev(x.data_ptr(), n, y.data_ptr(), s)
        if probe.kernel == "poly":
            torch.cuda.synchronize()
            return n
    raise AssertionError("the 129-tap rate-8 chain never reported fir_poly8_kernel up to 2^12 samples")


CASES = ["fir_os1024_kernel", "fir_os1024_dyn_kernel", "fir_decim_wave_kernel", "fir_decim_kernel", "fir_poly8_kernel"]


def _case(c, name):
    if name == "fir_os1024_kernel":       # 1366 segments: more than 1024, so 16-wave workgroups, fewer than 4096
        return _fir(c, 1 << 20, name)
    if name == "fir_os1024_dyn_kernel":   # 5462 segments: the ticketed kernel
        return _fir(c, 1 << 22, name)
    if name == "fir_decim_wave_kernel":   # 63 real taps, rate 4: 4096 tiles of 128 outputs
        return _chain(c, 63, 4, 4 * 128 * 4096, "time")
    if name == "fir_decim_kernel":        # ... and 4097 tiles
        return _chain(c, 63, 4, 4 * 128 * 4097, "time")
    return _chain(c, 129, 8, _poly8_smallest_n(c), "poly")


@pytest.mark.parametrize("name", CASES)
def test_timed_and_plain_launches_are_the_same_launch(c, name):
    import torch

    make, n, n_out, after = _case(c, name)
    x = torch.empty(n, dtype=torch.complex64, device="cuda:0")
    c.synth_iq_dev(x.data_ptr(), n, 0, 0xA11CE)
    s = torch.cuda.current_stream().cuda_stream
    plain, timed = make(), make()
    t = c.KernelTimer(4).attach(timed)
    calls = 2  # (the second call reads the history the first one advanced)
    outs = []
    for node in (plain, timed):
        ys = [torch.zeros(n_out, dtype=torch.complex64, device="cuda:0") for _ in range(calls)]
        for y in ys:
            node.run_dev(x.data_ptr(), n, y.data_ptr(), s)
            after(node)
        outs.append(ys)
    torch.cuda.synchronize()
    for a, b in zip(*outs):
        assert _same_bits(a, b), name
    ms = t.read_ms()
    print("%s: n=%d, %s ms" % (name, n, ms))
    assert ms.size == calls, (name, ms)                      # exactly one launch counted per call
    assert np.all(np.isfinite(ms)) and np.all(ms > 0), (name, ms)
    t.close()


def test_no_launch_is_timed_by_accident(c):
    """A timed call on one handle, then a call on a timer-less handle in the same thread: the pair of the first never
    reaches the second's launch."""
    import torch

    n = 4 * 1001
    x = torch.empty(n, dtype=torch.complex64, device="cuda:0")
    c.synth_iq_dev(x.data_ptr(), n, 0, 77)
    s = torch.cuda.current_stream().cuda_stream
    a, b, ref = (c.ChainNode(0.2, 0.3, _lp(63, 0.1), 4, False, kernel="time") for _ in range(3))
    ya, yb, yr = (torch.zeros(n // 4, dtype=torch.complex64, device="cuda:0") for _ in range(3))
    ref.run_dev(x.data_ptr(), n, yr.data_ptr(), s)
    t = c.KernelTimer(4).attach(a)
    a.run_dev(x.data_ptr(), n, ya.data_ptr(), s)
    assert a.kernel == "time"
    assert t.read_ms().size == 1
    b.run_dev(x.data_ptr(), n, yb.data_ptr(), s)
    assert b.kernel == "time"
    torch.cuda.synchronize()
    assert t.read_ms().size == 1
    assert _same_bits(yb, yr)
    assert _same_bits(ya, yr)
    t.close()


_CHILD = r"""
import numpy as np
import comms_rs_amd as c

assert c.device_count() >= 2
n = 1 << 20
k = np.arange(255) - 127.0
taps = (0.1 * np.sinc(0.1 * k) * np.hamming(255)).astype(np.float32).astype(np.complex64)
x = c.synth_iq(n, 5)
out = {}
for dev in (1, 0):  # the second device first: nothing has opted in anywhere yet
    fir = c.BatchFirNode(taps, device=dev)
    assert fir.kernel_for(n) == "fir_os1024_kernel"
    fft = c.FFTBatchNode(16384, False, device=dev)
    out[dev] = (fir.run(x), fft.run(x[:16384]))
for a, b in zip(out[0], out[1]):
    assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
print("devices agree")
"""


def test_lds_opt_in_per_device(c):
    """Both kernels ask for more than 64 KiB of LDS: a device without the opt-in fails the launch.  In a child process,
    so that no kernel has been granted anything on either device before."""
    if c.device_count() < 2:
        pytest.skip("needs two devices")
    out = subprocess.run([sys.executable, "-c", _CHILD], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "devices agree" in out.stdout
