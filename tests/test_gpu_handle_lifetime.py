"""Every handle of the C library owns its device memory through owner types (DevBuf, Scratch, Pinned, History:
csrc/common.hpp) and is ended by one path (destroy_handle: select the device, drain the stream it followed last, delete).
What that path has to keep, whatever the node:

  * a handle that still FOLLOWS a pooled stream its owner has handed back can be destroyed without any getter in between,
    and leaves no follower behind: comms_stream_pool_trim succeeds afterwards and the library works on;
  * a create that fails after its handle exists leaves nothing behind either (same error every time, the pool trims);
  * create / destroy cycles of handles with large allocations give all their device memory back.

Shapes: the smallest legal configuration of every node; a block of 4104 samples (a multiple of every rate used here, and
more than one tile of every tiled kernel: the largest is 2048) for the stateful nodes, one transform for the FFTs."""
import ctypes as C
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 4104
BUF_BYTES = 1 << 20  # every call below reads and writes less


@pytest.fixture(scope="module")
def c():
    import comms_rs_amd as c

    assert c.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested (no CPU fallback)"
    return c


@pytest.fixture(scope="module")
def bufs():
    """Zeroed device input and (separate) output; zeros are valid samples of every format."""
    import torch

    x = torch.zeros(BUF_BYTES, dtype=torch.uint8, device="cuda:0")
    y = torch.zeros(BUF_BYTES, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    return x.data_ptr(), y.data_ptr(), (x, y)


def _detection(c):
    from comms_rs_amd import nodes

    return np.zeros(0, nodes.FRAME_DETECTION_DTYPE)


# name -> (make(c), run(c, node, x, y, stream)): one tiny block through the node's device entry
KINDS = {
    "fir": (lambda c: c.BatchFirNode([1, 0.5]), lambda c, h, x, y, s: h.run_dev(x, N, y, s)),
    "pulse": (lambda c: c.PulseNode([1, 0.5, 0.25], 2), lambda c, h, x, y, s: h.run_dev(x, N, y, s)),
    "fir_i16": (lambda c: c.BatchFirNodeI16([[1, 0], [2, 0]]), lambda c, h, x, y, s: h.run_dev(x, N, y, s)),
    "pulse_i16": (lambda c: c.PulseNodeI16([[1, 0], [2, 0]], 2), lambda c, h, x, y, s: h.run_dev(x, N, y, s)),
    "fir_f64": (lambda c: c.BatchFirNodeF64([1, 0.5]), lambda c, h, x, y, s: h.run_dev(x, N, y, s)),
    "pulse_f64": (lambda c: c.PulseNodeF64([1, 0.5], 2), lambda c, h, x, y, s: h.run_dev(x, N, y, s)),
    "mixer": (lambda c: c.MixerNode(0.1), lambda c, h, x, y, s: h.run_dev(x, N, y, s)),
    "fmdemod": (lambda c: c.FMDemodNode(), lambda c, h, x, y, s: h.run_dev(x, N, y, s)),
    "fmdemod_f64": (lambda c: c.FMDemodNodeF64(), lambda c, h, x, y, s: h.run_dev(x, N, y, s)),
    "fft": (lambda c: c.FFTBatchNode(8, False), lambda c, h, x, y, s: h.run_dev(x, N, y, s)),
    "fft_bluestein": (lambda c: c.FFTBatchNode(513, False), lambda c, h, x, y, s: h.run_dev(x, N, y, s)),
    "fft_f64": (lambda c: c.FFTBatchNodeF64(8, False), lambda c, h, x, y, s: h.run_dev(x, N, y, s)),
    "fft_f64_bluestein": (lambda c: c.FFTBatchNodeF64(4617, False), lambda c, h, x, y, s: h.run_dev(x, 4617, y, s)),
    "chain_fused": (lambda c: c.ChainNode(0.1, 0.0, [1, 0.5], 8, False), lambda c, h, x, y, s: h.run_dev(x, N, y, s)),
    "chain_fm": (lambda c: c.ChainNode(0.1, 0.0, [1, 0.5], 8, True), lambda c, h, x, y, s: h.run_dev(x, N, y, s)),
    "chain_series": (lambda c: c.ChainNode(0.1, 0.0, [1, 0.5], 8, True, unfused=True), lambda c, h, x, y, s: h.run_dev(x, N, y, s)),
    "rfir": (lambda c: c.RealFirDecimNode([1, 0.5], 2), lambda c, h, x, y, s: h.run_dev(x, N, y, s)),
    "rfir_series": (lambda c: c.RealFirDecimNode(np.ones(258), 2), lambda c, h, x, y, s: h.run_dev(x, N, y, s)),
    "resample": (lambda c: c.ResampleNode([1, 0.5, 0.25], 2, 3), lambda c, h, x, y, s: h.run_dev(x, N, y, s)),
    "resample_series": (lambda c: c.ResampleNode([1, 0.5, 0.25], 257, 2), lambda c, h, x, y, s: h.run_dev(x, 8, y, s)),
    "channelizer": (lambda c: c.ChannelizerNode([1, 0.5, 0.25], 2, 2), lambda c, h, x, y, s: h.run_dev(x, N, y, s)),
    "channelizer_series": (lambda c: c.ChannelizerNode([1, 0.5, 0.25], 3, 3), lambda c, h, x, y, s: h.run_dev(x, N, y, s)),
    "symsync": (lambda c: c.SymbolSyncNode([1, 0.5, 0.25, 0.125], 2, 2), lambda c, h, x, y, s: h.run_dev(x, N, y, s)),
    "prns": (lambda c: c.PrnsNode(0xB8, 1), lambda c, h, x, y, s: h.run_dev(N, y, packed=True, stream=s)),
    "noise": (lambda c: c.NoiseSource(1), lambda c, h, x, y, s: h.bits_dev(N, y, packed=True, stream=s)),
    "timing": (lambda c: c.TimingEstimatorNode(2, 2, 0.25), lambda c, h, x, y, s: h.run_dev(x, N, s)),
    "syncest": (lambda c: c.SyncEstimatorNode(2, 2, 0.25), lambda c, h, x, y, s: h.run_dev(x, N, s)),
    "framesync": (lambda c: c.FrameSyncNode([1, -1, 1, 1], 0.5, 1), lambda c, h, x, y, s: h.run_dev(x, N, stream=s)),
    "deframe": (lambda c: c.DeframeNode(8, 0, 4), lambda c, h, x, y, s: h.run_dev(x, N, _detection(c), y, 0, stream=s)),
    "nco": (lambda c: c.NcoNode(0.1), lambda c, h, x, y, s: h.run_dev(x, N, y, s)),
}


def _fir_check(c):
    """One BatchFirNode run on fixed samples (a fresh node each time: the same bits whenever the library works)."""
    return c.BatchFirNode([0.5, 0.25 - 0.5j, 0.125]).run(c.synth_iq(4096, 0, 3))


def _trim(c):
    from comms_rs_amd._lib import check, lib

    gc.collect()  # (buffers and handles that earlier tests dropped without closing them)
    check(lib().comms_stream_pool_trim(0))


@pytest.fixture(scope="module")
def before(c):
    return _fir_check(c)


@pytest.mark.parametrize("kind", list(KINDS))
def test_destroy_while_following_a_released_pooled_stream(c, bufs, before, kind):
    """The handle runs one block on a stream from comms_stream_create, the stream goes back to the pool, and the handle
    is destroyed with no getter in between: the destroy itself drains the (still existing) stream and detaches."""
    import torch
    from comms_rs_amd._lib import check, lib

    x, y, _ = bufs
    make, run = KINDS[kind]
    node = make(c)
    sp = C.c_void_p()
    check(lib().comms_stream_create(0, C.byref(sp)))
    run(c, node, x, y, sp.value)
    check(lib().comms_stream_destroy(0, sp))
    node.close()
    torch.cuda.synchronize()


def test_pool_trims_and_library_works_after_the_destroys(c, bufs, before):
    """After every kind has been through the test above no handle follows a pooled stream: the pool trims, and a fresh
    node computes what it computed before."""
    x, y, _ = bufs
    from comms_rs_amd._lib import check, lib

    for kind, (make, run) in KINDS.items():  # (once more, all of them before ONE trim: the test above may run a subset)
        node = make(c)
        sp = C.c_void_p()
        check(lib().comms_stream_create(0, C.byref(sp)))
        run(c, node, x, y, sp.value)
        check(lib().comms_stream_destroy(0, sp))
        node.close()
    _trim(c)
    np.testing.assert_array_equal(_fir_check(c).view(np.uint8), before.view(np.uint8))


# Creates that fail AFTER their handle exists, on a healthy device (found by reading csrc/): the FFT plans are built on
# the new handle and reject these lengths; the chain makes its FIR node on the new chain handle, and that rejects 0 taps.
def _failing_creates(c):
    from comms_rs_amd._lib import lib

    taps = np.ones(2, np.complex64)
    vp = taps.ctypes.data_as(C.c_void_p)

    def call(f, *args):
        h = C.c_void_p()
        st = f(*args, 0, C.byref(h))
        assert not h.value, "a failed create must leave *out NULL"
        return st

    return {
        "fft_bluestein_too_long": lambda: call(lib().comms_fft_create, 3 << 22, 0),
        "fft_pow2_too_long": lambda: call(lib().comms_fft_create, 1 << 25, 0),
        "fft_f64_bluestein_too_long": lambda: call(lib().comms_fft_f64_create, 3 << 22, 0),
        "fft_f64_pow2_too_long": lambda: call(lib().comms_fft_f64_create, 1 << 25, 0),
        "chain_without_taps": lambda: call(lib().comms_chain_create_ex, 0.1, 0.0, vp, 0, 8, 0),
    }


def test_failing_creates_leave_nothing_behind(c, before):
    for name, create in _failing_creates(c).items():
        codes = {create() for _ in range(64)}
        assert codes == {c.COMMS_ERR_ARG}, (name, codes)
    _trim(c)
    np.testing.assert_array_equal(_fir_check(c).view(np.uint8), before.view(np.uint8))


def _free_bytes():
    import torch

    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


@pytest.mark.parametrize("cls,n,elem", [("FFTBatchNode", 3 << 20, 8), ("FFTBatchNodeF64", 3 << 19, 16)])
def test_no_device_memory_is_lost_over_create_destroy_cycles(c, cls, n, elem):
    """Bluestein transforms: chirp, spectrum, the plan's tables and two work buffers of the padded length -- several
    allocations of tens of MiB per handle.  Free memory after 16 more cycles is within ONE footprint of free memory after
    the warm-up cycle (a buffer leaked per cycle would exceed that several times over); the footprint is measured, and
    must be at least 64 MiB for the test to mean anything.  (Measured: 254 MiB each; 3.4 s and 7.1 s, most of it the
    seventeen plans' tables computed on the host.)"""
    import torch
    from comms_rs_amd._lib import lib

    x = torch.zeros(n * elem, dtype=torch.uint8, device="cuda:0")
    y = torch.zeros(n * elem, dtype=torch.uint8, device="cuda:0")
    lib().comms_buf_pool_trim(0)

    def cycle():
        node = getattr(c, cls)(n, False)
        node.run_dev(x.data_ptr(), n, y.data_ptr(), 0)
        used = _free_bytes()
        node.close()
        return used

    free0 = _free_bytes()
    footprint = free0 - cycle()
    after_warmup = _free_bytes()
    print("footprint %d MiB, free before %d, after warm-up %d" % (footprint >> 20, free0, after_warmup))
    assert footprint >= 64 << 20, footprint
    for _ in range(16):
        cycle()
    after = _free_bytes()
    print("free after 16 cycles %d (lost %d)" % (after, after_warmup - after))
    assert after_warmup - after < footprint, (after_warmup, after, footprint)
