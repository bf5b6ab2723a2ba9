"""GPU tests of the Complex<f32> synchronisation estimators (comms_syncest_*, syncest_kernel; comms_*_phase_estimate_c32,
phase_c32_kernel) against the oracle on the widened input.  Inputs, references and tolerances come from tests/syncest_ref.py;
tests/test_syncest_ref.py measures on the CPU what the timing tolerance rests on.  Run with -m gpu."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
import rx_ref
import symsync_ref
import syncest_ref as sr
from test_estimators import freq_stream, psk_stream, qam16_stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def c():
    import comms_rs_amd as c

    assert c.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested (no CPU fallback)"
    return c


def kernel_of(node, n):
    name = node.kernel(n)
    assert name.startswith("syncest_kernel"), name
    return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", name)}


def bits_equal(a, b):
    f = lambda e: np.array([e.timing, e.freq, e.timing_sum.real, e.timing_sum.imag, e.freq_sum.real, e.freq_sum.imag]).view(np.uint64)
    return np.array_equal(f(a), f(b))


def check(got, idx, what):
    """One estimate against case idx's reference: the sums relative to the sums of |terms|, then the angles."""
    name, n, d, alpha, x = sr.cases()[idx]
    ref = sr.reference(idx)
    what = (what, name, n, d, alpha, x.size)
    dfs = abs(got.freq_sum - ref["fs"])
    print("%s: timing %+.6f (oracle %+.6f), freq %+.6f (oracle %+.6f)" % (what, got.timing, ref["timing"], got.freq, ref["freq"]))
    assert dfs <= sr.FREQ_SUM_TOL * ref["fa"], (what, dfs, ref["fa"])
    assert abs(got.freq - ref["freq"]) <= sr.ANGLE_TOL, (what, got.freq, ref["freq"])
    assert abs(got.freq - np.arctan2(got.freq_sum.imag, got.freq_sum.real)) <= 1e-15
    if x.size < 2:
        assert got.freq_sum == 0 and got.freq == 0.0
    if ref["ta"] == 0.0:                       # len <= n d, or alpha = 0
        assert got.timing_sum == 0 and got.timing == 0.0, (what, got)
        return
    dts = abs(got.timing_sum - ref["ts"]) / ref["ta"]
    dt = sr.circ(got.timing, ref["timing"], n)
    print("    timing sum off by %.3e of sum|terms| (tolerance %.3e), estimate by %.3e samples (tolerance %.3e)"
          % (dts, sr.TIMING_SUM_TOL, dt, sr.TIMING_TOL))
    assert dts <= sr.TIMING_SUM_TOL, (what, dts)
    assert dt <= sr.TIMING_TOL, (what, got.timing, ref["timing"], dt)
    assert sr.circ(got.timing, sr.timing_of(got.timing_sum, n), n) <= 1e-12


# ------------------------------------------------------------------ 1. every case against the oracle
@pytest.mark.parametrize("n,d", sr.ND)
def test_lengths_grid(c, n, d):
    node = c.SyncEstimatorNode(n, d, 0.25)
    k = kernel_of(node, sr.TILE)
    assert k["tile"] == sr.TILE and k["tiles"] == 1 and k["taps"] >= 2 * n * d + 1 and k["max_grid"] <= sr.GRID_CAP
    for idx, (name, cn, cd, alpha, x) in enumerate(sr.cases()):
        if (cn, cd) != (n, d) or not name.startswith("len"):
            continue
        got = node.run(x)
        check(got, idx, "grid")
        assert bits_equal(got, node.run(x))                         # fresh filter state on every call, reproducible
        if x.size:
            buf = c.DeviceBuf(8 * x.size).upload(x)                 # the input ends where its allocation ends
            assert bits_equal(got, node.run_dev(buf.ptr, x.size))   # host-pointer run == run_dev, bit for bit
        else:
            assert bits_equal(got, node.run_dev(0, 0))


def test_alpha(c):
    for idx, (name, n, d, alpha, x) in enumerate(sr.cases()):
        if name.startswith("alpha"):
            check(c.SyncEstimatorNode(n, d, alpha).run(x), idx, "alpha")


def test_more_tiles_than_the_persistent_grid(c):
    idx = [i for i, cs in enumerate(sr.cases()) if cs[0] == "past-the-grid"][0]
    _, n, d, alpha, x = sr.cases()[idx]
    node = c.SyncEstimatorNode(n, d, alpha)
    k = kernel_of(node, x.size)
    assert k["tiles"] > k["grid"] == k["max_grid"]                           # workgroups walk several tiles
    buf = c.DeviceBuf(8 * x.size).upload(x)
    got = node.run_dev(buf.ptr, x.size)
    check(got, idx, "grid cap")
    assert bits_equal(got, node.run_dev(buf.ptr, x.size))
    assert bits_equal(got, node.run(x))                                      # device scratch route of the host entry
    # a short call afterwards reads back only its own partials
    small = [i for i, cs in enumerate(sr.cases()) if cs[0] == "len%d" % (sr.TILE + 1) and cs[1:3] == (n, d)][0]
    check(node.run(sr.cases()[small][4]), small, "short after long")


def test_input_pointer_aligned_to_one_sample_only(c):
    idx = [i for i, cs in enumerate(sr.cases()) if cs[0] == "offset-pointer"][0]
    _, n, d, alpha, x = sr.cases()[idx]
    assert x.size == sr.TILE + 1
    node = c.SyncEstimatorNode(n, d, alpha)
    buf = c.DeviceBuf(8 * (x.size + 1))
    assert buf.ptr % 16 == 0
    buf.upload(np.concatenate([np.full(1, 1e6 + 1e6j, np.complex64), x]))    # the sample in front must not be read
    got = node.run_dev(buf.ptr + 8, x.size)
    check(got, idx, "offset")
    assert bits_equal(got, node.run(x))


def test_impulses_at_the_tile_edges(c):
    seen = 0
    for idx, (name, n, d, alpha, x) in enumerate(sr.cases()):
        if name.startswith("impulse"):
            check(c.SyncEstimatorNode(n, d, alpha).run(x), idx, "impulse")
            seen += 1
    assert seen == 4


def test_arguments(c):
    from comms_rs_amd import _lib

    lib = _lib.lib()
    h = C.c_void_p()
    for n, d, alpha in ((8, 64, 0.25), (257, 1, 0.25), (4, 4, 1.5), (0, 1, 0.25), (4, 0, 0.25)):
        assert lib.comms_syncest_create(n, d, alpha, 0, C.byref(h)) == c.COMMS_ERR_ARG and not h
    with pytest.raises(c.CommsError):
        c.SyncEstimatorNode(4, 4, 1.5)
    node = c.SyncEstimatorNode(8, 63, 0.25)                                   # 1009 taps: accepted
    timer = c.KernelTimer(4).attach(node)
    buf = c.DeviceBuf(4096)
    out = (C.c_double * 6)()
    assert lib.comms_syncest_run_dev(node._h, buf.ptr + 4, 8, out, None) == c.COMMS_ERR_ARG   # half a sample off
    assert lib.comms_syncest_run_dev(node._h, None, 8, out, None) == c.COMMS_ERR_ARG
    assert lib.comms_syncest_run_dev(node._h, buf.ptr, 8, None, None) == c.COMMS_ERR_ARG
    assert timer.read_ms().size == 0
    node.run(sr.signal(8, 4096))
    ms = timer.read_ms()
    assert ms.size == 1 and 0 < ms[0] < 100
    timer.close()


def test_frequency_on_the_reference_test_signal(c):
    x = freq_stream(np.random.default_rng(0), 0.123456789).astype(np.complex64)
    got = c.SyncEstimatorNode(4, 4, 0.25).run(x).freq
    assert abs(got - oracle.frequency_offset_estimate(x.astype(np.complex128))) <= sr.ANGLE_TOL
    assert abs(0.123456789 - got) < 0.01                                      # frequency_estimator.rs's own bound


# ------------------------------------------------------------------ 2. phase entries
PH_T = 8 * 256 * 256                     # phase_c32_kernel's grid cap times its 256 lanes
PH_N = (0, 1, 255, 256, 257, 3 * PH_T + 2)   # the last: past the grid cap AND into the four-accumulator loop


@functools.lru_cache(maxsize=None)
def phase_input(kind, m):
    rng = np.random.default_rng(300 + m)
    x = psk_stream(rng, m, max(PH_N), 0.123456) if kind == "psk" else qam16_stream(rng, max(PH_N), 0.123456)
    return x.astype(np.complex64)


@pytest.mark.parametrize("kind,m", [("psk", 1), ("psk", 2), ("psk", 4), ("psk", 8), ("qam", 4)])
def test_phase_entries(c, kind, m):
    x = phase_input(kind, m)
    buf = c.DeviceBuf(8 * x.size).upload(x)
    for n in PH_N + (257, 1):                                                  # short calls after the long one
        xs = x[:n]
        X = xs.astype(np.complex128)
        if kind == "psk":
            want, host, dev = oracle.psk_phase_estimate(X, m), c.psk_phase_estimate_c32(xs, m), c.psk_phase_estimate_c32_dev(buf.ptr, n, m)
        else:
            want, host, dev = oracle.qam_phase_estimate(X), c.qam_phase_estimate_c32(xs), c.qam_phase_estimate_c32_dev(buf.ptr, n)
        assert host == dev, (kind, m, n, host, dev)
        assert abs(host - want) <= sr.ANGLE_TOL, (kind, m, n, host, want)
        if n == 0:
            assert host == 0.0
        if n == max(PH_N):
            assert abs(host - 0.123456) < (1e-6 if kind == "psk" else 0.01)     # phase_estimator.rs's own bounds
    if kind == "psk":
        assert c.psk_phase_estimate_c32_dev(buf.ptr + 8, 257, m) == c.psk_phase_estimate_c32(x[1:258], m)   # 8-byte aligned only
        with pytest.raises(c.CommsError):
            c.psk_phase_estimate_c32(x[:4], 0)
        out = C.c_double()
        assert c.lib().comms_psk_phase_estimate_c32_dev(buf.ptr + 4, 16, m, C.byref(out), 0, None) == c.COMMS_ERR_ARG


# ------------------------------------------------------------------ 3. the loop it exists for
@pytest.mark.parametrize("dd", sr.LOOP_DD)
def test_the_loop_on_the_device(c, dd):
    """SyncEstimatorNode -> tau -> SymbolSyncNode symbols -> psk_phase_estimate_c32(m = 4) -> set_rotation -> bits: one of the
    four quarter-turn hypotheses has zero bit errors (tests/test_syncest_ref.py: so has the reference recipe alone)."""
    L, S = sr.LOOP_L, sr.LOOP_S
    v, x, h = sr.loop_signal(dd)
    est = c.SyncEstimatorNode(S, sr.LOOP_D, sr.LOOP_BETA).run(x)
    want = oracle.timing_push(x.astype(np.complex128), S, sr.LOOP_D, sr.LOOP_BETA)
    assert abs(est.freq) < 0.05                       # no offset was applied (the estimate's bias on shaped PSK remains)
    tau = symsync_ref.tau_from_estimate(est.timing, h.size, L, S)
    node = c.SymbolSyncNode(h, L, S)
    node.timing = tau
    assert node.timing == symsync_ref.mu_of(symsync_ref.tau_from_estimate(want, h.size, L, S), L, S)
    y = node.run(x)
    ph = c.psk_phase_estimate_c32(y, 4)
    assert abs(ph - oracle.psk_phase_estimate(y.astype(np.complex128), 4)) <= sr.ANGLE_TOL
    errs = []
    for rot in sr.loop_rotations(ph):
        rx = c.SymbolSyncNode(h, L, S).set_output(2)
        rx.timing = tau
        rx.set_rotation(0.0, rot)
        got = rx_ref.unpack_values(rx.run(x), x.size // S, 2)
        n_err, n_bits = sr.loop_bit_errors(got, v, h, c.bit_errors)
        errs.append(n_err)
    print("dd=%d: estimate %+.4f samples (oracle %+.4f), phase %+.4f, bit errors of the four quarter turns %s of %d"
          % (dd, est.timing, want, ph, errs, n_bits))
    assert n_bits > 3500 and min(errs) == 0


# ------------------------------------------------------------------ 4. host graph
def test_host_graph_nodes(c):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "comms_rs_amd", "host"), "-s"], timeout=600)
    out = subprocess.run([os.path.join(ROOT, "comms_rs_amd", "lib", "test_syncest_nodes_gpu")], capture_output=True,
                         text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all passed" in out.stdout
