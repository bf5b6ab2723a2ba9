"""GPU tests of the symbol synchroniser (comms_symsync_*, symsync_kernel) against tests/symsync_ref.py, the float64
reference that tests/test_symsync_ref.py pins to the oracle's composition on the CPU.  Run with -m gpu."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
import rx_ref
import symsync_ref as sr
from resample_ref import close
from symsync_ref import SymSyncRef
from test_symsync_ref import count_errors, half_symbol_margin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
CASES = [(1, 4, 33), (32, 4, 1025), (32, 2, 513), (7, 3, 50), (8, 1, 64), (16, 4, 5), (256, 4, 4096), (1, 1, 1), (4, 256, 4096)]
CANARY = 0xA5


@pytest.fixture(scope="module")
def c():
    import comms_rs_amd as c

    assert c.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested (no CPU fallback)"
    return c


def rand_c(rng, n):
    return (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(np.complex64)


def make_taps(rng, N):
    return rng.uniform(-1, 1, N).astype(np.float32)


def mus(L, S):
    return sorted({0, 1 % (S * L), L - 1, L % (S * L), S * L - 1})


def tile_of(node, n):
    name = node.kernel(n)
    assert "symsync_kernel" in name, name
    return int(re.search(r"tile=(\d+)", name).group(1)), int(re.search(r"max_grid=(\d+)", name).group(1))


def pair(c, taps, L, S, mu=0, rot=None):
    node, ref = c.SymbolSyncNode(taps, L, S), SymSyncRef(taps, L, S)
    node.timing = mu / float(max(L, 1))
    ref.mu = mu
    assert node.timing == mu
    if rot:
        node.set_rotation(*rot)
        ref.set_rotation(*rot)
    return node, ref


def bits_equal(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


# ------------------------------------------------------------------ 1. parity grid
@pytest.mark.parametrize("L,S,N", CASES)
def test_parity_grid(c, L, S, N):
    rng = np.random.default_rng(100 * L + 10 * S + N)
    taps = make_taps(rng, N)
    TO, _ = tile_of(c.SymbolSyncNode(taps, L, S), S)
    lens = [S, S * (TO - 1), S * TO, S * (TO + 1), S * 4099]
    xs = [rand_c(rng, n) for n in lens]
    for mu in mus(L, S):
        for rot in (None, (0.37, 1.1)) if mu in (0, S * L - 1) else (None,):
            node, ref = pair(c, taps, L, S, mu, rot)
            for x in xs:           # the calls of one stream: the state carries
                assert "symsync_kernel" in node.kernel(x.size)
                got = node.run(x)
                want = ref.run(x)
                close(got, want, taps, ref.x_max, (L, S, N, mu, rot, x.size))
                if mu % L >= N:    # a phase without a tap
                    assert np.all(got == 0.0)
            assert np.array_equal(node.state, ref.state())


# ------------------------------------------------------------------ 2. last sample
def test_last_sample_reaches_the_last_output_and_nothing_beyond_is_read(c):
    L, S, N = 32, 4, 1025
    taps = make_taps(np.random.default_rng(2), N)
    node = c.SymbolSyncNode(taps, L, S)
    node.timing = (S * L - 1) / L
    for n in (S, S * 1000):
        x = np.zeros(n, np.complex64)
        x[-1] = 3.0 - 2.0j
        buf = c.DeviceBuf(8 * n + 8 * (n // S))           # the input ends where its allocation ends
        out_off = 0
        in_off = 8 * (n // S)
        buf.upload(x, in_off)
        node.state = np.zeros(node.state_len(), np.complex64)
        node.run_dev(buf.ptr + in_off, n, buf.ptr + out_off)
        y = buf.download(np.complex64, n // S, out_off)
        assert y[-1] == np.complex64(taps[L - 1]) * x[-1] and np.all(y[:-1] == 0)


# ------------------------------------------------------------------ 3. past the grid cap
def test_more_tiles_than_the_persistent_grid(c):
    L, S, N = 4, 256, 4096                               # the smallest tile and the fewest resident workgroups
    rng = np.random.default_rng(3)
    taps = make_taps(rng, N)
    node, ref = pair(c, taps, L, S, 5)
    TO, cap = tile_of(node, S)
    n_out = (2 * cap + 1) * TO - 3                        # every workgroup walks two tiles, one walks three; the last is partial
    name = node.kernel(S * n_out)
    assert int(re.search(r"tiles=(\d+)", name).group(1)) == 2 * cap + 1 and int(re.search(r"grid=(\d+)", name).group(1)) == cap
    x = rand_c(rng, S * n_out)
    close(node.run(x), ref.run(x), taps, ref.x_max, "grid cap")


# ------------------------------------------------------------------ 4. streaming
@pytest.mark.parametrize("L,S,N", [(32, 4, 1025), (7, 3, 50), (4, 8, 4096)])
@pytest.mark.parametrize("rot", [None, (2 * np.pi * 0.0371, 0.3)])
def test_cut_stream_equals_the_uncut_stream_bit_for_bit(c, L, S, N, rot):
    rng = np.random.default_rng(4)
    taps = make_taps(rng, N)
    x = rand_c(rng, S * 20011)
    whole, _ = pair(c, taps, L, S, L + 3, rot)
    want = whole.run(x)
    Q = whole.state_len()
    for cut in (1, 7, -(-Q // S), 4099):
        node, _ = pair(c, taps, L, S, L + 3, rot)
        a, b = node.run(x[:S * cut]), node.run(x[S * cut:])
        assert bits_equal(np.concatenate([a, b]), want), (L, S, N, rot, cut)   # with any dphase: the rotor is closed-form
        assert np.array_equal(node.state, whole.state) and node.rotation[1] == whole.rotation[1]
    # checkpoint: state + phase + timing into a fresh handle
    first, _ = pair(c, taps, L, S, L + 3, rot)
    first.run(x[:S * 4099])
    fresh = c.SymbolSyncNode(taps, L, S)
    fresh.state = first.state
    fresh.set_rotation(first.rotation[0], first.rotation[1])
    fresh.timing = first.timing / L
    assert bits_equal(fresh.run(x[S * 4099:]), want[4099:])
    # n < Q: the history is only partly replaced
    if Q > S:
        node, ref = pair(c, taps, L, S, 1)
        for n in (S, S, S * 3, S):
            xs = rand_c(rng, n)
            close(node.run(xs), ref.run(xs), taps, 1.5, "short calls")
            assert np.array_equal(node.state, ref.state())


# ------------------------------------------------------------------ 5. timing change between calls
def test_timing_changes_between_calls_leave_the_history_alone(c):
    L, S, N = 32, 4, 1025
    rng = np.random.default_rng(5)
    taps = make_taps(rng, N)
    node, ref = pair(c, taps, L, S)
    for mu in (0, L + 3, S * L - 1):
        node.timing = mu / L
        ref.mu = mu
        assert node.timing == mu
        x = rand_c(rng, S * 777)
        close(node.run(x), ref.run(x), taps, ref.x_max, mu)
        assert np.array_equal(node.state, ref.state())
    for tau, mu in ((0.37, 12), (-0.02, 127), (4.0, 0), (1e6 + 0.5, 16)):
        node.timing = tau
        assert node.timing == mu == sr.mu_of(tau, L, S)


# ------------------------------------------------------------------ 6. bits
@pytest.mark.parametrize("k", [1, 2])
def test_bits_are_the_decisions_of_the_c32_output(c, k):
    L, S, N = 32, 4, 1025
    rng = np.random.default_rng(6 + k)
    taps = make_taps(rng, N)
    tables = [None] + [t for kk, t in rx_ref.TABLES.values() if kk == k]
    for table in tables:
        for rot in (None, (0.21, 0.4)):
            a, _ = pair(c, taps, L, S, 37, rot)
            b, _ = pair(c, taps, L, S, 37, rot)
            b.set_output(k, table)
            for n_sym in (1, 7, 8, 9, 31, 32, 33, 4099):
                x = rand_c(rng, S * n_sym)
                y = a.run(x)
                nb = (n_sym * k + 7) // 8
                buf = c.DeviceBuf(8 * x.size + nb + 64 + 8)
                buf.upload(x, 0)
                buf.upload(np.full(nb + 64, CANARY, np.uint8), 8 * x.size)
                b.run_dev(buf.ptr, x.size, buf.ptr + 8 * x.size)
                got = buf.download(np.uint8, nb + 64, 8 * x.size)
                want = rx_ref.sym_to_bits(y, k, table)
                assert np.array_equal(got[:nb], want), (k, n_sym)
                assert (n_sym * k) % 8 == 0 or got[nb - 1] >> ((n_sym * k) % 8) == 0     # tail bits zero
                assert np.all(got[nb:] == CANARY)                                        # the guard bytes
                assert np.array_equal(a.state, b.state) and a.rotation[1] == b.rotation[1]
    # switching the format between calls leaves state and phase as they were
    a, _ = pair(c, taps, L, S, 5, (0.1, 0.0))
    b, _ = pair(c, taps, L, S, 5, (0.1, 0.0))
    for i, fmt in enumerate((k, None, k, k, None)):
        x = rand_c(rng, S * (501 + i))
        y = a.run(x)
        b.set_output(fmt)
        got = b.run(x)
        assert np.array_equal(got, rx_ref.sym_to_bits(y, k)) if fmt else bits_equal(got, y)


# ------------------------------------------------------------------ 7. arguments
def test_arguments(c):
    from comms_rs_amd import _lib

    lib = _lib.lib()
    rng = np.random.default_rng(7)
    L, S, N = 32, 4, 1025
    taps = make_taps(rng, N)
    node = c.SymbolSyncNode(taps, L, S)
    timer = c.KernelTimer(8).attach(node)
    node.state = rand_c(rng, node.state_len())
    before = node.state
    buf = c.DeviceBuf(4096)
    p = taps.ctypes.data_as(C.c_void_p)
    h = C.c_void_p()
    assert lib.comms_symsync_run_dev(node._h, buf.ptr, S + 1, buf.ptr + 2048, None) == 1          # n % S != 0
    assert lib.comms_symsync_set_timing(node._h, float("nan")) == 1 and lib.comms_symsync_set_timing(node._h, float("inf")) == 1
    assert lib.comms_symsync_create(p, N, 257, S, 0, C.byref(h)) == 1 and not h                   # L > 256
    assert lib.comms_symsync_create(p, N, 1, S, 0, C.byref(h)) == 1 and not h                     # ceil(N / L) > 1024
    assert timer.read_ms().size == 0 and np.array_equal(node.state, before) and node.timing == 0  # no launch
    assert lib.comms_symsync_create(None, N, L, S, 0, C.byref(h)) == 1 and not h                  # NULL taps
    assert lib.comms_symsync_set_output_format(node._h, _lib.SYM_BITS, 3, None) == 1              # bits_per_sym = 3
    assert lib.comms_symsync_set_output_format(node._h, 7, 1, None) == 1
    assert lib.comms_symsync_run_dev(node._h, buf.ptr, 8, buf.ptr, None) == 1                     # in place
    assert lib.comms_symsync_run_dev(node._h, buf.ptr + 4, 8, buf.ptr + 2048, None) == 1          # misaligned input
    assert lib.comms_symsync_run_dev(node._h, buf.ptr, 8, buf.ptr + 2052, None) == 1              # misaligned c32 output
    assert lib.comms_symsync_run_dev(node._h, None, 8, None, None) == 1
    node.set_output(1)
    assert lib.comms_symsync_run_dev(node._h, buf.ptr, 8, buf.ptr + 2049, None) == 1              # misaligned bits output
    assert lib.comms_symsync_run_dev(node._h, buf.ptr, 8, buf.ptr + 2052, None) == 0              # 4-byte aligned is enough
    node.set_output(None)
    assert timer.read_ms().size == 1
    before = node.state
    assert node.run(np.zeros(0, np.complex64)).shape == (0,)                                      # n == 0: OK, nothing changes
    assert lib.comms_symsync_run_dev(node._h, None, 0, None, None) == 0
    assert np.array_equal(node.state, before) and timer.read_ms().size == 1
    assert lib.comms_symsync_set_state(node._h, before.ctypes.data_as(C.c_void_p), before.size - 1) == 1
    assert lib.comms_symsync_get_state(node._h, before.ctypes.data_as(C.c_void_p), before.size + 1) == 1
    assert lib.comms_symsync_set_rotation(node._h, float("nan"), 0.0) == 1
    timer.close()


def test_host_entry_equals_device_entry(c):
    L, S, N = 32, 4, 1025
    rng = np.random.default_rng(8)
    taps = make_taps(rng, N)
    for n in (S * 9, S * 3001, S * ((1 << 20) + 5)):           # pinned staging, past the zero-copy limit, device scratch
        for k in (None, 2):
            hst, _ = pair(c, taps, L, S, 70, (0.05, 0.0))
            dev, _ = pair(c, taps, L, S, 70, (0.05, 0.0))
            hst.set_output(k)
            dev.set_output(k)
            x = rand_c(rng, n)
            nb = dev.out_bytes(n)
            buf = c.DeviceBuf(8 * n + nb + 8).upload(x)
            dev.run_dev(buf.ptr, n, buf.ptr + 8 * n)
            assert np.array_equal(hst.run(x).view(np.uint8), buf.download(np.uint8, nb, 8 * n))


# ------------------------------------------------------------------ 8. end to end, no noise
@pytest.mark.parametrize("dd", [0, 5, 16, 27])
def test_end_to_end_timing_recovery_without_noise(c, dd):
    L, S, NP, beta, n_sym = 32, 4, 33, 0.35, 4096
    bits = c.PrnsNode(0xB8, 0xFF, 8).run_batch(2 * n_sym, packed=True)
    v = rx_ref.unpack_values(bits, n_sym, 2)
    sym16 = c.qpsk_bit_mod(v.astype(np.uint8))
    sym = (sym16[:, 0] + 1j * sym16[:, 1]).astype(np.complex64)
    assert np.array_equal(sym, rx_ref.QPSK_DEF[v])
    # the transmit pulse at S samples per symbol is every L-th tap of the pulse at L S: dd = 0 is the PulseNode's stream
    x = sr.fractional_delay(sym, NP, S, L, beta, dd, oracle.rrc_taps, oracle.pulse)
    if dd == 0:
        tx = c.PulseNode(c.rrc_taps(NP, float(S), beta), S).run(sym)[: x.size]
        assert np.max(np.abs(tx - x)) <= 1e-5 * np.sum(np.abs(c.rrc_taps(NP, float(S), beta))) * np.sqrt(2)
    N = (NP - 1) * L + 1
    h = oracle.rrc_taps(N, float(L * S), beta, np.complex128).real.astype(np.float32)
    e = c.TimingEstimatorNode(S, 8, beta).run(x.astype(np.complex128))
    tau = sr.tau_from_estimate(e, N, L, S)
    x32 = x.astype(np.complex64)

    def y_of_mu(mu):
        ref = SymSyncRef(h, L, S)
        ref.mu = mu
        return ref.run_c(x32)

    def node_errors(got, n_sym_out):
        """comms_bit_errors between the node's packed bits and the transmitted ones, transients dropped, at the best whole-
        symbol lag of -2 .. 2 around the filters' delay (the alignment of count_errors)."""
        skip = NP
        delay = int(round(((NP - 1) / 2.0 + (N - 1) / (2.0 * L)) / S))
        k = np.arange(skip, n_sym_out - skip)
        mine = rx_ref.pack(rx_ref.unpack_values(got, n_sym_out, 2)[k], 2)
        return min(c.bit_errors(mine, rx_ref.pack(v[k - delay - lag], 2), 2 * k.size) for lag in range(-2, 3)), 2 * k.size

    for off, what in ((0.0, "on time"), (S / 2.0, "half a symbol off")):
        node = c.SymbolSyncNode(h, L, S).set_output(2)
        node.timing = tau + off
        mu = node.timing
        assert mu == sr.mu_of(tau + off, L, S)
        got = node.run(x32)
        errs, n_bits = node_errors(got, x.size // S)
        want_errs, flippable, _ = count_errors(y_of_mu(mu), v, NP, h, x)       # the reference alone, first
        print("dd=%d %s: mu=%d, %d of %d bits wrong (reference %d, %d within the f32 bound of a decision line)"
              % (dd, what, mu, errs, n_bits, want_errs, flippable))
        if off == 0.0:
            assert want_errs == 0 and errs == 0
        else:
            margin = half_symbol_margin(y_of_mu, mu, v, NP, h, x)   # derived from the CPU sweep's accuracy: see there
            print("dd=%d: margin %d" % (dd, margin))
            assert margin > 0 and errs >= margin


# ------------------------------------------------------------------ 9. host graph
def test_host_graph_nodes(c):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "comms_rs_amd", "host"), "-s"], timeout=600)
    out = subprocess.run([os.path.join(ROOT, "comms_rs_amd", "lib", "test_symsync_nodes_gpu")], capture_output=True,
                         text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all passed" in out.stdout


def test_kernel_timer_brackets_the_launch(c):
    rng = np.random.default_rng(9)
    node = c.SymbolSyncNode(make_taps(rng, 1025), 32, 4)
    timer = c.KernelTimer(8).attach(node)
    x = rand_c(rng, 1 << 14)
    for _ in range(3):
        node.run(x)
    ms = timer.read_ms()
    assert ms.size == 3 and np.all(ms > 0) and np.all(ms < 100)
    node.set_timer(None)
    node.run(x)
    assert timer.read_ms().size == 3
    timer.close()
