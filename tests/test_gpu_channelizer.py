"""ChannelizerNode (comms_channelizer_*): M chains mixer -> FIR -> decimator over one Complex<f32> stream -- one launch
(channelizer_kernel) or, beyond its range, M launches of the chain node -- against tests/channelizer_ref.py, the float64
filter bank that tests/test_channelizer_ref.py pins to M ChainRefs and to the oracle's composition.  Bound: the chain's,
chain_ref.out_bound = 2e-5 sum|h| max|x| per output, every output from the first."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from chain_ref import ChainRef, check_outputs, out_bound
from channelizer_ref import ChannelizerRef, check, out_len

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAG_LIB = os.path.join(ROOT, "comms_rs_amd", "lib", "libcomms_hip_diag.so")  # build()'s diagnostic build: the only one with kernel selectors

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def c():
    import comms_rs_amd as c

    assert c.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested (no CPU fallback)"
    return c


def rand(rng, n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def make_taps(rng, n_taps):
    return rng.uniform(-1, 1, n_taps).astype(np.float32)


def field(name, key):
    return int(re.search(key + r"=(\d+)", name).group(1))


def run_dev(c, node, x):
    """The device entry on device buffers (legacy stream), downloaded."""
    n, shape = x.size, node.shape(x.size)
    m = shape[0] * shape[1]
    din, dout = c.DeviceBuf(max(8 * n, 8)).upload(x), c.DeviceBuf(max(8 * m, 8))
    node.run_dev(din.ptr, n, dout.ptr)
    return dout.download(np.complex64, m).reshape(shape)


# ------------------------------------------------------------------ 1. parity, one launch
def grid_of(M):
    rates = sorted({M, max(M // 2, 1), 3, M + 1})
    taps = sorted({1, max(M - 1, 1), M + 1, 4 * M + 3} | ({16 * M} if M in (2, 64) else set()))
    grid = [(D, N) for D in rates for N in taps]
    if M == 1024:   # this kernel's own corner: spans that do not fit in LDS are read from global memory (from nine taps per branch)
        grid += [(1024, 16384), (3, 8195), (1025, 9300), (4096, 16384)]
    return grid


@pytest.mark.parametrize("M", [2, 4, 8, 16, 64, 256, 1024])
def test_parity_one_launch(c, M):
    """Per case: two full tiles, one frame and a remainder that is not a multiple of D; both layouts, which hold the same
    bits."""
    seen = set()
    for D, N in grid_of(M):
        rng = np.random.default_rng(1000 * M + 10 * D + N)
        taps = make_taps(rng, N)
        node = c.ChannelizerNode(taps, M, D)
        F = field(node.kernel(1), "frames/tile")
        n = (2 * F + 1) * D + (D // 2 if D > 1 else 0) + (1 if D > 2 else 0)
        assert D == 1 or n % D != 0
        name = node.kernel(n)
        assert name.startswith("channelizer_kernel<") and "series" not in name, (M, D, N, name)
        assert field(name, "tiles") == -(-out_len(n, D) // F) >= 3
        seen.add(name.split(">")[0])
        x = rand(rng, n)
        got = node.run(x)
        ref = ChannelizerRef(taps, M, D)
        want = ref.run(x)
        assert got.shape == (M, out_len(n, D)) and got.dtype == np.complex64
        check(got, want, ref, (M, D, N, n))
        frm = c.ChannelizerNode(taps, M, D, layout="frame")
        assert "channelizer_kernel" in frm.kernel(n)
        assert np.array_equal(frm.run(x), got.T), (M, D, N)
    if M == 1024:   # both sources of the samples and both places of the taps have been through the grid
        assert seen == {"channelizer_kernel<samples in LDS, taps in LDS", "channelizer_kernel<samples in LDS, taps in global memory",
                        "channelizer_kernel<samples in global memory, taps in global memory"}, seen
    else:
        assert seen == {"channelizer_kernel<samples in LDS, taps in LDS"}, seen


@pytest.mark.parametrize("N,samples,taps", [(14 * 512, "LDS", "global memory"), (15 * 512, "global memory", "global memory"),
                                            (16 * 512, "global memory", "global memory"), (8 * 512, "LDS", "LDS"),
                                            (9 * 512, "LDS", "global memory")])
def test_planner_boundaries_at_512_channels(c, N, samples, taps):
    """M = 512 sits on both of the planner's limits: one frame's span of 15 x 512 samples beside a 513-sample frame buffer is
    (513 + 7680) 8 = 65544 bytes, eight more than the 64 KiB a workgroup asks for, so from fifteen taps per branch the samples
    stay in global memory; the tap table leaves LDS above 16 KiB, from nine taps per branch."""
    M, D = 512, 512
    rng = np.random.default_rng(512 + N)
    h = make_taps(rng, N)
    node = c.ChannelizerNode(h, M, D)
    F = field(node.kernel(1), "frames/tile")
    n = (2 * F + 25) * D + 7        # past the first tiles, which reach into the history
    name = node.kernel(n)
    assert name.startswith("channelizer_kernel<samples in %s, taps in %s>" % (samples, taps)), name
    assert field(name, "lds") <= 64 * 1024
    x = rand(rng, n)
    got = node.run(x)
    ref = ChannelizerRef(h, M, D)
    check(got, ref.run(x), ref, (M, D, N, n))
    assert np.array_equal(c.ChannelizerNode(h, M, D, layout="frame").run(x), got.T)


# ------------------------------------------------------------------ 2. the convention, without the helper
@pytest.mark.parametrize("k0", [0, 1, 9, 15])
def test_a_tone_lands_in_its_channel(c, k0):
    M = N = D = 16
    taps = (np.ones(M) / M).astype(np.float32)
    n = 40 * D
    t = np.arange(n, dtype=np.float64)
    x = np.exp(2j * np.pi * k0 * t / M).astype(np.complex64)
    node = c.ChannelizerNode(taps, M, D)
    assert "channelizer_kernel" in node.kernel(n)
    got = node.run(x).astype(np.complex128)
    b = out_bound(taps, 1.0)
    want = np.zeros((M, 40))
    want[k0] = 1.0
    assert np.max(np.abs(got[:, 1:] - want[:, 1:])) <= b, (k0, float(np.max(np.abs(got[:, 1:] - want[:, 1:]))), b)


# ------------------------------------------------------------------ 3. state
STATE_CASES = [(8, 3, 35), (64, 32, 200), (16, 17, 16), (12, 5, 25), (4, 17, 9)]   # the last two: the series


@pytest.mark.parametrize("M,D,N", STATE_CASES)
def test_state_across_ragged_calls(c, M, D, N):
    rng = np.random.default_rng(3000 + M + N)
    taps = make_taps(rng, N)
    node = c.ChannelizerNode(taps, M, D)
    ref = ChannelizerRef(taps, M, D)
    assert node.state_len() == N - 1
    seen = np.zeros(N - 1, np.complex64)
    for n in (1, N - 3, 0, 4 * D + 1, 1001, 7 * D + D // 2 + 1):
        x = rand(rng, n)
        got = node.run(x)
        check(got, ref.run(x), ref, (M, D, N, n))
        seen = np.concatenate([seen, x])[-(N - 1):]
        assert node.phase == ref.phase()
    assert np.array_equal(node.get_state(), seen[::-1])   # the last N - 1 inputs, newest first
    assert np.array_equal(node.get_state(2), seen[::-1][:2])


@pytest.mark.parametrize("layout", ["channel", "frame"])
@pytest.mark.parametrize("M,D,N", [(8, 3, 35), (64, 32, 1024), (1024, 512, 4099), (1024, 512, 9300), (256, 257, 255), (2, 1, 32)])
def test_cut_invariance_bit_for_bit(c, M, D, N, layout):
    rng = np.random.default_rng(4000 + M + N)
    taps = make_taps(rng, N)
    node = c.ChannelizerNode(taps, M, D, layout=layout)
    F = field(node.kernel(1), "frames/tile")
    units = 5 * F + 3
    x = rand(rng, units * D)
    assert "channelizer_kernel" in node.kernel(x.size)
    whole = node.run(x)
    axis = 1 if layout == "channel" else 0
    many = sorted(set(int(v) for v in rng.integers(1, units, 12)))
    for cuts in ([units // 2], [1, units - 1], many):
        node = c.ChannelizerNode(taps, M, D, layout=layout)
        edges = [0] + [k * D for k in cuts] + [x.size]
        got = np.concatenate([node.run(x[a:b]) for a, b in zip(edges[:-1], edges[1:])], axis=axis)
        assert np.array_equal(got, whole), (M, D, N, cuts[:4])


@pytest.mark.parametrize("M,D,N", [(8, 3, 35), (64, 32, 200), (1024, 3, 1025), (1024, 3, 9300)])
def test_checkpoint_and_shard_hooks(c, M, D, N):
    rng = np.random.default_rng(5000 + M + N)
    taps = make_taps(rng, N)
    j0 = 37                                # the second shard's first frame: s = j0 D is no multiple of M
    s = j0 * D
    assert s % M != 0
    x = rand(rng, s + 50 * D + 1)
    whole = c.ChannelizerNode(taps, M, D).run(x)
    # checkpoint: state and phase of a node that ran the first part, into a fresh handle
    first = c.ChannelizerNode(taps, M, D)
    a = first.run(x[:s])
    saved, t = first.get_state(), first.phase
    halo = np.concatenate([np.zeros(N - 1, np.complex64), x[:s]])[::-1][:N - 1]
    assert np.array_equal(saved, halo) and t == s % M
    fresh = c.ChannelizerNode(taps, M, D)
    fresh.state = saved
    fresh.phase = t
    assert np.array_equal(fresh.get_state(), saved) and fresh.phase == t
    b = fresh.run(x[s:])
    assert np.array_equal(np.concatenate([a, b], axis=1), whole)
    # shard: the halo in front and the stream index itself (reduced by the node)
    shard = c.ChannelizerNode(taps, M, D)
    shard.set_state(halo)
    shard.set_phase(s)
    assert shard.phase == s % M
    assert np.array_equal(shard.run(x[s:]), whole[:, j0:])


# ------------------------------------------------------------------ 4. host entry == device entry
@pytest.mark.parametrize("M,D,N,n,layout", [(8, 3, 35, 10000, "channel"), (64, 64, 256, 1 << 16, "frame"), (64, 32, 256, 1 << 21, "channel"),
                                             (12, 5, 25, 10000, "channel")])
def test_host_entry_equals_device_entry(c, M, D, N, n, layout):
    """Short calls run on zero-copy staging, longer ones through device scratch (2^21 samples: 16 MiB in, 32 MiB out)."""
    rng = np.random.default_rng(6000 + M)
    taps = make_taps(rng, N)
    x = rand(rng, n)
    host = c.ChannelizerNode(taps, M, D, layout=layout).run(x)
    dev = run_dev(c, c.ChannelizerNode(taps, M, D, layout=layout), x)
    assert host.shape == dev.shape and np.array_equal(host, dev)


# ------------------------------------------------------------------ 5. beyond the kernel's range: the series
# M = 1, M not a power of two, one filter past N = 16 M, one rate past D = 4 M
@pytest.mark.parametrize("layout", ["channel", "frame"])
@pytest.mark.parametrize("M,D,N", [(1, 2, 5), (12, 5, 25), (4, 4, 65), (4, 17, 9)])
def test_series_beyond_the_kernels_range(c, M, D, N, layout):
    rng = np.random.default_rng(2000 + M + N)
    taps = make_taps(rng, N)
    node = c.ChannelizerNode(taps, M, D, layout=layout)
    ref = ChannelizerRef(taps, M, D, layout)
    for n in (4097, 20 * D, 1001):
        x = rand(rng, n)
        name = node.kernel(n)
        assert "series" in name and "channelizer_kernel" not in name, name
        got = node.run(x)
        assert got.shape == ((M, out_len(n, D)) if layout == "channel" else (out_len(n, D), M))
        check(got, ref.run(x), ref, (M, D, N, n))
    # the documented limits themselves are the kernel's
    for m, d, nt in ((4, 4, 64), (4, 16, 9), (2, 8, 32), (1024, 4096, 16384)):
        assert "channelizer_kernel" in c.ChannelizerNode(make_taps(rng, nt), m, d).kernel(100), (m, d, nt)
    with pytest.raises(c.CommsError) as e:   # more channels than the series takes
        c.ChannelizerNode(taps, 1025, 3)
    assert e.value.code == 1


def test_forced_series_agrees_with_the_kernel():
    """The diagnostic build's COMMS_CHANNELIZER_SERIES runs an in-range handle as its series: the same handle, state and
    phase carried across the switch, within twice the bound of the kernel's outputs."""
    code = r'''
import os, sys
sys.path.insert(0, %r)
sys.path.insert(0, os.path.join(%r, "tests"))
import numpy as np
import comms_rs_amd as c
from chain_ref import out_bound
rng = np.random.default_rng(9)
M, D, N = 16, 8, 70
taps = rng.uniform(-1, 1, N).astype(np.float32)
x = (rng.standard_normal(3 * 4000 + 5) + 1j * rng.standard_normal(3 * 4000 + 5)).astype(np.complex64)
plain = c.ChannelizerNode(taps, M, D)
want = [plain.run(x[a:a + 4000]) for a in (0, 4000, 8000)]
node = c.ChannelizerNode(taps, M, D)
got = []
for i, a in enumerate((0, 4000, 8000)):
    if i == 1:
        os.environ["COMMS_CHANNELIZER_SERIES"] = "1"
    else:
        os.environ.pop("COMMS_CHANNELIZER_SERIES", None)
    assert ("series" in node.kernel(4000)) == (i == 1), node.kernel(4000)
    got.append(node.run(x[a:a + 4000]))
b = 2 * out_bound(taps, float(np.max(np.abs(x))))
assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
d = float(np.max(np.abs(got[1].astype(np.complex128) - want[1])))
assert 0 < d <= b, (d, b)
print("ok", d, b)
''' % (ROOT, ROOT)
    assert os.path.exists(DIAG_LIB), "the diagnostic build is part of build(): %s" % DIAG_LIB
    env = dict(os.environ, COMMS_HIP_LIB=DIAG_LIB)
    env.pop("COMMS_CHANNELIZER_SERIES", None)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ok" in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------ 6. past the grid
def test_more_tiles_than_twice_the_grid(c):
    """M = 1024 at D = 3 with two taps per branch: a tile is two frames, six samples, so 2 grid + 1 tiles are under 10 000
    samples and every workgroup walks three tiles.  An impulse comb plus noise, every output checked."""
    M, D, N = 1024, 3, 1025
    rng = np.random.default_rng(77)
    taps = make_taps(rng, N)
    node = c.ChannelizerNode(taps, M, D, layout="frame")
    name = node.kernel(1)
    F, max_grid = field(name, "frames/tile"), field(name, "max_grid")
    tiles = 2 * max_grid + 1
    n = tiles * F * D
    assert n <= 1 << 16
    name = node.kernel(n)
    assert "channelizer_kernel" in name and field(name, "tiles") == tiles and field(name, "grid") <= max_grid
    x = (0.01 * rand(rng, n)).astype(np.complex64)
    x[::97] += 1.0
    got = node.run(x)
    ref = ChannelizerRef(taps, M, D, "frame")
    check(got, ref.run(x), ref, "past the grid")


# ------------------------------------------------------------------ 7. into the existing nodes
@pytest.mark.parametrize("k", [0, 3])
def test_a_channel_feeds_the_fm_demodulator(c, k):
    """Channel k of a channel-major call is a contiguous device stream: comms_fmdemod_run_dev takes it where it lies.  Against
    the chain node with dphase = -2 pi k / M, the same taps, rate and FM demod, on the same input; both within the chain's FM
    bound of the f64 chain."""
    M, D, N = 8, 4, 64
    rng = np.random.default_rng(700 + k)
    idx = np.arange(N) - (N - 1) / 2.0
    taps = (np.sinc(idx / M) / M * np.hamming(N)).astype(np.float32)
    n = 1 << 14
    t = np.arange(n, dtype=np.float64)
    x = (np.exp(1j * (2 * np.pi * k * t / M + 3.0 * np.cos(2 * np.pi * t / 512))) + 0.01 * rand(rng, n)).astype(np.complex64)
    frames = n // D
    node = c.ChannelizerNode(taps, M, D)
    assert "channelizer_kernel" in node.kernel(n)
    din, dmid, dfm = c.DeviceBuf(8 * n).upload(x), c.DeviceBuf(8 * M * frames), c.DeviceBuf(4 * frames)
    node.run_dev(din.ptr, n, dmid.ptr)
    c.FMDemodNode().run_dev(dmid.ptr + 8 * k * frames, frames, dfm.ptr)
    got = dfm.download(np.float32, frames)
    chain = c.ChainNode(-2 * math.pi * k / M, 0.0, taps.astype(np.complex64), D, True).run(x)
    ref = ChainRef(taps.astype(np.complex64), D, -2 * math.pi * k / M, 0.0, True, False)
    want, y = ref.run(x)
    x_max = float(np.max(np.abs(x)))
    check_outputs(got, want, y, 0j, taps, x_max, True, "channel %d -> FM demod" % k)
    check_outputs(chain, want, y, 0j, taps, x_max, True, "chain %d" % k)


# ------------------------------------------------------------------ 8. arguments
def test_arguments(c):
    import ctypes as C

    from comms_rs_amd import _lib

    lib = _lib.lib()
    t = np.ones(4, np.float32)
    h = C.c_void_p()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.comms_channelizer_create(p(t), 0, 4, 2, 0, 0, C.byref(h)) == 1 and not h          # n_taps == 0
    assert lib.comms_channelizer_create(None, 4, 4, 2, 0, 0, C.byref(h)) == 1 and not h          # NULL taps
    assert lib.comms_channelizer_create(p(t), 4, 0, 2, 0, 0, C.byref(h)) == 1 and not h          # no channel
    assert lib.comms_channelizer_create(p(t), 4, 4, 2, 2, 0, C.byref(h)) == 1 and not h          # unknown layout
    assert lib.comms_channelizer_create(p(t), 4, 4, 2, 0, 0, None) == 1                         # NULL out
    rng = np.random.default_rng(7)
    for M, D, N in ((8, 3, 35), (12, 5, 25)):
        node = c.ChannelizerNode(make_taps(rng, N), M, D)
        H = node.state_len()
        assert H == N - 1
        node.set_state(rand(rng, H))
        node.set_phase(5)
        before = node.get_state()
        assert node.run(np.zeros(0, np.complex64)).shape == (M, 0)                               # n == 0: OK, nothing written
        assert lib.comms_channelizer_run_dev(node._h, None, 0, None, None) == 0
        assert lib.comms_channelizer_run(node._h, None, 0, None) == 0
        assert np.array_equal(node.get_state(), before) and node.phase == 5                      #   ... and the state stays
        assert lib.comms_channelizer_run_dev(node._h, None, 8, None, None) == 1                  # NULL device pointers
        assert lib.comms_channelizer_run(node._h, None, 8, None) == 1
        assert lib.comms_channelizer_get_state(node._h, None, 1) == 1
        assert lib.comms_channelizer_get_state(node._h, p(before), H + 1) == 1                   # more than the state
        assert lib.comms_channelizer_set_state(node._h, p(before), H - 1) == 1                   # not exactly the state
        assert lib.comms_channelizer_set_state(node._h, p(before), H + 1) == 1
        assert lib.comms_channelizer_get_phase(node._h, None) == 1
        assert lib.comms_channelizer_get_kernel(node._h, 8, None, 0) == 1
        buf = c.DeviceBuf(1024)
        assert lib.comms_channelizer_run_dev(node._h, buf.ptr, 8, buf.ptr, None) == 1            # in place
        assert lib.comms_channelizer_run_dev(node._h, buf.ptr, 8, buf.ptr + 32, None) == 1       # overlapping
        assert lib.comms_channelizer_run_dev(node._h, buf.ptr + 4, 2, buf.ptr + 512, None) == 1  # misaligned
        assert lib.comms_channelizer_run_dev(node._h, buf.ptr, 1 << 62, buf.ptr + 512, None) == 1   # frames * M overflows
        assert np.array_equal(node.get_state(), before) and node.phase == 5                      # refused calls change nothing
        node.set_phase(3 * M + 2)
        assert node.phase == 2
    assert lib.comms_channelizer_destroy(None) == 0
    assert lib.comms_channelizer_set_timer(None, None) == 1


# ------------------------------------------------------------------ 9. timer
@pytest.mark.parametrize("M,D,N", [(64, 32, 256), (12, 5, 25)])
def test_kernel_timer_brackets_the_launch(c, M, D, N):
    rng = np.random.default_rng(8)
    x = rand(rng, 1 << 14)
    node = c.ChannelizerNode(make_taps(rng, N), M, D)
    timer = c.KernelTimer(8).attach(node)
    for _ in range(3):
        node.run(x)
    ms = timer.read_ms()
    assert ms.size == 3 and np.all(ms > 0) and np.all(ms < 100)
    node.set_timer(None)
    node.run(x)
    assert timer.read_ms().size == 3
    timer.close()


# ------------------------------------------------------------------ 10. the C++ graph
def test_cpp_channelizer_nodes_graph(tmp_path):
    """Source -> ChannelizerNode -> M sinks in a Graph (and ChannelizerNodeDev on device messages), against values this
    helper writes."""
    M, D, N = 8, 3, 35
    rng = np.random.default_rng(10)
    taps = make_taps(rng, N)
    ref = ChannelizerRef(taps, M, D)
    msgs = [rand(rng, n) for n in (1000, 7, 4096)]
    want = [ref.run(x) for x in msgs]
    path = str(tmp_path / "channelizer_case.bin")
    with open(path, "wb") as f:
        np.array([M, D, N, len(msgs)], np.uint64).tofile(f)
        taps.tofile(f)
        np.array([ref.bound()], np.float64).tofile(f)
        for x, w in zip(msgs, want):
            np.array([x.size, w.shape[1]], np.uint64).tofile(f)
            x.tofile(f)
            w.astype(np.complex128).tofile(f)
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "comms_rs_amd", "host"), "-s"], timeout=600)
    out = subprocess.run([os.path.join(ROOT, "comms_rs_amd", "lib", "test_channelizer_nodes_gpu"), path], capture_output=True,
                         text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all passed" in out.stdout
