"""The polyphase stream nodes at every tile plan: symsync_kernel, resample_kernel and channelizer_kernel plan tile, workgroup,
unroll, LDS tier, stride and the place of taps and samples per handle, and tests/plan_cases.py has one format for every plan
(tests/test_plan_cases.py holds that table to the planners, on the CPU).  Every case

  * reads from kernel() that the device chose the plan the port predicts;
  * runs one stream of calls with the state carried -- one output's worth of input, a tile less one, a tile, a tile and one,
    three tiles and five -- against the float64 reference of its node under the project's f32 FIR bound, close() of
    tests/resample_ref.py: 1e-5 sum|taps| max|x|;
  * compares the node's state with the reference's;
  * and holds the plan, bit for bit, to one that the other GPU tests verify: the headers' guarantee that an output's bits depend
    on the taps, the phase count and its own phase only.

Run with -m gpu."""
import re

import numpy as np
import pytest

import plan_cases as pc
import rx_ref
from channelizer_ref import ChannelizerRef
from resample_ref import ResampleRef, close, out_len
from symsync_ref import SymSyncRef

pytestmark = pytest.mark.gpu
CANARY = 0xA5
ROT = (0.37, 1.1)


@pytest.fixture(scope="module")
def c():
    import comms_rs_amd as c

    assert c.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested (no CPU fallback)"
    return c


def rand(rng, n, dtype=np.complex64):
    if np.dtype(dtype).kind == "c":
        return (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(dtype)
    return rng.uniform(-1, 1, n).astype(dtype)


def make_taps(rng, N):
    return rng.uniform(-1, 1, N).astype(np.float32)


def field(name, key):
    return int(re.search(key + r"=(\d+)", name).group(1))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def ident(f):
    return "-".join(str(v) for v in f)


# ------------------------------------------------------------------ symsync
SS_ALL = pc.SYMSYNC_CASES + pc.SYMSYNC_MORE


def ss_node(c, taps, L, S, mu, rot=None):
    node = c.SymbolSyncNode(taps, L, S)
    node.timing = mu / float(L)
    assert node.timing == mu
    if rot:
        node.set_rotation(*rot)
    return node


def ss_chose(node, L, S, N):
    """The device's plan is the port's; the name has no stride: lds = 8 S stride determines it."""
    t = pc.symsync_tile(L, S, N)
    name = node.kernel(S)
    assert name.startswith("symsync_kernel<%d, " % t.plan.U), (name, t)
    assert (field(name, "tile"), field(name, "wg"), field(name, "lds")) == (t.plan.TO, t.plan.WG, t.lds), (name, t)
    assert t.lds == 8 * S * t.stride
    return t


@pytest.mark.parametrize("L,S,N", SS_ALL, ids=[ident(f) for f in SS_ALL])
def test_symsync_at_every_plan(c, L, S, N):
    rng = np.random.default_rng(7000 + 10 * S + N)
    taps = make_taps(rng, N)
    t = ss_chose(c.SymbolSyncNode(taps, L, S), L, S, N)
    xs = [rand(rng, S * k) for k in pc.call_outputs(t.plan.TO)]
    mus = pc.symsync_mus(L, S)
    for mu, rot in [(mu, None) for mu in mus] + [(mus[-1], ROT)]:
        node, ref = ss_node(c, taps, L, S, mu, rot), SymSyncRef(taps, L, S)
        ref.mu = mu
        if rot:
            ref.set_rotation(*rot)
        # the same taps at one sample per symbol and the same row: every sample of the filtered stream, by the largest tile
        # (at S = 1 the twin would be the node's own format: nothing to compare)
        twin = None if rot or S == 1 else ss_node(c, taps, L, 1, mu % L)
        for x in xs:
            got, want = node.run(x), ref.run(x)
            close(got, want, taps, ref.x_max, (L, S, N, mu, rot, x.size))
            if twin is not None:
                full = twin.run(x)
                assert full.shape == (x.size,)
                assert same_bits(got, full[mu // L::S]), (L, S, N, mu, x.size)
            assert np.array_equal(node.state, ref.state()), (L, S, N, mu, x.size)
        if twin is not None:
            assert "tile=1024" in twin.kernel(1) and np.array_equal(twin.state, node.state)


SS_BITS = tuple(f for f in SS_ALL if pc.symsync_tile(*f).plan.TO <= 256)


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("L,S,N", SS_BITS, ids=[ident(f) for f in SS_BITS])
def test_symsync_bits_at_the_small_plans(c, L, S, N, k):
    """The packed decisions of tiles of 256, 128, 64 and 32 outputs -- a word's lanes that are dead because the tile is narrower
    than the workgroup, words that straddle two tiles' outputs at k = 2 -- are the decisions of the same node's Complex<f32>
    output; the tail bits are zero and the bytes behind the output are untouched."""
    rng = np.random.default_rng(7100 + 10 * S + N + k)
    taps = make_taps(rng, N)
    t = ss_chose(c.SymbolSyncNode(taps, L, S), L, S, N)
    assert {1, 31, 32, 33, t.plan.TO - 1, t.plan.TO, t.plan.TO + 1, 3 * t.plan.TO + 5} == set(pc.bits_n_sym(t.plan.TO))
    mu = pc.symsync_mus(L, S)[-1]
    for rot in (None, (0.21, 0.4)):
        a, b = ss_node(c, taps, L, S, mu, rot), ss_node(c, taps, L, S, mu, rot)
        b.set_output(k)
        assert ("bits%d" % k) in b.kernel(S) and field(b.kernel(S), "tile") == t.plan.TO
        for n_sym in pc.bits_n_sym(t.plan.TO):
            x = rand(rng, S * n_sym)
            y = a.run(x)
            nb = (n_sym * k + 7) // 8
            buf = c.DeviceBuf(8 * x.size + nb + 64 + 8)
            buf.upload(x, 0)
            buf.upload(np.full(nb + 64, CANARY, np.uint8), 8 * x.size)
            b.run_dev(buf.ptr, x.size, buf.ptr + 8 * x.size)
            got = buf.download(np.uint8, nb + 64, 8 * x.size)
            assert np.array_equal(got[:nb], rx_ref.sym_to_bits(y, k, None)), (L, S, N, k, rot, n_sym)
            assert (n_sym * k) % 8 == 0 or got[nb - 1] >> ((n_sym * k) % 8) == 0     # tail bits zero
            assert np.all(got[nb:] == CANARY), (L, S, N, k, rot, n_sym)              # the guard bytes
            assert np.array_equal(a.state, b.state) and a.rotation[1] == b.rotation[1]


# ------------------------------------------------------------------ resample
RS_ALL = pc.RESAMPLE_CASES + pc.RESAMPLE_MORE
RS_DTYPE = {"f32": np.float32, "c32": np.complex64}


@pytest.mark.parametrize("L,M,N,dt", RS_ALL, ids=[ident(f) for f in RS_ALL])
def test_resample_at_every_plan(c, L, M, N, dt):
    dtype = RS_DTYPE[dt]
    rng = np.random.default_rng(8000 + 7 * L + 3 * M + N)
    taps = make_taps(rng, N)
    t = pc.resample_tile(L, M, N, dt)
    node, ref, twin = c.ResampleNode(taps, L, M, dtype), ResampleRef(taps, L, M, dtype), c.ResampleNode(taps, L, 1, dtype)
    name = node.kernel(1)
    where = "taps in LDS" if t.plan.tab_lds else "taps in global memory"
    assert name.startswith("resample_kernel<%s, %s>" % (dt, where)), (name, t)
    assert (field(name, "tile"), field(name, "lds")) == (t.plan.TO, t.lds), (name, t)     # (the workgroup follows from the tile)
    assert "resample_kernel" in twin.kernel(1)
    for k in pc.call_outputs(t.plan.TO):
        x = rand(rng, pc.resample_len(k, L, M), dtype)
        got, want = node.run(x), ref.run(x)
        assert got.shape == (out_len(x.size, L, M),) and got.dtype == dtype
        close(got, want, taps, ref.x_max, (L, M, N, dt, x.size))
        # output j is sample j M of the interpolated stream, which the (L, 1) node writes whole
        full = twin.run(x)
        assert full.shape == (x.size * L,)
        assert same_bits(got, full[::M]), (L, M, N, dt, x.size)
        assert np.array_equal(node.get_state(), ref.state()) and np.array_equal(twin.get_state(), ref.state())
    if not t.plan.tab_lds:
        # one phase of thousands of taps: the (L, 1) twin keeps its table in LDS only where the row is short enough.  The f32 node
        # of the same format always does, and a real stream's real parts go through the same multiply-adds in both
        real = c.ResampleNode(taps, L, M, np.float32)
        assert "taps in LDS" in real.kernel(1)
        fresh = c.ResampleNode(taps, L, M, dtype)
        for k in pc.call_outputs(t.plan.TO):
            x = rand(rng, pc.resample_len(k, L, M), np.float32)
            assert same_bits(fresh.run(x.astype(dtype)).real, real.run(x)), (L, M, N, x.size)


# ------------------------------------------------------------------ channelizer
CHZ_ALL = pc.CHANNELIZER_CASES + pc.CHANNELIZER_MORE


def chz_chose(node, M, D, N):
    t = pc.channelizer_tile(M, D, N)
    name = node.kernel(1)
    want = "channelizer_kernel<samples in %s, taps in %s>" % ("LDS" if t.plan.staged else "global memory", "LDS" if t.plan.tab_lds else "global memory")
    assert name.startswith(want), (name, t)
    assert (field(name, "M"), field(name, "frames/tile"), field(name, "lds")) == (M, t.plan.F, t.lds), (name, t)
    return t


@pytest.mark.parametrize("M,D,N", CHZ_ALL, ids=[ident(f) for f in CHZ_ALL])
def test_channelizer_at_every_plan(c, M, D, N):
    rng = np.random.default_rng(9000 + 100 * M + 10 * D + N)
    taps = make_taps(rng, N)
    node, frm, ref = c.ChannelizerNode(taps, M, D), c.ChannelizerNode(taps, M, D, layout="frame"), ChannelizerRef(taps, M, D)
    t = chz_chose(node, M, D, N)
    chz_chose(frm, M, D, N)
    F = t.plan.F
    for k in pc.call_outputs(F):
        x = rand(rng, k * D)
        got, want = node.run(x), ref.run(x)
        assert got.shape == (M, k)
        close(got, want, taps, ref.x_max, (M, D, N, x.size))
        assert same_bits(frm.run(x), got.T), (M, D, N, x.size)                          # the layouts hold the same bits
        assert np.array_equal(node.get_state(), ref.state()) and node.phase == ref.phase()
        assert np.array_equal(frm.get_state(), ref.state()) and frm.phase == ref.phase()
    # the last call again, uncut on a fresh handle and cut at a tile boundary and one frame either side
    k = 3 * F + 5
    x = rand(rng, k * D)
    whole = c.ChannelizerNode(taps, M, D).run(x)
    for cut in sorted({F - 1, F, F + 1, 2 * F} - {0}):
        two = c.ChannelizerNode(taps, M, D)
        got = np.concatenate([two.run(x[:cut * D]), two.run(x[cut * D:])], axis=1)
        assert same_bits(got, whole), (M, D, N, cut)
