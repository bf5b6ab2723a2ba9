"""The channel-state output of OfdmDemodNode (ofdm_demod_kernel<N, true>) and the weighted soft demapper (demap_*_kernel with
weights) on an MI355X against tests/csi_ref.py.  Cases, weights, bounds and the link's noise are csi_ref's
(tests/test_csi_ref.py holds them to their rules); no bound here comes from a kernel's output.  The checks themselves are
tests/csi_children.py's, which also runs them on capped grids.  Every figure is printed before it is asserted."""
import os
import subprocess
import sys

import numpy as np
import pytest

import csi_children as ch
import csi_ref as cr
import ofdm_ref as r
import symmap_ref as sr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAG_LIB = os.path.join(ROOT, "comms_rs_amd", "lib", "libcomms_hip_diag.so")


@pytest.fixture(scope="module")
def c():
    import comms_rs_amd as c

    assert c.device_count() >= 1
    return c


@pytest.mark.parametrize("n_frames", r.FRAME_COUNTS)
@pytest.mark.parametrize("kind,name,cpe", cr.csi_cases())
def test_csi_against_the_definition(c, kind, name, cpe, n_frames):
    ch.check_csi(c, kind, name, cpe, n_frames)


def test_csi_with_several_blocks_per_frame(c):
    """n512_cp36 with one frame: two blocks of symbols, both form 1 / H_k, the one that starts at symbol 0 writes the record."""
    k = ch.check_csi(c, "channel", "n512_cp36", False, 1)
    assert k["blocks"] >= 2 and k["items"] == k["blocks"], k


def test_zero_training_gives_zero_csi_in_its_frame_only(c):
    f, rx = r.degenerate_case("zero_training")
    args, kw = f.node_args()
    dem = c.OfdmDemodNode(*args, **kw)
    rec, g = dem.run(rx, csi=True)
    bad = np.arange(r.DEGENERATE_FRAMES) == r.DEGENERATE_FRAME
    assert not g[bad].view(np.uint32).any()                                   # +0.0 exactly
    err = float(cr.csi_errors(g[~bad], cr.ref_csi(f, rx)[~bad]).max())
    print("every other frame's csi off by %.3e, bound %.3e" % (err, cr.CSI_BOUND))
    assert err <= cr.CSI_BOUND
    assert rec.tobytes() == dem.run(rx).tobytes()


@pytest.mark.parametrize("force_table", (False, True))
@pytest.mark.parametrize("name", cr.WEIGHT_TABLES)
def test_weighted_demapper_bit_for_bit(c, name, force_table):
    for F, P in cr.WEIGHT_SHAPES:
        for n_frames in cr.WEIGHT_FRAMES:
            k = ch.check_weighted(c, name, F, P, n_frames, force_table)
    print(k)


def test_weighted_device_form_and_guard(c):
    m, table, node = ch.demap_node(c, "16qam", 100, False)
    z = sr.demap_input(table, 500, 3).reshape(5, 100)
    w = cr.weights_for(100, 48, 5, 4)
    want = cr.ref_weighted_llr(z.ravel(), w, table, 100)
    d_z, d_w = c.DeviceBuf(z.nbytes).upload(z), c.DeviceBuf(w.nbytes).upload(w)
    d_out = c.DeviceBuf(want.nbytes + ch.GUARD).upload(np.full(want.nbytes + ch.GUARD, 0xFF, np.uint8))
    node.run_dev(d_z.ptr, 5, d_out.ptr, weight_ptr=d_w.ptr, weight_period=48)
    raw = d_out.download(np.uint8, want.nbytes + ch.GUARD)
    assert np.all(raw[want.nbytes:] == 0xFF) and sr.same_floats(raw[: want.nbytes].view(np.float32).reshape(want.shape), want)


def test_capped_grids():
    """Every CSI case and every weighted shape again under the library's grid cap of 1 and 3 workgroups."""
    assert os.path.exists(DIAG_LIB), "the diagnostic build is part of build(): %s" % DIAG_LIB
    env = dict(os.environ, COMMS_HIP_LIB=DIAG_LIB)
    env.pop(ch.KNOB, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "csi_children.py")], env=env, capture_output=True, text=True, timeout=300)
    print(out.stdout[-4000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-3000:] + out.stderr[-3000:]


def test_argument_errors(c):
    lib = c.lib()
    f = r.FORMATS["n64_11a"]
    args, kw = f.node_args()
    dem = c.OfdmDemodNode(*args, **kw)
    buf = c.DeviceBuf(8 * (f.frame_samples + f.data_syms) + 4 * f.D + 64)
    d_in, d_out, d_csi = buf.ptr, buf.ptr + 8 * f.frame_samples, buf.ptr + 8 * (f.frame_samples + f.data_syms)
    run = lib.comms_ofdm_demod_csi_run_dev
    assert run(dem._h, d_in, 1, d_out, d_csi, None) == c.COMMS_OK                          # adjacent is not overlapping
    assert run(dem._h, d_in, 0, None, None, None) == c.COMMS_OK                            # n_frames = 0: a no-op
    assert run(dem._h, d_in, 1, d_out, None, None) == c.COMMS_ERR_ARG                      # NULL
    assert run(dem._h, d_in, 1, d_out, d_csi + 2, None) == c.COMMS_ERR_ARG                 # alignment
    assert run(dem._h, d_in, 1, d_out, d_out + 8, None) == c.COMMS_ERR_ARG                 # overlaps the records
    assert run(dem._h, d_in, 1, d_out, d_in + 8 * f.frame_samples - 4, None) == c.COMMS_ERR_ARG   # overlaps the input
    g = f.but(n_train=0)
    args0, kw0 = g.node_args()
    blind = c.OfdmDemodNode(*args0, **kw0)
    big = c.DeviceBuf(8 * (g.frame_samples + g.data_syms) + 4 * g.D)
    assert run(blind._h, big.ptr, 1, big.ptr + 8 * g.frame_samples, big.ptr + 8 * (g.frame_samples + g.data_syms), None) == c.COMMS_ERR_ARG
    with pytest.raises(c.CommsError) as e:
        blind.run(r.samples(g, 1), csi=True)                                               # T = 0: nothing to estimate
    assert e.value.code == c.COMMS_ERR_ARG
    assert dem.run(np.zeros((0, f.frame_samples), np.complex64), csi=True)[1].shape == (0, f.D)

    F = 20
    node = c.DemapNode(4, c.qam_table(4), F)
    z = np.zeros((2, F), np.complex64)
    for bad in (np.ones((2, 0), np.float32), np.ones((2, F + 1), np.float32)):             # P = 0, P > F
        with pytest.raises(c.CommsError) as e:
            node.run(z, weights=bad)
        assert e.value.code == c.COMMS_ERR_ARG
    dz, dw, do = c.DeviceBuf(8 * 2 * F), c.DeviceBuf(4 * 2 * F + 16), c.DeviceBuf(16 * 2 * F + 64)
    wrun = lib.comms_demap_run_weighted_dev
    assert wrun(node._h, dz.ptr, dw.ptr, F, 2, do.ptr, None) == c.COMMS_OK
    assert wrun(node._h, dz.ptr, dw.ptr, F, 0, None, None) == c.COMMS_OK
    assert wrun(node._h, dz.ptr, None, F, 2, do.ptr, None) == c.COMMS_ERR_ARG              # NULL weights
    assert wrun(node._h, dz.ptr, dw.ptr + 2, F, 2, do.ptr, None) == c.COMMS_ERR_ARG        # alignment
    assert wrun(node._h, dz.ptr, do.ptr + 16, 1, 2, do.ptr, None) == c.COMMS_ERR_ARG       # the weights overlap the output
    assert lib.comms_demap_run_weighted(node._h, z.ctypes.data, None, 1, 2, z.ctypes.data) == c.COMMS_ERR_ARG
    node.set_output_format("bits")
    assert wrun(node._h, dz.ptr, dw.ptr, F, 2, do.ptr, None) == c.COMMS_ERR_ARG            # BITS format
    with pytest.raises(c.CommsError) as e:
        c.DemapNode(4, c.qam_table(4), F).set_output_format("bits").run(z, weights=np.ones((2, 1), np.float32))
    assert e.value.code == c.COMMS_ERR_ARG


@pytest.mark.parametrize("m", sorted(cr.LINK_NOISE))
def test_coded_link_needs_the_weights(c, m):
    """ConvEncoderNode -> RateMatchNode (interleaver) -> SymbolMapNode -> OfdmModNode, csi_ref's channel and noise on the host,
    OfdmDemodNode with channel state -> DemapNode -> RateDematchNode -> ViterbiNode, decoded with and without the weights."""
    import viterbi_ref as vr

    L = cr.link_format(m)
    f, T, E = L["f"], L["T"], L["E"]
    payload, sent, tx_ref = cr.link_transmit(m)
    args, kw = f.node_args()
    enc = c.ConvEncoderNode(T, 7, vr.GENS[(7, 2)])
    match = c.RateMatchNode(E, None, cr.LINK_COLS)
    mapper = c.SymbolMapNode(m, c.qam_table(m), E)
    mod, dem = c.OfdmModNode(*args, **kw), c.OfdmDemodNode(*args, **kw)
    bits = match.run(enc.run(vr.pack_records(payload)))
    assert vr.unpack_records(bits, E).tobytes() == sent.tobytes()
    tx = mod.run(mapper.run(bits))
    assert r.symbol_errors(tx, tx_ref, f.sym_len).max() <= r.FFT_BOUND
    rx = cr.link_channel(m, tx)                                        # the reference's channel and noise, on the host

    s, s_flat, qscale = cr.link_scales(m)
    demap = c.DemapNode(m, c.qam_table(m), L["F"])
    dematch = c.RateDematchNode(E, None, cr.LINK_COLS)
    dec = c.ViterbiNode(T, 7, vr.GENS[(7, 2)], qscale=qscale)

    def decode(llr):
        return vr.unpack_records(dec.run(dematch.run(llr)), T)

    rec, g = dem.run(rx, csi=True)
    llr = demap.set_llr_scale(s).run(rec, weights=g)
    wrong = cr.frames_wrong(decode(llr), payload)
    flat = cr.frames_wrong(decode(demap.set_llr_scale(s_flat).run(rec)), payload)
    ref_flat = cr.frames_wrong(cr.link_receive(m, rx, False)[0], payload)
    print("m %d: %d of 16 frames wrong with weights, %d without (reference chain: %d), largest |q| %.1f" %
          (m, wrong, flat, ref_flat, float(np.abs(llr).max() * qscale)))
    assert wrong == 0
    assert flat >= 1

    dead = rx.copy().reshape(cr.LINK_FRAMES, -1, f.sym_len)
    dead[5, : f.n_train] = 0                                           # a frame without training symbols: all erasures
    rec0, g0 = dem.run(dead.reshape(rx.shape), csi=True)
    llr0 = demap.set_llr_scale(s).run(rec0, weights=g0)
    others = np.arange(cr.LINK_FRAMES) != 5
    assert not g0[5].view(np.uint32).any() and r.nonfinite(rec0[5]).all()
    assert not llr0[5].view(np.uint32).any() and not np.isnan(llr0).any()
    assert llr0[others].tobytes() == llr[others].tobytes()
    assert cr.frames_wrong(decode(llr0)[others], payload[others]) == 0


def test_host_graph_nodes(c):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "comms_rs_amd", "host"), "-s"], timeout=600)
    out = subprocess.run([os.path.join(ROOT, "comms_rs_amd", "lib", "test_csi_nodes_gpu")], capture_output=True, text=True, timeout=300, cwd=ROOT)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all passed" in out.stdout
