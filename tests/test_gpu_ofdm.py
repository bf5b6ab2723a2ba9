"""OfdmModNode and OfdmDemodNode (ofdm.hip) on an MI355X against tests/ofdm_ref.py, the complex128 definition of
include/comms_hip.h's "OFDM modulator and demodulator".  Formats, inputs and bounds are ofdm_ref's (tests/test_ofdm_ref.py
holds them to their rules); no bound here comes from a kernel's output.  Every figure is printed before it is asserted."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import ofdm_ref as r

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 256   # bytes behind a device output, as in tests/test_gpu_symmap.py


def fields(name):
    return {a: int(b) for a, b in re.findall(r"(\w+)=(\d+)", name)}


@pytest.fixture(scope="module")
def c():
    import comms_rs_amd as c

    assert c.device_count() >= 1
    return c


def nodes(c, f):
    args, kw = f.node_args()
    return c.OfdmModNode(*args, **kw), c.OfdmDemodNode(*args, **kw)


def split_runs(node, x):
    """The same call in two: frames [0, 2) and [2, n)."""
    return np.concatenate([node.run(x[:2]), node.run(x[2:])])


@pytest.mark.parametrize("n_frames", r.FRAME_COUNTS)
@pytest.mark.parametrize("name", sorted(r.FORMATS))
def test_modulator(c, name, n_frames):
    f = r.FORMATS[name]
    mod, _ = nodes(c, f)
    assert (mod.data_syms, mod.frame_samples) == (f.data_syms, f.frame_samples)
    z = r.data_values(f, n_frames)
    got = mod.run(z)
    err, frame, sym = r.worst(r.symbol_errors(got, r.ref_mod(f, z), f.sym_len))
    print("%s frames %d: worst symbol %.3e (frame %d symbol %d)  [%s]" % (name, n_frames, err, frame, sym, mod.kernel(n_frames)))
    assert err <= r.FFT_BOUND, (name, err, frame, sym)
    s = got.reshape(n_frames, -1, f.sym_len)
    assert s[..., : f.n_cp].tobytes() == s[..., f.sym_len - f.n_cp:].tobytes()
    if n_frames > 2:
        assert split_runs(mod, z).tobytes() == got.tobytes()


@pytest.mark.parametrize("n_frames", r.FRAME_COUNTS)
@pytest.mark.parametrize("name", sorted(r.FORMATS))
def test_demodulator_without_training(c, name, n_frames):
    f = r.FORMATS[name].but(n_train=0)
    _, dem = nodes(c, f)
    rx = r.samples(f, n_frames)
    got = dem.run(rx)
    amp = f.n_fft * float(f.tx_scale)   # Z = Y / (N tx_scale): the same relative error as Y on the data bins
    want = r.ref_spectra(f, rx)[..., f.data_bins].reshape(n_frames, -1)
    err, frame, sym = r.worst(r.symbol_errors(got.astype(np.complex128) * amp, want, f.D))
    print("%s frames %d: worst symbol %.3e (frame %d symbol %d)  [%s]" % (name, n_frames, err, frame, sym, dem.kernel(n_frames)))
    assert err <= r.FFT_BOUND, (name, err, frame, sym)
    assert r.symbol_errors(got, r.ref_demod(f, rx), f.D).max() <= r.FFT_BOUND
    if n_frames > 2:
        assert split_runs(dem, rx).tobytes() == got.tobytes()


@pytest.mark.parametrize("n_frames", r.FRAME_COUNTS)
@pytest.mark.parametrize("name", r.CHANNEL_FORMATS)
def test_demodulator_behind_a_channel(c, name, n_frames):
    f, _, rx = r.channel_case(name, n_frames)
    _, dem = nodes(c, f)
    got = dem.run(rx)
    err, frame, sym = r.worst(r.symbol_errors(got, r.ref_demod(f, rx), f.D))
    print("%s frames %d: worst symbol %.3e (frame %d symbol %d), bound %.3e" % (name, n_frames, err, frame, sym, r.CHANNEL_BOUND))
    assert err <= r.CHANNEL_BOUND, (name, err, frame, sym)
    if n_frames > 2:
        assert split_runs(dem, rx).tobytes() == got.tobytes()


@pytest.mark.parametrize("n_frames", r.FRAME_COUNTS)
@pytest.mark.parametrize("name", r.CPE_FORMATS)
def test_pilot_phase_correction(c, name, n_frames):
    f, z, rx = r.channel_case(name, n_frames, cpe=True, rotate=True)
    _, dem = nodes(c, f)
    got = dem.run(rx)
    err, frame, sym = r.worst(r.symbol_errors(got, r.ref_demod(f, rx), f.D))
    print("%s frames %d: worst symbol %.3e (frame %d symbol %d), bound %.3e" % (name, n_frames, err, frame, sym, r.CHANNEL_BOUND))
    assert err <= r.CHANNEL_BOUND, (name, err, frame, sym)
    assert r.symbol_errors(got, z, f.D).max() <= 1e-5                      # the rotation is gone
    g = f.but(cpe=False)                                                   # flag off: it stays
    off = nodes(c, g)[1].run(rx)
    assert r.symbol_errors(off, r.ref_demod(g, rx), g.D).max() <= r.CHANNEL_BOUND
    th = r.symbol_thetas(g)[g.n_train:]
    want = z.reshape(n_frames, g.n_syms, g.D) * np.exp(1j * th)[None, :, None]
    assert r.symbol_errors(off, want.reshape(n_frames, -1), g.D).max() <= 1e-5


@functools.lru_cache(maxsize=None)
def training(name, n_frames, cpe, seed=0):
    """(format, received samples, ref_demod of them) of a training-sum case, computed once and shared read-only."""
    f, _, rx = r.training_case(name, n_frames, cpe, cpe, seed)
    want = r.ref_demod(f, rx)
    rx.setflags(write=False)
    want.setflags(write=False)
    return f, rx, want


TRAINING_CASES = [(name, cpe) for name, cpe, _ in r.training_cases()]


@pytest.mark.parametrize("n_frames", r.FRAME_COUNTS)
@pytest.mark.parametrize("name,cpe", TRAINING_CASES)
def test_demodulator_sums_every_training_symbol(c, name, cpe, n_frames):
    """T = 1 ... 2 ROUND + 1 training symbols that all differ: tests/test_ofdm_ref.py shows that a sum which leaves a slot out,
    or reads a neighbouring slot or the next wave's for it, is at least 10 bounds off in every one of these cases."""
    f, rx, want = training(name, n_frames, cpe)
    _, dem = nodes(c, f)
    got = dem.run(rx)
    err, frame, sym = r.worst(r.symbol_errors(got, want, f.D))
    print("%s cpe %d frames %d: worst symbol %.3e (frame %d symbol %d), bound %.3e  [%s]" %
          (name, cpe, n_frames, err, frame, sym, r.TRAINING_BOUND, dem.kernel(n_frames)))
    assert err <= r.TRAINING_BOUND, (name, err, frame, sym)
    if n_frames > 2:
        assert split_runs(dem, rx).tobytes() == got.tobytes()
    # other frames on the same handle, then the first again: nothing of a call (1 / H_k, the exchange buffers) reaches the next
    _, rx2, want2 = training(name, n_frames, cpe, seed=1)
    err2 = float(r.symbol_errors(dem.run(rx2), want2, f.D).max())
    print("    other frames: worst symbol %.3e" % err2)
    assert err2 <= r.TRAINING_BOUND, (name, err2)
    assert dem.run(rx).tobytes() == got.tobytes()


@pytest.mark.parametrize("n_frames", r.FRAME_COUNTS)
@pytest.mark.parametrize("name,cpe", TRAINING_CASES)
def test_demodulator_device_call_writes_its_records_and_no_more(c, name, cpe, n_frames):
    f, rx, want = training(name, n_frames, cpe)
    _, dem = nodes(c, f)
    nbytes = 8 * n_frames * f.data_syms
    d_in = c.DeviceBuf(rx.nbytes).upload(rx)
    d_out = c.DeviceBuf(nbytes + GUARD).upload(np.full(nbytes + GUARD, 0xFF, np.uint8))
    dem.run_dev(d_in.ptr, n_frames, d_out.ptr)
    raw = d_out.download(np.uint8, nbytes + GUARD)
    assert np.all(raw[nbytes:] == 0xFF), "the guard region was written"
    assert not np.any(raw[:nbytes].view(np.uint32) == 0xFFFFFFFF), "an output value was not written"
    got = raw[:nbytes].view(np.complex64).reshape(n_frames, -1)
    err = float(r.symbol_errors(got, want, f.D).max())
    print("%s cpe %d frames %d: worst symbol %.3e, bound %.3e" % (name, cpe, n_frames, err, r.TRAINING_BOUND))
    assert err <= r.TRAINING_BOUND, (name, err)
    assert dem.run(rx).tobytes() == got.tobytes()


@pytest.mark.parametrize("n_frames", r.FRAME_COUNTS)
@pytest.mark.parametrize("name", r.LONG_TRAINING_FORMATS)
def test_modulator_with_long_training(c, name, n_frames):
    """T of a round or more: the block rule gives a frame blocks of whole rounds, and the first of them holds training symbols
    only (block <= T, asserted from kernel() for every call of one frame)."""
    f = r.TRAINING_FORMATS[name]
    mod, _ = nodes(c, f)
    assert (mod.data_syms, mod.frame_samples) == (f.data_syms, f.frame_samples)
    z = r.data_values(f, n_frames)
    got = mod.run(z)
    k = fields(mod.kernel(n_frames))
    err, frame, sym = r.worst(r.symbol_errors(got, r.ref_mod(f, z), f.sym_len))
    print("%s frames %d: worst symbol %.3e (frame %d symbol %d)  [%s]" % (name, n_frames, err, frame, sym, mod.kernel(n_frames)))
    assert err <= r.FFT_BOUND, (name, err, frame, sym)
    s = got.reshape(n_frames, -1, f.sym_len)
    assert s[..., : f.n_cp].tobytes() == s[..., f.sym_len - f.n_cp:].tobytes()
    assert (k["block"], k["blocks"]) == r.block_rule(f.n_fft, f.n_train + f.n_syms, n_frames, k["max_grid"]) and k["train"] == f.n_train
    if n_frames == 1:
        assert k["block"] == r.round_of(f.n_fft) <= f.n_train and k["blocks"] >= 2, k      # block 0: training symbols only
    else:
        assert split_runs(mod, z).tobytes() == got.tobytes()


@pytest.mark.parametrize("kind", r.DEGENERATE_KINDS)
def test_degenerate_frames_stay_in_their_frame(c, kind):
    """include/comms_hip.h: a symbol whose pilot sum is 0 or not finite is left unrotated (all zeros; NaN or infinite values);
    a frame whose training sum is 0 is NaN or infinite throughout.  One frame of five is degenerate: the others, and in the
    first two kinds the frame's other symbols, are held to the bound."""
    f, rx = r.degenerate_case(kind)
    with np.errstate(all="ignore"):
        want = r.ref_demod(f, rx)
    _, dem = nodes(c, f)
    got = dem.run(rx)
    err = r.check_degenerate(f, kind, got, want, r.TRAINING_BOUND)
    print("%s: every other symbol within %.3e, bound %.3e  [%s]" % (kind, err, r.TRAINING_BOUND, dem.kernel(r.DEGENERATE_FRAMES)))
    assert split_runs(dem, rx).tobytes() == got.tobytes()


def test_link_16qam_bits_are_exact(c):
    f = r.FORMATS[r.LINK_FORMAT]
    table = c.qam_table(4)
    n_bits = 4 * f.data_syms
    bits = np.random.default_rng(9).integers(0, 2, (r.LINK_FRAMES, n_bits), dtype=np.uint8)
    records = np.packbits(bits, axis=1, bitorder="little")
    mapper = c.SymbolMapNode(4, table, n_bits)
    assert mapper.out_frame_syms == f.data_syms and mapper.in_frame_bytes == records.shape[1]
    mod, dem = nodes(c, f)
    rx = r.through_channel(f, mod.run(mapper.run(records)))
    demap = c.DemapNode(4, table, f.data_syms).set_output_format("bits")
    got = demap.run(dem.run(rx))
    assert got[:, : records.shape[1]].tobytes() == records.tobytes()


def test_host_graph_nodes(c):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "comms_rs_amd", "host"), "-s"], timeout=600)
    out = subprocess.run([os.path.join(ROOT, "comms_rs_amd", "lib", "test_ofdm_nodes_gpu")], capture_output=True, text=True, timeout=300, cwd=ROOT)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all passed" in out.stdout


def test_argument_errors(c):
    f = r.FORMATS["n64_11a"]
    args, kw = f.node_args()

    def refused(*a, **k):
        with pytest.raises(c.CommsError) as e:
            c.OfdmModNode(*a, **k)
        return e.value.code == c.COMMS_ERR_ARG

    assert refused(96, 16, np.ones(96, np.uint8), n_syms=3)                                   # bad N
    assert refused(64, 65, f.kind, **kw)                                                       # CP > N
    assert refused(64, 16, np.zeros(64, np.uint8), n_syms=3)                                   # no data carrier
    bad = f.train.copy()
    bad[f.data_bins[3]] = 0
    assert refused(*args, **dict(kw, train=bad))                                               # train zero on a used bin
    assert refused(64, 16, r.map_all_data(64), n_syms=3, cpe=True)                             # CPE without pilots
    assert refused(*args, **dict(kw, n_syms=0))
    assert refused(*args, **dict(kw, tx_scale=0.0))
    mod, dem = nodes(c, f)
    assert mod.run(np.zeros((0, f.data_syms), np.complex64)).shape == (0, f.frame_samples)     # n_frames = 0: a no-op
    assert dem.run(np.zeros((0, f.frame_samples), np.complex64)).shape == (0, f.data_syms)
    lib = c.lib()
    assert lib.comms_ofdm_mod_run_dev(mod._h, None, 0, None, None) == c.COMMS_OK
    assert lib.comms_ofdm_mod_run_dev(mod._h, None, 1, None, None) == c.COMMS_ERR_ARG
    assert lib.comms_ofdm_data_syms(None) == 0 and lib.comms_ofdm_frame_samples(None) == 0
    # overlapping buffers: refused before any launch (the buffer holds either direction's ranges)
    buf = c.DeviceBuf(8 * 2 * (f.frame_samples + f.data_syms))
    assert lib.comms_ofdm_mod_run_dev(mod._h, buf.ptr, 1, buf.ptr + 8 * (f.data_syms - 1), None) == c.COMMS_ERR_ARG
    assert lib.comms_ofdm_demod_run_dev(dem._h, buf.ptr + 8, 1, buf.ptr, None) == c.COMMS_ERR_ARG
    assert lib.comms_ofdm_demod_run_dev(dem._h, buf.ptr, 1, buf.ptr + 8 * f.frame_samples, None) == c.COMMS_OK   # adjacent is not overlapping
