"""The soft demapper (comms_demap_*; demap_axis_kernel<MI, MQ, FMT>, demap_table_kernel<M, FMT>) on an MI355X at every split
mI + mQ = m of every m = 1 ... 8, at seven bits per symbol, on tables that leave the choice of the split open, on tables with
repeated levels and points and on tables scaled to where f32 squares are subnormal, against tests/symmap_ref.py's brute force and
tests/csi_ref.py's weighted form.  The contract is exact, so every comparison is equality: LLRs as uint32 with NaN matching NaN
by position, BITS records as bytes.  The cases are tests/demap_cases.py's (tests/test_demap_cases.py holds them to their rules).
The last test asserts that the launches of this module covered every instantiation, so run the module whole.  Run with -m gpu."""
import re

import numpy as np
import pytest

import csi_ref as cr
import demap_cases as dc
import symmap_ref as sr

pytestmark = pytest.mark.gpu
GUARD = 256
SEEN = set()        # the first word of kernel() of every launch of this module: "demap_axis_kernel<3,4,bits>"


@pytest.fixture(scope="module")
def c():
    import comms_rs_amd as c

    assert c.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested (no CPU fallback)"
    return c


def fields(name):
    return {a: int(b) for a, b in re.findall(r"(\w+)=(\d+)", name)}


def launch(c, node, z, frames, weights=None):
    """run_dev into a 0xFF-filled buffer with a guard region behind it; float32 (frames, F m) or uint8 (frames, record bytes)."""
    SEEN.add(node.kernel(frames).split(" ")[0])
    nbytes = frames * node.out_frame_bytes
    d_in = c.DeviceBuf(max(z.nbytes, 8)).upload(z)
    d_out = c.DeviceBuf(nbytes + GUARD).upload(np.full(nbytes + GUARD, 0xFF, np.uint8))
    if weights is None:
        node.run_dev(d_in.ptr, frames, d_out.ptr)
    else:
        d_w = c.DeviceBuf(weights.nbytes).upload(weights)
        node.run_dev(d_in.ptr, frames, d_out.ptr, weight_ptr=d_w.ptr, weight_period=weights.shape[1])
    raw = d_out.download(np.uint8, nbytes + GUARD)
    assert np.all(raw[nbytes:] == 0xFF), "the guard region was written"
    return raw[:nbytes].view(np.float32).reshape(frames, -1) if node.format == "llr" else raw[:nbytes].reshape(frames, -1)


def same_bytes(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def handles(c, m, table, split, F):
    """(the default handle, the forced-table one), their kernel() strings held to the contract's choice."""
    node, forced = c.DemapNode(m, table, F), c.DemapNode(m, table, F, force_table=True)
    kd, kf = node.kernel(2), forced.kernel(2)
    assert "form=table" in kf and kf.startswith("demap_table_kernel<%d,llr>" % m) and fields(kf)["points"] == 1 << m, kf
    if split is None:
        assert kd == kf
    else:
        assert "form=axis" in kd and kd.startswith("demap_axis_kernel<%d,%d,llr>" % split), kd
        assert fields(kd)["points"] == (1 << split[0]) + (1 << split[1]), kd
    for h in (node, forced):
        h.set_llr_scale(dc.LLR_SCALE)
    return node, forced


def check_table(c, name):
    """Both forms in LLR, BITS and weighted-LLR format at every length of the case, one frame and three."""
    m, table, split = dc.tables()[name]
    for F in dc.lengths(m):
        node, forced = handles(c, m, table, split, F)
        assert node.in_frame_bytes == 8 * F
        for frames in dc.FRAME_COUNTS:
            z = dc.case_input(table, F, frames)
            want_llr = sr.ref_llr_records(z, table, F, dc.LLR_SCALE)
            want_bits = sr.ref_bits_records(z, table, F)
            for h in (node, forced):
                assert h.out_frame_bytes == 4 * F * m
                got_llr = launch(c, h, z, frames)
                assert sr.same_floats(got_llr, want_llr), (name, F, frames, h.kernel(frames))
                h.set_output_format("bits")
                assert h.out_frame_bytes == sr.record_bytes(F * m) and ",bits>" in h.kernel(frames)
                got_bits = launch(c, h, z, frames)
                assert same_bytes(got_bits, want_bits), (name, F, frames, h.kernel(frames), np.argwhere(got_bits != want_bits)[:4])
                h.set_output_format("llr")
                bit = sr.unpack_records(got_bits, F * m)
                assert np.all(bit[got_llr > 0] == 0) and np.all(bit[got_llr < 0] == 1)
        for P in dc.weight_periods(F):                                         # (z: the three frames)
            w = cr.weights_for(F, P, frames, 9 + F + P)
            want = cr.ref_weighted_llr(z, w, table, F, dc.LLR_SCALE)
            for h in (node, forced):
                assert sr.same_floats(launch(c, h, z, frames, w), want), (name, F, P, h.kernel(frames))


# ------------------------------------------------------------------ every split
@pytest.mark.parametrize("mI,mQ", dc.SPLITS)
def test_every_split_equals_the_brute_force(c, mI, mQ):
    """The table's levels are distinct, so (mI, mQ) is the only split the library can have chosen; (3,4) and (4,3) are the
    per-axis form at seven bits per symbol."""
    check_table(c, dc.split_name(mI, mQ))


# ------------------------------------------------------------------ seven bits per symbol
def test_seven_bits_without_structure_run_the_table_form(c):
    assert dc.tables()["rand7"][2] is None
    check_table(c, "rand7")
    assert {"demap_table_kernel<7,llr>", "demap_table_kernel<7,bits>"} <= SEEN


@pytest.mark.parametrize("name", ["rand7"] + [dc.split_name(*s) for s in dc.SEP7])
def test_seven_bit_mapper_output_demaps_to_the_input_bits(c, name):
    m, table, split = dc.tables()[name]
    E, frames = 32 * m + 5, 4
    bits = np.random.default_rng(m).integers(0, 2, (frames, E), dtype=np.uint8)
    mapper = c.SymbolMapNode(m, table, E)
    F = mapper.out_frame_syms
    assert F * m > E and F * m % 32
    sym = np.ascontiguousarray(mapper.run(sr.dirty_records(bits, 2))).ravel()
    padded = np.zeros((frames, F * m), np.uint8)
    padded[:, :E] = bits
    for h in handles(c, m, table, split, F):
        assert same_bytes(launch(c, h.set_output_format("bits"), sym, frames), sr.pack_records(padded)), h.kernel(frames)


# ------------------------------------------------------------------ the packed records at every m
@pytest.mark.parametrize("m", range(1, 9))
def test_known_decisions_pack_into_the_right_words(c, m):
    """Symbols on table points in patterns whose records are known without arithmetic, a frame per pattern: a field of
    wave_words<M> that is dropped, doubled or shifted by one shows as a wrong byte."""
    table = dc.pack_table(m)
    split = (m // 2, m - m // 2)
    for F in dc.pack_lengths(m):
        parts = [dc.pattern_symbols(table, F, kind) for kind in dc.PATTERNS]
        z = np.concatenate([p[0] for p in parts])
        want = dc.index_records(np.concatenate([p[1] for p in parts]), m, F)
        for h in handles(c, m, table, split, F):
            got = launch(c, h.set_output_format("bits"), z, len(parts))
            assert same_bytes(got, want), (m, F, h.kernel(len(parts)), np.argwhere(got != want)[:4])


# ------------------------------------------------------------------ tables that leave a choice, repeated levels and points
@pytest.mark.parametrize("name", list(dc.ambiguous()))
def test_ambiguous_tables_take_the_contracts_split_and_the_lowest_index(c, name):
    check_table(c, name)
    m, table, split = dc.tables()[name]
    z = np.tile(table, 3)                                                      # symbols on the points themselves: exact ties
    for h in handles(c, m, table, split, table.size):
        assert same_bytes(launch(c, h.set_output_format("bits"), z, 3), sr.ref_bits_records(z, table, table.size)), h.kernel(3)


# ------------------------------------------------------------------ scaled tables
@pytest.mark.parametrize("name", list(dc.scaled()))
def test_scaled_tables_equal_the_reference(c, name):
    """At 2^-70 most squared differences are subnormal and the LLRs rest on them (test_demap_cases.py): f32 denormals are
    kept, not flushed."""
    check_table(c, name)


# ------------------------------------------------------------------ several passes per lane at m = 7
@pytest.mark.parametrize("name", ["rand7", dc.split_name(*dc.SEP7[0])])
def test_seven_bit_lanes_make_several_passes(c, name):
    m, table, split = dc.tables()[name]
    F = dc.PASS_F
    node, forced = handles(c, m, table, split, F)
    k = fields(node.kernel(10 ** 7))
    assert k["grid"] == k["max_grid"] == sr.GRID_CAP
    frames = k["grid"] * k["wg"] // F + 300
    z0 = sr.demap_input(table, dc.PASS_DISTINCT, 5)                            # the reference once, on the distinct symbols
    z = np.resize(z0, frames * F)
    want_llr = np.resize(sr.ref_llr(z0, table, dc.LLR_SCALE), (frames * F, m)).reshape(frames, F * m)
    want_bits = dc.index_records(np.resize(sr.ref_index(z0, table), frames * F), m, F)
    for h in (node,) if split is None else (node, forced):
        kk = fields(h.kernel(frames))
        assert kk["items"] > kk["grid"] * kk["wg"] and kk["grid"] == kk["max_grid"]
        assert sr.same_floats(launch(c, h, z, frames), want_llr), h.kernel(frames)
        h.set_output_format("bits")
        kk = fields(h.kernel(frames))
        assert kk["items"] == 2 * frames and kk["lanes"] > kk["grid"] * kk["wg"]
        assert same_bytes(launch(c, h, z, frames), want_bits), h.kernel(frames)


# ------------------------------------------------------------------ what ran
def test_every_instantiation_was_launched():
    """All 44 demap_axis_kernel<mI,mQ,..> splits and demap_table_kernel<M,..> for M = 1 ... 8, each as llr and as bits (the
    weighted form reports llr), by the tests above."""
    want = {"demap_axis_kernel<%d,%d,%s>" % (mI, mQ, fmt) for mI, mQ in dc.SPLITS for fmt in ("llr", "bits")}
    want |= {"demap_table_kernel<%d,%s>" % (m, fmt) for m in range(1, 9) for fmt in ("llr", "bits")}
    assert len(want) == 2 * 44 + 16
    assert not want - SEEN, sorted(want - SEEN)
    assert not SEEN - want, sorted(SEEN - want)
