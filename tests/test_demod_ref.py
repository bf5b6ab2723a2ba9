"""tests/demod_ref.py held to its conditions without a GPU: the oracle's Nco agrees with the exact int64 / np.longdouble
reference on every stream the GPU tests run, the timing filters meet every seam of timing_kernel's passes, and every timing
block is coherent enough to test an angle on."""
import numpy as np

import demod_ref as dr
import oracle
import syncest_ref as sr


def test_exact_rotor_is_exact_where_the_answer_is_known():
    assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is no wider than f64 here"
    assert float(dr.TWO_PI) == 2 * np.pi and abs(float(dr.TWO_PI - np.longdouble(2 * np.pi)) - 2.4492935982947064e-16) < 2.2e-19   # half an ulp of the 64-bit mantissa
    k = np.array([0, 1, -1, 1 << 40, -(1 << 40)], dtype=np.int64)
    got = dr.rotor_exact(k)
    assert got[0] == 1.0 and got[1] == np.exp(1j * dr.UNIT) and got[2] == np.conj(got[1])
    turns = int(round((1 << 40) * dr.UNIT / (2 * np.pi)))             # 1024 rad: 163 turns, reduced in extended precision
    assert abs(got[3] - np.exp(1j * float(np.longdouble(1024.0) - turns * dr.TWO_PI))) < 2e-16 and got[4] == np.conj(got[3])
    # the cumulative sum: increment first, then the output (nco.rs:72-76)
    e = np.array([5, -7, 11], dtype=np.int64)
    assert dr.nco_phases(100, 3, e).tolist() == [108, 104, 118] and dr.nco_exact(100, 3, e)[1] == 118
    assert dr.nco_exact(100, 3, e[:0])[1] == 100


def test_nco_inputs_cover_what_they_claim():
    assert dr.N_BIG == (8 * 256 + 3) * 2048 + 5 and dr.N_LONG > dr.SWEEP * dr.TILE and dr.N_CUT == 3 * 2048 + 5
    assert {e.size for _, _, _, e in dr.small_cases()} == set(dr.SMALL_N) == {1, 2, 3, 511, 512, 513, 2047, 2048, 2049, 4095, 4097}
    assert {(np.sign(d), p0) for _, d, p0, _ in dr.small_cases()} == {(1, dr.P_NEAR_TURN), (-1, dr.P_QUARTER)}
    assert 0 < 2 * np.pi - dr.P_NEAR_TURN * dr.UNIT < dr.UNIT
    for kind, lo, hi in (("small", 0.007, 0.0079), ("large", 49.0, 50.0)):
        for e in [e for nm, _, _, e in dr.small_cases() if nm.startswith(kind) and e.size >= 2047] + [dr.cut_stream(kind)[2]]:
            assert lo < np.max(np.abs(e)) * dr.UNIT < hi
    big = dr.big_stream()[2]
    assert 40.0 < np.max(np.abs(big)) * dr.UNIT < 50.0 and np.mean(np.abs(big) * dr.UNIT > 2 * np.pi) > 0.5   # whole turns in most steps
    # neighbouring tiles, tiles a grid apart and tiles a sweep apart have different sums: a scan that permutes, drops or repeats
    # tile sums, or carries the wrong total into the second sweep, moves every phase behind it
    for d, _, e in (dr.big_stream(), dr.long_stream()):
        sums = np.add.reduceat(d + e, np.arange(0, e.size, dr.TILE))
        assert np.unique(sums).size == sums.size
    # the cuts: one sample, an odd index, both sides of a tile edge, single-sample calls across one
    assert dr.CUTS["at-1"] == (1,) and dr.CUTS["odd"][0] % 2 == 1
    assert {dr.CUTS[k][0] for k in ("2047", "2048", "2049")} == {2047, 2048, 2049}
    s = dr.CUTS["single-samples-across-an-edge"]
    assert np.all(np.diff(s) == 1) and s[0] < 2 * dr.TILE < s[-1]
    for cuts in dr.CUTS.values():
        assert list(cuts) == sorted(cuts) and 0 < cuts[0] and cuts[-1] < dr.N_CUT


def test_oracle_nco_agrees_with_the_exact_reference_on_every_gpu_input():
    worst = {}

    def held(name, got, want, phase, k_end):
        d = float(np.max(np.abs(got - want)))
        dp = abs(np.exp(1j * phase) - dr.rotor_exact(np.array([k_end]))[0])
        worst[name.split("-")[0]] = max(worst.get(name.split("-")[0], 0.0), d, dp)
        assert d <= dr.ORACLE_NCO_TOL and dp <= dr.ORACLE_NCO_TOL, (name, d, dp)

    for name, d, p0, e in dr.small_cases():
        got, phase = dr.oracle_nco(p0, d, e)
        want, k_end = dr.nco_exact(p0, d, e)
        held(name, got, want, phase, k_end)
    for kind in dr.KINDS:
        d, p0, e = dr.cut_stream(kind)
        want, k_end = dr.nco_exact(p0, d, e)
        for name, cuts in [("uncut", ())] + list(dr.CUTS.items()):
            got, phase = dr.oracle_nco(p0, d, e, cuts)
            held("cut-" + kind + name, got, want, phase, k_end)
    d, p0, e = dr.big_stream()
    got, phase = dr.oracle_nco(p0, d, e)
    want, k_end = dr.nco_exact(p0, d, e)                                 # every sample
    held("big", got, want, phase, k_end)
    d, p0, e = dr.long_stream()                                          # tests/test_estimators.py; its first call (the second doubles
    got, phase = dr.oracle_nco(p0, d, e)                                 # the oracle's wraps by fl(2 pi): 1.6e-10 from the exact values)
    idx = dr.seam_indices(e.size)
    want, k_end = dr.nco_exact(p0, d, e, idx)
    held("long", got[idx], want, phase, k_end)
    print("oracle Nco against the exact reference:", {k: "%.2e" % v for k, v in worst.items()}, "(tolerance %.0e)" % dr.ORACLE_NCO_TOL)


def test_timing_filters_meet_every_seam_of_the_passes():
    taps = {(n, d): 2 * n * d + 1 for n, d in dr.FILTERS}
    assert [taps[f] for f in dr.FILTERS] == [1, 3, 11, 13, 1019, 1019, 1021, 2041, 2041, 2601]
    passes = {f: dr.pass_lengths(*f) for f in dr.FILTERS}
    assert passes[(4, 0)] == passes[(1, 1)] == passes[(5, 1)] == [12] and passes[(3, 2)] == [24]
    assert passes[(509, 1)] == passes[(1, 509)] == [1020]                 # exactly one full pass
    assert passes[(10, 51)] == [1020, 12]                                 # twelve taps spill
    assert passes[(1, 1020)] == passes[(3, 340)] == [1020, 1020, 12] and passes[(2, 650)] == [1020, 1020, 564]
    for f, p in passes.items():
        assert sum(p) == (taps[f] + 11) // 12 * 12 and all(nk % 12 == 0 and 0 < nk <= dr.TE_QMAX for nk in p)
    # timing_kernel steps its LDS blocks by 4 or 5 slots according to (nk - 1) & 7: both residues of nk mod 8
    assert {nk % 8 for p in passes.values() for nk in p} == {0, 4}
    assert {n for n, _ in dr.FILTERS} >= {1} and any(d == 0 for _, d in dr.FILTERS)
    for n, d in dr.FILTERS:
        nd = n * d
        assert set(dr.block_lengths(n, d)) == {nd, nd + 1, 2047, 2048, 2049, 2048 + nd, 2 * 2048 + nd + 1}
        assert oracle.qfilt_taps(2 * nd + 1, dr.ALPHA, n).size == taps[(n, d)]
    assert abs(dr.ANGLE_TOL - 2 * np.pi * 1e-9 / 10) < 1e-24


def test_timing_blocks_are_coherent_and_the_oracle_takes_them():
    """The condition the angle bound rests on, on exactly the blocks the GPU test estimates; and the oracle against the f64
    restatement of syncest_ref on them (the two fold the same products in different orders)."""
    assert len(dr.timing_cases()) == 2 * sum(len(dr.block_lengths(n, d)) for n, d in dr.FILTERS)
    low, worst = 1.0, 0.0
    for kind, n, d, ln in dr.timing_cases():
        x = dr.timing_block(kind, n, d, ln)
        want = dr.timing_reference(kind, n, d, ln)
        assert x.size == ln and x.dtype == np.complex128
        if ln <= n * d:                                                    # no product: atan2(0, 0) = 0, times -n
            assert want == 0.0 and np.signbit(want), (kind, n, d, ln, want)
            continue
        ts, _, ta, _ = sr.ref_sums(x, n, d, dr.ALPHA)
        assert abs(ts) / ta >= sr.MIN_COHERENCE, (kind, n, d, ln, abs(ts) / ta)
        low = min(low, abs(ts) / ta)
        if ln == n * d + 1:                                                # one product
            assert abs(abs(ts) / ta - 1.0) < 1e-12 and x[0] != 0
        err = dr.angle_error(sr.timing_of(ts, n), want, n)
        worst = max(worst, err)
        assert err <= dr.ANGLE_TOL / 100, (kind, n, d, ln, err)
        if kind == "sparse":
            assert 1 <= np.count_nonzero(x) <= 8 and (np.count_nonzero(x) >= 4 or len(dr.sparse_positions(n, d, ln)) < 4)
            assert set(np.flatnonzero(x).tolist()) <= set(dr.sparse_positions(n, d, ln))
    print("timing blocks: lowest coherence %.3f (condition %.2f), oracle against the f64 restatement %.2e rad (device bound %.2e)"
          % (low, sr.MIN_COHERENCE, worst, dr.ANGLE_TOL))
    # pure noise does not qualify as an angle input
    rng = np.random.default_rng(0)
    noise = rng.standard_normal(4096) + 1j * rng.standard_normal(4096)
    assert dr.coherence(noise, 4, 0) < 2 * sr.MIN_COHERENCE


def test_sparse_blocks_put_energy_on_the_tile_edges_and_the_filter_offsets():
    """Over the sparse blocks of one filter, impulses sit on a tile edge - 1, + 0 and + 1 and n d away from one, and -- where
    the filter takes several passes -- k_lo away from one."""
    for n, d in dr.FILTERS:
        nd, hit = n * d, set()
        for ln in dr.block_lengths(n, d):
            pos = np.flatnonzero(dr.timing_block("sparse", n, d, ln))
            for p in pos.tolist():
                for e in (-1, 0, 1):
                    if p >= dr.TILE - 1 and (p - e) % dr.TILE == 0:
                        hit.add(("edge", e))
                    if nd and ((p - e - nd) % dr.TILE == 0 and p - nd >= dr.TILE - 1 or (p - e + nd) % dr.TILE == 0):
                        hit.add("nd")
                    for k_lo in range(dr.TE_QMAX, 2 * nd + 1, dr.TE_QMAX):
                        if (p - e - k_lo) % dr.TILE == 0 or (p - e + k_lo) % dr.TILE == 0:
                            hit.add("k_lo")
        want = {("edge", -1), ("edge", 0), ("edge", 1)} | ({"nd"} if nd else set()) | ({"k_lo"} if 2 * nd + 1 > dr.TE_QMAX else set())
        assert hit >= want, (n, d, want - hit)
