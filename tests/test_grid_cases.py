"""The capped-grid case table (tests/grid_cases.py) held to its rules: a case for every persistent kernel, at least four passes
and a ragged last one, both sides of every seam, every regime of the (frame, position) walks, small calls, and inputs that
meet the conditions the nodes' tolerances rest on.  No GPU."""
import os
import re

import numpy as np

import deframe_ref as dr
import framesync_ref as fr
import grid_cases as gc
import ratematch_ref as rr
import symmap_ref as sm
import syncest_ref as sr
import viterbi_ref as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_formulas_still_stand_in_the_source():
    texts = {}
    for path, text in gc.ANCHORS:
        if path not in texts:
            with open(os.path.join(ROOT, path)) as f:
                texts[path] = f.read()
        assert text in texts[path], "%s no longer reads %r: restate the launch in tests/grid_cases.py" % (path, text)


def test_every_persistent_kernel_has_a_case():
    """Every .hip file that sizes a grid by resident_workgroups( -- or by grid_cap( itself: the two handles of demod.hip -- has a
    case per call of it."""
    csrc = os.path.join(ROOT, "comms_rs_amd", "csrc")
    calls = {}
    for name in sorted(os.listdir(csrc)):
        if name.endswith(".hip"):
            with open(os.path.join(csrc, name)) as f:
                n = len(re.findall(r"\b(?:resident_workgroups|grid_cap)\(", f.read()))
            if n:
                calls[name] = n
    assert calls == {"demod.hip": 2, "syncest.hip": 1, "symsync.hip": 1, "framesync.hip": 1, "resample.hip": 1, "channelizer.hip": 1, "deframe.hip": 1,
                     "convcode.hip": 2, "ratematch.hip": 2, "crc.hip": 1, "symmap.hip": 2, "ofdm.hip": 1}, calls
    have = {}
    for cs in gc.CASES:
        have.setdefault(cs.kernel, set()).add(cs.fmt.get("node") or cs.fmt.get("dir") or "")
    assert {k: len(v) for k, v in have.items()} == calls
    assert have["demod.hip"] == {"timing", "nco"}
    assert have["convcode.hip"] == {"encoder", "viterbi"} and have["ratematch.hip"] == {"tx", "rx"} and have["symmap.hip"] == {"map", "demap"}
    assert {cs.fmt["direction"] for cs in gc.cases_of("ofdm")} == {"mod", "demod"}     # ofdm.hip takes its cap once for both
    assert {cs.family for cs in gc.CASES} == set(gc.FAMILIES)


def test_every_case_makes_four_passes_and_a_ragged_last_one():
    for cs in gc.CASES:
        for cap in gc.CAPS:
            w = gc.walk(cs, cap)
            assert w.passes >= gc.MIN_PASSES, (cs.name, cap, w)
            assert w.grid == cap, (cs.name, cap, w)
            assert gc.ragged(cs, cap) or gc.never_ragged(cs, cap), (cs.name, cap, w)
    # the exceptions are the frames and receive lengths the workgroup divides and the OFDM kernels' one item per pass, at cap 1 only
    assert [(cs.name, cap) for cs in gc.CASES for cap in gc.CAPS if not gc.ragged(cs, cap)] == \
        [("F2048-K%d-%s" % (K, fmt), 1) for K in (1, 2) for fmt in ("bits", "llr")] + [("rx-N256", 1), ("rx-N2048", 1)] + \
        [(cs.name, 1) for cs in gc.cases_of("ofdm")]
    assert {cs.fmt["F"] for cs in gc.cases_of("deframe")} >= {64, 2048}                 # the issue's two frame lengths


def test_no_case_moves_more_than_a_few_megabytes():
    for cs in gc.CASES:
        for cap in gc.CAPS:
            assert gc.bytes_moved(cs, cap) <= gc.MAX_BYTES, (cs.name, cap, gc.bytes_moved(cs, cap))


def test_grid_dependent_steps_take_nonzero_residues():
    # syncest: mt_step = (gridDim.x * SE_TILE) % n2
    by_n = {cs.fmt["n"]: [(cap * gc.SE_TILE) % (2 * cs.fmt["n"]) for cap in gc.CAPS] for cs in gc.cases_of("syncest")}
    assert by_n[4] == by_n[8] == [0, 0, 0]                          # the issue's two formats: powers of two, never a residue
    assert sum(r != 0 for r in by_n[3]) == 2 and all(by_n[5]) and len({*by_n[5]}) == 3
    # resample: step_p = (gridDim.x TO M) % L at every tile its planner may choose
    for L, M, N, _ in gc.RESAMPLE_FORMATS:
        for TO in (16, 32, 64, 128, 256, 512, 1024):
            assert sum((cap * TO * M) % L != 0 for cap in gc.CAPS) >= 2, (L, M, TO)
    assert any(L & (L - 1) for L, _, _, _ in gc.RESAMPLE_FORMATS)


def test_tile_planned_cases_reach_more_than_the_largest_tile():
    """symsync: four, two and one output per lane in flight, the last on a tile narrower than 256 lanes; resample: a tile of 256
    outputs, one trip per lane, beside the larger ones (the plans are tests/plan_cases.py's, pinned to the source there)."""
    import plan_cases as pc

    ss = [pc.symsync_tile(cs.fmt["L"], cs.fmt["S"], cs.fmt["N"]).plan for cs in gc.cases_of("symsync")]
    assert {p.U for p in ss} == {4, 2, 1} and any(p.TO <= 128 and p.WG == p.TO for p in ss)
    assert all(cs.fmt["mu"] < cs.fmt["S"] * cs.fmt["L"] for cs in gc.cases_of("symsync"))
    rs = [pc.resample_tile(cs.fmt["L"], cs.fmt["M"], cs.fmt["N"], cs.fmt["dtype"]).plan for cs in gc.cases_of("resample")]
    assert {p.TO for p in rs} >= {1024, 256} and all(p.tab_lds for p in rs)


def test_seam_cases_sit_on_both_sides():
    rx = [cs.fmt["n_coded"] for cs in gc.cases_of("ratematch") if cs.fmt["dir"] == "rx"]
    tx = [cs.fmt["n_tx"] for cs in gc.cases_of("ratematch") if cs.fmt["dir"] == "tx"]
    for sizes in (rx, tx):
        assert any(v <= rr.LDS_SEAM for v in sizes) and any(v > rr.LDS_SEAM for v in sizes)
    assert rr.LDS_SEAM in rx and rr.LDS_SEAM + 1 in rx
    assert sorted(gc.rm_tx_words(E) for E in tx) == sorted(gc.RM_TX_WORDS) and {64, 65} <= set(gc.RM_TX_WORDS)   # 2045 and 2077 bits
    for cs in gc.cases_of("ratematch"):
        assert rr.n_tx_bits(cs.fmt["n_coded"], gc.P34) == cs.fmt.get("n_tx", rr.n_tx_bits(cs.fmt["n_coded"], gc.P34)) >= gc.RM_COLS
    steps = [cs.fmt["steps"] for cs in gc.cases_of("convcode") if cs.fmt["node"] == "viterbi"]
    assert vr.LDS_STEPS in steps and steps.count(vr.LDS_STEPS + 1) == 2 and {6, 70} <= set(steps)
    assert {cs.fmt["n"] for cs in gc.cases_of("convcode") if cs.fmt.get("steps") == vr.LDS_STEPS + 1} == {2, 3}
    assert any(cs.fmt.get("kinds") == ("special", "noisy") for cs in gc.cases_of("convcode"))


def test_constellation_cases_reach_the_seams():
    """symmap.hip takes its grid cap twice (the mapper, the demapper): ragged map calls, fields that straddle two words and
    fields that do not, both demapper forms in both formats, a record that is no whole number of 64-symbol chunks and one of
    several chunks."""
    maps = [cs.fmt for cs in gc.cases_of("symmap") if cs.fmt["node"] == "map"]
    demaps = [cs.fmt for cs in gc.cases_of("symmap") if cs.fmt["node"] == "demap"]
    assert all(gc.ragged(cs, cap) for cs in gc.cases_of("symmap") for cap in gc.CAPS)
    assert {32 % f["m"] != 0 for f in maps} == {True, False}
    assert any(f["P"] and f["G"] for f in maps) and any(not f["P"] and not f["G"] for f in maps)
    for fmt in ("llr", "bits"):
        assert {sm.table_of(f["table"])[3] is None for f in demaps if f["fmt"] == fmt} == {True, False}      # table form, per-axis form
        assert {(f["table"], f["F"]) for f in demaps if f["fmt"] == fmt} == set(gc.SYMMAP_DEMAP_FORMATS)
    assert any(f["F"] % 64 for f in demaps) and any(f["F"] > 64 for f in demaps)


def test_ofdm_cases_reach_every_transform_and_a_ragged_group():
    """The three shapes of the transform (N = 64: no third step; 512 and 1024: radix 2 and 4 in it), the pilot phase correction
    and the channel estimate in every case, and a last group of a block that a wave does not fill."""
    assert {f.n_fft for f in gc.OFDM_FORMATS.values()} >= {64, 512, 1024}
    for cs in gc.cases_of("ofdm"):
        f, direction = gc.OFDM_FORMATS[cs.fmt["format"]], cs.fmt["direction"]
        assert f.cpe and f.n_train
        for cap in gc.CAPS:
            items = gc.walk(cs, cap).total
            assert cap == 1 or items % cap, (cs.name, cap)                   # the last pass is ragged across workgroups ...
        per_frame = f.n_syms + (f.n_train if direction == "mod" else 0)
        assert per_frame % (1024 // f.n_fft) or f.n_fft == 1024              # ... and the last group of a block within a wave


def test_ofdm_training_case_redoes_a_sum_of_three_rounds_per_item():
    """n512_t17: 2 ROUND + 1 training symbols that all differ, on the demodulator, whose workgroups walk four or more items and
    sum the training spectra anew for each.  The conditions TRAINING_BOUND rests on hold on these calls: the f32 model is within
    a quarter of the bound of the definition, and every wrong training sum moves a symbol by ten bounds or more."""
    import ofdm_ref as r

    assert gc.OFDM_TRAINING == {"n512_t17": "n512_cp36_t17"} and gc.OFDM_DIRECTIONS == {"n512_t17": ("demod",)}
    (cs,) = [cs for cs in gc.cases_of("ofdm") if cs.fmt["format"] == "n512_t17"]
    f = gc.OFDM_FORMATS["n512_t17"]
    assert (f.n_fft, f.n_train, f.cpe) == (512, 2 * r.round_of(512) + 1, True) and cs.fmt["direction"] == "demod"
    for cap in gc.CAPS:
        frames = cs.size(cap)
        g, _, rx = r.training_case("n512_cp36_t17", frames, cpe=True, rotate=True)
        assert g.frame_samples == f.frame_samples and gc.walk(cs, cap).passes >= gc.MIN_PASSES
        want = r.ref_demod(f, rx)
        assert r.symbol_errors(r.model_demod(f, rx), want, f.D).max() <= r.TRAINING_MODEL_WORST, (cap, frames)
        for _, t, src in r.training_mutants(f):
            moved = r.symbol_errors(r.ref_demod(f, r.mutant_samples(f, rx, t, src)), want, f.D)
            assert moved.max(axis=1).min() >= r.TRAINING_SENSITIVITY * r.TRAINING_BOUND, (cap, t, src)      # in every frame


def test_rate_matching_walks_take_every_regime():
    """RmWalk by its additions equals the division at every item of every case, and the cases meet its four regimes: no whole
    frame per stride, whole frames and a remainder, no remainder, and a lane that carries on every step -- one of them on
    `pos == per`, where `>` for `>=` would leave the frame."""
    seen = {"rx": set(), "tx": set()}
    for cs in gc.cases_of("ratematch"):
        d = cs.fmt["dir"]
        per = cs.fmt["n_coded"] if d == "rx" else gc.rm_tx_words(cs.fmt["n_tx"])
        for cap in gc.CAPS:
            w = gc.walk(cs, cap)
            stride = w.grid * gc.WG
            seen[d].add(gc.rm_regime(stride, per))
            for first in range(0, stride, max(stride // 97, 1)):
                assert gc.rm_walk_positions(first, stride, per, w.total) == [divmod(i, per) for i in range(first, w.total, stride)]
                carries, on_equal = gc.rm_carries(first, stride, per, w.total)
                if len(carries) >= gc.MIN_PASSES - 1 and all(carries):
                    seen[d].add("carry on every step")
                if on_equal:
                    seen[d].add("carry on equality")
                    wrong = gc.rm_walk_positions(first, stride, per, w.total, strict=True)
                    assert any(pos == per for _, pos in wrong), (cs.name, cap, first)   # position `per`: the next record, or past the table
    everything = {"stride_frames=0", "stride_frames>=1", "stride_pos=0", "carry on every step", "carry on equality"}
    assert seen["rx"] == everything, seen["rx"]
    assert seen["tx"] == everything, seen["tx"]


def test_deframe_walks_take_every_regime():
    """The deframer steps (frame, pos) by dq = stride div lpf, dr = stride mod lpf with the same carry: replayed against the
    division at every case, and met in every regime -- 64 lanes: dr = 0; 2048 and 2053: dq = 0, at 2048 and cap 1 a carry on
    `pos == lpf`; 100, 112 lanes: whole frames and a remainder."""
    seen = set()
    for cs in gc.cases_of("deframe"):
        lpf = gc.deframe_lpf(cs.fmt["F"], cs.fmt["K"], cs.fmt["fmt"])
        for cap in gc.CAPS:
            w = gc.walk(cs, cap)
            stride = w.grid * gc.WG
            seen.add(gc.rm_regime(stride, lpf))
            for first in range(0, stride, max(stride // 97, 1)):
                assert gc.rm_walk_positions(first, stride, lpf, w.total) == [divmod(i, lpf) for i in range(first, w.total, stride)]
                carries, on_equal = gc.rm_carries(first, stride, lpf, w.total)
                if any(carries) and gc.rm_regime(stride, lpf) == "stride_frames>=1":
                    seen.add("whole frames, a remainder and a carry")
                if on_equal:
                    seen.add("carry on equality")
    assert seen == {"stride_frames=0", "stride_frames>=1", "stride_pos=0", "whole frames, a remainder and a carry", "carry on equality"}, seen
    for cs in gc.cases_of("deframe"):                              # F = 2048 at cap 1: two frames, the eighth step carries, on equality
        if cs.fmt["F"] == 2048:
            assert cs.size(1) == 2 and gc.rm_carries(0, gc.WG, 2048, gc.walk(cs, 1).total) == ([False] * 7 + [True] + [False] * 7, True)


def test_viterbi_frames_that_would_share_a_slot_differ():
    """A condition on the inputs: frames two apart -- the waves a slot indexed by frame parity would bring together -- and
    neighbouring frames decode to different bits in every "noisy" case, so a survivor slot shared or left stale shows."""
    for cs in gc.cases_of("convcode"):
        f = cs.fmt
        if f["node"] != "viterbi":
            continue
        for cap in gc.CAPS:
            frames = cs.size(cap)
            assert frames >= 4 * cap * vr.WAVES + 3
            for kind in f["kinds"]:
                vc = vr.make_case(f["K"], f["n"], f["terminated"], f["steps"], frames, kind)
                _, llr, bits, _ = vr.case_data(vc)
                assert llr.shape[0] == frames
                if f["steps"] > 6:                                  # (six steps: 64 words at most, frames repeat)
                    for lag in (1, 2, 4 * cap):
                        assert np.all(np.any(bits[lag:] != bits[:-lag], axis=1)), (cs.name, cap, kind, lag)


def test_crc_cases_reach_every_group_and_corrupt_every_pass():
    import crc_ref

    groups = [crc_ref.group_of(T) for _, T in gc.CRC_FORMATS]
    assert groups == [1, 2, 64, 64] and [gc.cdiv((T + 31) // 32, g) for (_, T), g in zip(gc.CRC_FORMATS, groups)] == [1, 1, 1, 2]
    for cs in gc.cases_of("crc"):
        fpw = 64 // crc_ref.group_of(cs.fmt["T"])
        for cap in gc.CAPS:
            frames, w = cs.size(cap), gc.walk(cs, cap)
            assert fpw == 1 or frames % fpw != 0                   # the last wave-item is partly empty
            bad = gc.crc_corrupted(frames)
            waves = w.grid * 4
            item = bad // fpw
            for p in range(w.passes):                              # every pass of the grid meets corrupted frames ...
                assert np.any(item // waves == p), (cs.name, cap, p)
            for wave in range(waves):                              # ... and so does every wave
                assert np.any(item % waves == wave), (cs.name, cap, wave)
            assert 0 < bad.size < frames                           # ... and clean ones


def test_framesync_inputs_keep_the_decision_margin():
    """The condition framesync_ref's tolerances rest on (tests/test_framesync_ref.py), on these streams; the detections are the
    planted words, which sit on the tile edges of a workgroup's third and fourth pass."""
    for cs in gc.cases_of("framesync"):
        P, G, thr = cs.fmt["P"], cs.fmt["G"], cs.fmt["thr"]
        w = gc.framesync_word(cs.fmt["word"])
        assert w.size == P and G == P - 1
        for cap in gc.CAPS:
            y = gc.framesync_stream(P, cap)
            planted = gc.framesync_positions(P, G, cap)
            k, c, m, e, mm = fr.ref_detect(y, w, thr, G)
            assert k.tolist() == planted, (cs.name, cap, k, planted)
            assert float(np.min(np.abs(mm - thr))) >= fr.DECISION_MARGIN
            for ki, mi in zip(k, m):
                i = ki + G
                assert np.all(mi - np.concatenate([mm[i - G: i], mm[i + 1: i + G + 1]]) >= fr.DECISION_MARGIN), (cs.name, ki)
            tiles_of = {(kk + P + G - 1) // gc.FS_TILE for kk in planted}
            assert {t // cap for t in tiles_of} >= {2, 3}          # third and fourth passes
            edge = [(kk + P + G - 1) % gc.FS_TILE for kk in planted]
            assert 0 in edge and gc.FS_TILE - 1 in edge
            assert any(kk // gc.FS_TILE != (kk + P - 1) // gc.FS_TILE for kk in planted)   # a word across two tiles' symbols
            mk, mc, mmm, me, _ = fr.model_detect(y, w, thr, G)
            Ep = float(np.sum(np.abs(w.astype(np.complex128)) ** 2))
            assert np.array_equal(mk, k) and np.max(np.abs(mmm - m)) <= fr.MODEL_METRIC_DISTANCE
            assert np.max(np.abs(mc - c) / np.sqrt(Ep * e)) <= fr.MODEL_CORR_DISTANCE and np.max(np.abs(me - e) / e) <= fr.MODEL_CORR_DISTANCE


def test_syncest_inputs_are_within_the_model_distance():
    """The condition syncest_ref's tolerances rest on (tests/test_syncest_ref.py), on these blocks."""
    for cs in gc.cases_of("syncest"):
        n, d, alpha = cs.fmt["n"], cs.fmt["d"], cs.fmt["alpha"]
        for cap in gc.CAPS:
            x = gc.syncest_signal(cs, cap)
            ts, fs, ta, fa = sr.ref_sums(x, n, d, alpha)
            mts, mfs = sr.model_sums(x, n, d, alpha)
            assert abs(ts) / ta >= sr.MIN_COHERENCE and abs(fs) / fa >= sr.MIN_COHERENCE, (cs.name, cap)
            assert abs(mts - ts) / ta <= sr.MODEL_SUM_DISTANCE, (cs.name, cap, abs(mts - ts) / ta)
            assert sr.circ(sr.timing_of(mts, n), sr.timing_of(ts, n), n) <= sr.MODEL_TIMING_DISTANCE, (cs.name, cap)
            assert abs(mfs - fs) <= sr.FREQ_SUM_TOL * fa


def test_demod_inputs_meet_their_conditions():
    """The demod family: the filter lengths of one, exactly one, two and three passes; timing blocks coherent enough to test an
    angle on (tests/test_demod_ref.py's condition); NCO streams on which the oracle agrees with the exact reference, with tile
    sums that all differ, in both error ranges."""
    import demod_ref as dm

    timing = [cs for cs in gc.cases_of("demod") if cs.fmt["node"] == "timing"]
    assert [cs.fmt["n"] * cs.fmt["d"] for cs in timing] == [50, 509, 510, 1300]
    assert [dm.pass_lengths(cs.fmt["n"], cs.fmt["d"]) for cs in timing] == [[108], [1020], [1020, 12], [1020, 1020, 564]]
    for cs in timing:
        for cap in gc.CAPS:
            x = gc.demod_timing_block(cs, cap)
            assert x.size == cs.size(cap) and dm.coherence(x, cs.fmt["n"], cs.fmt["d"], cs.fmt["alpha"]) >= sr.MIN_COHERENCE, (cs.name, cap)
    nco = [cs for cs in gc.cases_of("demod") if cs.fmt["node"] == "nco"]
    assert [cs.fmt["errors"] for cs in nco] == ["small", "large"]
    for cs in nco:
        for cap in gc.CAPS:
            d, p0, e = gc.demod_nco_stream(cs, cap)
            assert e.size == 2 * cs.size(cap)
            sums = np.add.reduceat(d + e, np.arange(0, e.size, gc.NCO_TILE))
            assert np.unique(sums).size == sums.size
            got, phase = dm.oracle_nco(p0, d, e, (cs.size(cap),))
            want, k_end = dm.nco_exact(p0, d, e)
            assert np.max(np.abs(got - want)) <= dm.ORACLE_NCO_TOL, (cs.name, cap)
            assert abs(np.exp(1j * phase) - dm.rotor_exact(np.array([k_end]))[0]) <= dm.ORACLE_NCO_TOL


def test_deframe_inputs_keep_the_decision_margin():
    """The condition deframe_ref's exact bits rest on (tests/test_deframe_ref.py), on these streams; one call emits every frame."""
    done = set()
    for cs in gc.cases_of("deframe"):
        for cap in gc.CAPS:
            F, K, frames = cs.fmt["F"], cs.fmt["K"], cs.size(cap)
            if (F, K, frames) in done:
                continue
            done.add((F, K, frames))
            case = gc.deframe_case(F, K, frames)
            dets = dr.detect(case.y)
            assert dets["index"].tolist() == [7 + (dr.P + F + 3) * i for i in range(frames)]
            calls = dr.plan(case.y, dets, [])
            ref, left = dr.ref_frames(case, case.y, calls)
            assert left == 0 and ref[0]["index"].size == frames
            z = dr.joined(ref, "z").reshape(-1)
            assert float(np.min(dr.boundary_margin(z, dr.table_of(case)))) >= dr.DECISION_MARGIN
