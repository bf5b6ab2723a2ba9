"""The child processes of tests/test_gpu_small_grids.py: `python grid_children.py FAMILY` runs every case of one node family
from tests/grid_cases.py on handles made under COMMS_GRID_CAP = 1, 3 and 7 (the diagnostic build, which the parent selects
through COMMS_HIP_LIB).  Per case and cap: kernel() must report max_grid == grid == cap and the table's pass count; the outputs
are held to the node's own reference at the bound of its own GPU test, and -- syncest and the f64 timing estimator excepted,
whose partial sums are one per workgroup -- to the bits of the same calls on an uncapped handle of this process.  The first failure ends the process: an
assertion or a CommsError is an uncaught exception, and nothing is launched behind it.  The last line is "ok"."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import grid_cases as gc  # noqa: E402
import plan_cases  # noqa: E402

KNOB = "COMMS_GRID_CAP"


def fields(name):
    return {a: int(b) for a, b in re.findall(r"([\w/]+)=(\d+)", name)}


def make(factory, cap=None):
    """A handle made under the cap (None: the full chip); the knob is read at create."""
    if cap is None:
        os.environ.pop(KNOB, None)
    else:
        os.environ[KNOB] = str(cap)
    try:
        return factory()
    finally:
        os.environ.pop(KNOB, None)


def held(cs, cap, k, total, unit):
    """kernel()'s fields against the cap and the table: `total` items, `unit` per workgroup and pass."""
    w = gc.walk(cs, cap)
    assert k["max_grid"] == cap and k["grid"] == w.grid == cap, (cs.name, cap, k)
    assert total == w.total and gc.cdiv(total, k["grid"] * unit) == w.passes >= gc.MIN_PASSES, (cs.name, cap, k, w)
    return w


def rand_c(rng, n):
    return (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(np.complex64)


# ---------------------------------------------------------------- syncest
def syncest(c):
    import oracle
    import syncest_ref as sr

    for cs in gc.cases_of("syncest"):
        n, d, alpha = cs.fmt["n"], cs.fmt["d"], cs.fmt["alpha"]
        plain = make(lambda: c.SyncEstimatorNode(n, d, alpha))
        for cap in gc.CAPS:
            x = gc.syncest_signal(cs, cap)
            node = make(lambda: c.SyncEstimatorNode(n, d, alpha), cap)
            k = fields(node.kernel(x.size))
            held(cs, cap, k, k["tiles"], 1)
            assert k["tile"] == gc.SE_TILE and x.size % gc.SE_TILE != 0
            ts, fs, ta, fa = sr.ref_sums(x, n, d, alpha)
            X = x.astype(np.complex128)
            timing, freq = oracle.timing_push(X, n, d, alpha), oracle.frequency_offset_estimate(X)
            for got in (node.run(x), node.run(x), plain.run(x)):     # the second call: the partials of the first are overwritten
                dts, dt = abs(got.timing_sum - ts) / ta, sr.circ(got.timing, timing, n)
                dfs = abs(got.freq_sum - fs) / fa
                print("syncest %s cap %d: timing sum off by %.3e (tolerance %.3e), estimate by %.3e samples (%.3e), freq sum by %.3e (%.3e)"
                      % (cs.name, cap, dts, sr.TIMING_SUM_TOL, dt, sr.TIMING_TOL, dfs, sr.FREQ_SUM_TOL))
                assert dts <= sr.TIMING_SUM_TOL and dt <= sr.TIMING_TOL, (cs.name, cap, dts, dt)
                assert dfs <= sr.FREQ_SUM_TOL and abs(got.freq - freq) <= sr.ANGLE_TOL, (cs.name, cap, dfs)


# ---------------------------------------------------------------- demod: the f64 timing estimator and the NCO
def demod(c):
    import demod_ref as dm
    import oracle

    for cs in gc.cases_of("demod"):
        if cs.fmt["node"] == "nco":
            for cap in gc.CAPS:
                d, p0, e = gc.demod_nco_stream(cs, cap)
                n = cs.size(cap)
                new = lambda: c.NcoNode(float(dm.rad(d)), float(dm.rad(p0)))  # noqa: E731
                node, plain = make(new, cap), make(new)
                k = fields(node.kernel(n))
                held(cs, cap, k, k["tiles"], 1)
                assert k["tile"] == gc.NCO_TILE and n % gc.NCO_TILE != 0 and fields(plain.kernel(n))["max_grid"] == 8 * 256
                want, k_end = dm.nco_exact(p0, d, e)
                x = dm.rad(e)
                # two calls in a row: the tile offsets, the apply kernel's wave totals and the carried phase are used again
                got = np.concatenate([node.run(x[:n]), node.run(x[n:])])
                err = float(np.max(np.abs(got - want)))
                dp = abs(np.exp(1j * node.phase) - dm.rotor_exact(np.array([k_end]))[0])
                print("demod %s cap %d: 2 x %d samples, %d passes, off the exact values by %.3e, the phase by %.3e (tolerance %.0e)"
                      % (cs.name, cap, n, gc.walk(cs, cap).passes, err, dp, dm.NCO_TOL))
                assert err <= dm.NCO_TOL and dp <= dm.NCO_TOL, (cs.name, cap, err, dp)
                assert np.concatenate([plain.run(x[:n]), plain.run(x[n:])]).tobytes() == got.tobytes(), (cs.name, cap)
                assert plain.phase == node.phase
            continue
        n, d, alpha = cs.fmt["n"], cs.fmt["d"], cs.fmt["alpha"]
        plain = make(lambda: c.TimingEstimatorNode(n, d, alpha))
        for cap in gc.CAPS:
            x = gc.demod_timing_block(cs, cap)
            node = make(lambda: c.TimingEstimatorNode(n, d, alpha), cap)
            k = fields(node.kernel(x.size))
            held(cs, cap, k, k["tiles"], 1)
            assert k["tile"] == gc.TE_TILE and x.size % gc.TE_TILE != 0 and fields(plain.kernel(x.size))["max_grid"] == 4 * 256
            assert k["taps"] == 2 * n * d + 1 and k["filter_passes"] == len(dm.pass_lengths(n, d))
            want = oracle.timing_push(x, n, d, alpha)
            got = node.run(x)
            errs = [dm.angle_error(g, want, n) for g in (got, plain.run(x))]
            print("demod %s cap %d: %d samples, %d filter passes, estimate %.6f off the oracle's by %.3e rad of the sum, uncapped %.3e (tolerance %.3e)"
                  % (cs.name, cap, x.size, k["filter_passes"], got, errs[0], errs[1], dm.ANGLE_TOL))
            assert max(errs) <= dm.ANGLE_TOL, (cs.name, cap, errs)
            again = node.run(x)                                       # the second push: qacc and the partials are overwritten
            assert np.float64(again).tobytes() == np.float64(got).tobytes(), (cs.name, cap, got, again)


# ---------------------------------------------------------------- framesync
def framesync(c):
    import framesync_ref as fr

    def whole(node, y):
        return np.concatenate([node.run(y, raw=True), node.flush(raw=True)])

    for cs in gc.cases_of("framesync"):
        P, G, thr = cs.fmt["P"], cs.fmt["G"], cs.fmt["thr"]
        word = gc.framesync_word(cs.fmt["word"])
        Ep = float(np.sum(np.abs(word.astype(np.complex128)) ** 2))
        for cap in gc.CAPS:
            y = gc.framesync_stream(P, cap)
            node = make(lambda: c.FrameSyncNode(word, thr, G), cap)
            k = fields(node.kernel(y.size))
            held(cs, cap, k, k["tiles"], 1)
            assert k["tile"] == gc.FS_TILE and y.size % gc.FS_TILE != 0
            got = whole(node, y)
            idx, rc, rm, re_, _ = fr.ref_detect(y, word, thr, G)
            assert np.array_equal(got["index"].astype(np.int64), idx) and idx.tolist() == gc.framesync_positions(P, G, cap), (cs.name, cap, got["index"])
            corr = got["corr_re"].astype(np.float64) + 1j * got["corr_im"].astype(np.float64)
            dm = float(np.max(np.abs(got["metric"] - rm)))
            dc = float(np.max(np.abs(corr - rc) / np.sqrt(Ep * re_)))
            de = float(np.max(np.abs(got["energy"] - re_) / re_))
            print("framesync %s cap %d: %d detections, metric off by %.3e (tolerance %.3e), corr by %.3e, energy by %.3e (%.3e)"
                  % (cs.name, cap, got.size, dm, fr.METRIC_TOL, dc, de, fr.CORR_TOL))
            assert dm <= fr.METRIC_TOL and dc <= fr.CORR_TOL and de <= fr.CORR_TOL, (cs.name, cap, dm, dc, de)
            assert whole(make(lambda: c.FrameSyncNode(word, thr, G)), y).tobytes() == got.tobytes(), (cs.name, cap)
            node.set_position(0)                                      # the same handle again: count and list start over
            assert whole(node, y).tobytes() == got.tobytes(), (cs.name, cap)


# ---------------------------------------------------------------- symsync, resample: two calls of 4 cap + 1 tiles on one handle
def symsync(c):
    from resample_ref import bound
    from symsync_ref import SymSyncRef

    for cs in gc.cases_of("symsync"):
        L, S, N, mu = cs.fmt["L"], cs.fmt["S"], cs.fmt["N"], cs.fmt["mu"]
        rng = np.random.default_rng(100 * L + N)
        taps = rng.uniform(-1, 1, N).astype(np.float32)

        def new():
            node = c.SymbolSyncNode(taps, L, S)
            node.timing = mu / float(L)
            return node

        for cap in gc.CAPS:
            node, plain, ref = make(new, cap), make(new), SymSyncRef(taps, L, S)
            ref.mu = mu
            TO, worst = fields(node.kernel(S))["tile"], 0.0
            assert TO == plan_cases.symsync_tile(L, S, N).plan.TO <= gc.TILE_MAX        # the tile gc.bytes_moved counts with
            for call, cut in enumerate((TO // 2 + 1, 1)):             # the second call ends one output into its last tile
                n_out = (cs.size(cap) - 1) * TO + cut
                x = rand_c(rng, S * n_out)
                k = fields(node.kernel(x.size))
                held(cs, cap, k, k["tiles"], 1)
                got, want = node.run(x), ref.run(x)
                d = float(np.max(np.abs(got.astype(np.complex128) - want)))
                b = bound(taps, ref.x_max)
                worst = max(worst, d / b)
                assert got.shape == want.shape and d <= b, (cs.name, cap, call, d, b)
                assert plain.run(x).tobytes() == got.tobytes(), (cs.name, cap, call)
            assert np.array_equal(node.state, ref.state())
            print("symsync %s cap %d: tile %d, worst error %.3f of the bound" % (cs.name, cap, TO, worst))


def resample(c):
    from resample_ref import ResampleRef, bound, out_len

    for cs in gc.cases_of("resample"):
        L, M, N = cs.fmt["L"], cs.fmt["M"], cs.fmt["N"]
        dtype = np.complex64 if cs.fmt["dtype"] == "c32" else np.float32
        rng = np.random.default_rng(1000 + 7 * L + N)
        taps = rng.uniform(-1, 1, N).astype(np.float32)
        for cap in gc.CAPS:
            node, plain, ref = make(lambda: c.ResampleNode(taps, L, M, dtype), cap), make(lambda: c.ResampleNode(taps, L, M, dtype)), ResampleRef(taps, L, M, dtype)
            k0 = fields(node.kernel(1))
            TO, worst = k0["tile"], 0.0
            assert TO == plan_cases.resample_tile(L, M, N, cs.fmt["dtype"]).plan.TO <= gc.TILE_MAX and "resample_kernel" in node.kernel(1)
            print("resample %s cap %d: tile %d, (cap tile M) mod L = %d" % (cs.name, cap, TO, cap * TO * M % L))
            for call, cut in enumerate((TO // 3 + 1, 1)):
                n = ((cs.size(cap) - 1) * TO + cut) * M // L
                while gc.cdiv(out_len(n, L, M), TO) < cs.size(cap):
                    n += 1
                assert out_len(n, L, M) % TO != 0
                x = rand_c(rng, n) if dtype == np.complex64 else rng.uniform(-1, 1, n).astype(np.float32)
                k = fields(node.kernel(n))
                held(cs, cap, k, k["tiles"], 1)
                got, want = node.run(x), ref.run(x)
                d = float(np.max(np.abs(got.astype(np.complex128) - want)))
                b = bound(taps, ref.x_max)
                worst = max(worst, d / b)
                assert got.shape == want.shape and d <= b, (cs.name, cap, call, d, b)
                assert plain.run(x).tobytes() == got.tobytes(), (cs.name, cap, call)
            print("resample %s cap %d: worst error %.3f of the bound" % (cs.name, cap, worst))


# ---------------------------------------------------------------- channelizer
def channelizer(c):
    from channelizer_ref import ChannelizerRef, check, out_len

    for cs in gc.cases_of("channelizer"):
        M, D, N, layout = cs.fmt["M"], cs.fmt["D"], cs.fmt["N"], cs.fmt["layout"]
        rng = np.random.default_rng(1000 * M + N)
        taps = rng.uniform(-1, 1, N).astype(np.float32)
        for cap in gc.CAPS:
            new = lambda: c.ChannelizerNode(taps, M, D, layout=layout)  # noqa: E731
            node, plain, ref = make(new, cap), make(new), ChannelizerRef(taps, M, D, layout)
            F = fields(node.kernel(1))["frames/tile"]
            assert 1 < F <= gc.CHZ_TILE_POINTS // M
            for call, cut in enumerate((F // 2, 1)):
                frames = (cs.size(cap) - 1) * F + cut
                n = frames * D
                assert out_len(n, D) == frames
                x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
                name = node.kernel(n)
                k = fields(name)
                assert "channelizer_kernel" in name and k["max_grid"] == cap and k["grid"] == cap and k["tiles"] == cs.size(cap), name
                assert gc.cdiv(k["tiles"], k["grid"]) == gc.walk(cs, cap).passes >= gc.MIN_PASSES
                got = node.run(x)
                check(got, ref.run(x), ref, (cs.name, cap, call))
                assert plain.run(x).tobytes() == got.tobytes(), (cs.name, cap, call)
            print("channelizer %s cap %d: %d frames per tile, within its bound" % (cs.name, cap, F))


# ---------------------------------------------------------------- deframe
def deframe(c):
    import deframe_ref as dr

    for cs in gc.cases_of("deframe"):
        F, K, fmt = cs.fmt["F"], cs.fmt["K"], cs.fmt["fmt"]
        for cap in gc.CAPS:
            frames = cs.size(cap)
            case = gc.deframe_case(F, K, frames)
            dets = dr.detect(case.y)
            calls = dr.plan(case.y, dets, [])
            new = lambda: c.DeframeNode(F, case.offset, case.lookback, K).set_output_format(fmt).set_llr_scale(case.scale)  # noqa: E731
            node, plain = make(new, cap), make(new)
            k = fields(node.kernel(frames))
            held(cs, cap, k, k["lanes"], k["wg"])
            out = []
            for nd in (node, plain):
                parts, at = [], 0
                for n, d in calls:
                    parts.append(nd.run(case.y[at: at + n], d))
                    at += n
                out.append(np.concatenate(parts))
            got = out[0]
            ref, left = dr.ref_frames(case, case.y, calls)
            assert left == 0 and got.shape[0] == frames == ref[0]["index"].size
            if fmt == "bits":
                assert np.array_equal(got, dr.records(case, dr.joined(ref, "values"))), (cs.name, cap)
                print("deframe %s cap %d: %d frames, exact" % (cs.name, cap, frames))
            else:
                z, llr = dr.joined(ref, "z"), dr.joined(ref, "llr")
                dmax = np.max(np.abs(z[..., None] - dr.table_of(case).astype(np.complex128)) ** 2, axis=-1)
                rel = np.abs(got - llr).reshape(z.shape + (K,)) / (float(np.float32(case.scale)) * dmax)[..., None]
                print("deframe %s cap %d: %d frames, LLR off by %.3e of s max d (tolerance %.3e)" % (cs.name, cap, frames, float(np.max(rel)), dr.LLR_TOL))
                assert got.shape == llr.shape and float(np.max(rel)) <= dr.LLR_TOL, (cs.name, cap)
            assert out[1].tobytes() == got.tobytes(), (cs.name, cap)


# ---------------------------------------------------------------- convolutional code
def convcode(c):
    import viterbi_ref as vr

    for cs in gc.cases_of("convcode"):
        f = cs.fmt
        gens = vr.GENS[(f["K"], f["n"])]
        if f["node"] == "encoder":
            new = lambda: c.ConvEncoderNode(f["T"], f["K"], gens)  # noqa: E731
            plain = make(new)
            for cap in gc.CAPS:
                frames = cs.size(cap)
                node = make(new, cap)
                k = fields(node.kernel(frames))
                held(cs, cap, k, k["words"], k["wg"])
                sent = np.random.default_rng(f["T"] + cap).integers(0, 2, (frames, f["T"]), dtype=np.uint8)
                records = vr.pack_records(sent) | ~vr.pack_records(np.ones((frames, f["T"]), np.uint8))   # bits from T on do not count
                got = node.run(records)
                assert np.array_equal(got, vr.pack_records(vr.ref_encode(sent, f["K"], gens, True))), (cs.name, cap)
                assert plain.run(records).tobytes() == got.tobytes(), (cs.name, cap)
                print("convcode %s cap %d: %d frames, exact" % (cs.name, cap, frames))
            continue
        form = "lds" if f["steps"] <= vr.LDS_STEPS else "workspace"
        for cap in gc.CAPS:
            frames = cs.size(cap)
            node = plain = None
            for kind in f["kinds"]:                                   # the calls of one capped handle: a stale slot would show
                vc = vr.make_case(f["K"], f["n"], f["terminated"], f["steps"], frames, kind)
                new = lambda: c.ViterbiNode(vc.T, vc.K, vc.gens, terminated=vc.terminated, record_llrs=vc.record_llrs, qscale=vc.qscale)  # noqa: E731
                node, plain = node or make(new, cap), plain or make(new)
                name = node.kernel(frames)
                k = fields(name)
                assert name.startswith("viterbi_kernel<%d,%s>" % (f["n"], form)) and k["steps"] == f["steps"], name
                held(cs, cap, k, frames, k["waves"])
                slot = gc.cdiv(f["steps"], 64) * 64 * 8               # a wave's survivors
                assert (k["workspace"], k["lds"]) == ((cap * k["waves"] * slot, 0) if form == "workspace" else (0, k["waves"] * slot)), name
                _, llr, bits, metric = vr.case_data(vc)
                got, met = node.run(llr, metrics=True)
                assert np.array_equal(met, metric), (cs.name, cap, kind)
                assert np.array_equal(got, vr.pack_records(bits)), (cs.name, cap, kind)
                pg, pm = plain.run(llr, metrics=True)
                assert pg.tobytes() == got.tobytes() and np.array_equal(pm, met), (cs.name, cap, kind)
            print("convcode %s cap %d: %d frames x %s, bits and metrics exact" % (cs.name, cap, frames, "+".join(f["kinds"])))


# ---------------------------------------------------------------- rate matching
def ratematch(c):
    import ratematch_ref as rr

    for cs in gc.cases_of("ratematch"):
        N = cs.fmt["n_coded"]
        E = rr.n_tx_bits(N, gc.P34)
        scr = rr.scramble_bits(E, N)
        src, _ = rr.build_map(N, gc.P34, gc.RM_COLS)
        rx = cs.fmt["dir"] == "rx"
        new = lambda: (c.RateDematchNode if rx else c.RateMatchNode)(N, gc.P34, gc.RM_COLS, None, rr.pack_bits(scr))  # noqa: E731
        plain = make(new)
        for cap in gc.CAPS:
            frames = cs.size(cap)
            node = make(new, cap)
            name = node.kernel(frames)
            k = fields(name)
            held(cs, cap, k, k["values"] if rx else k["words"], k["wg"])
            assert ("table=lds" in name) == ((N if rx else E) <= rr.LDS_SEAM) and (k["lds"] > 0) == ("table=lds" in name), name
            if rx:
                data = rr.llr_words(frames, E, E, N + cap).view(np.float32)
                want = rr.ref_rx(data.view(np.uint32), src, N, scr)
                got = node.run(data)
                assert np.array_equal(got.view(np.uint32), want), (cs.name, cap, int(np.count_nonzero(got.view(np.uint32) != want)))
            else:
                bits = np.random.default_rng(N + cap).integers(0, 2, (frames, N), dtype=np.uint8)
                data = rr.pack_records(bits) | ~rr.pack_records(np.ones((frames, N), np.uint8))
                got = node.run(data)
                assert np.array_equal(got, rr.pack_records(rr.ref_tx(bits, src, scr))), (cs.name, cap)
            assert plain.run(data).tobytes() == got.tobytes(), (cs.name, cap)
            print("ratematch %s cap %d: %d frames, %s, %s, exact" % (cs.name, cap, frames, name.split(" seam")[0].split("wg=256 ")[1],
                                                                      gc.rm_regime(cap * gc.WG, N if rx else gc.rm_tx_words(E))))


# ---------------------------------------------------------------- CRC
def crc(c):
    import crc_ref as cr

    for cs in gc.cases_of("crc"):
        W, T = cs.fmt["W"], cs.fmt["T"]
        p = cr.SHAPE_PARAMS[W]
        new_att = lambda: c.CrcAttachNode(p.W, p.poly, p.init, p.xorout, T)  # noqa: E731
        new_chk = lambda: c.CrcCheckNode(p.W, p.poly, p.init, p.xorout, T)  # noqa: E731
        plain_att, plain_chk = make(new_att), make(new_chk)
        for cap in gc.CAPS:
            frames = cs.size(cap)
            att, chk = make(new_att, cap), make(new_chk, cap)
            for node, kname in ((att, "crc_attach_kernel"), (chk, "crc_check_kernel")):
                name = node.kernel(frames)
                k = fields(name)
                assert name.startswith(kname) and k["group"] == cr.group_of(T) and k["rounds"] == gc.cdiv((T + 31) // 32, k["group"]), name
                held(cs, cap, k, gc.cdiv(frames, 64 // k["group"]), 4)
            bits, dirty = cr.dirty_payload(frames, T, 100 * W + cap)
            got = att.run(dirty)
            assert np.array_equal(got, cr.pack_records(cr.ref_attach(bits, p))), (cs.name, cap)
            assert plain_att.run(dirty).tobytes() == got.tobytes(), (cs.name, cap)
            # the check: one flipped bit in the corrupted frames, the device counter over two calls
            full = np.zeros((frames, 8 * chk.in_frame_bytes), np.uint8)
            full[:, : T + W] = cr.ref_attach(bits, p)
            bad = gc.crc_corrupted(frames)
            full[bad, (7 * bad) % (T + W)] ^= 1
            records = np.packbits(full, axis=1, bitorder="little")
            want_payload, want_pass, want_crc = cr.ref_check(full, p, T)
            n_bad = int(np.count_nonzero(want_pass == 0))
            assert n_bad == bad.size
            d_in = c.DeviceBuf(records.nbytes).upload(records)
            counter = c.DeviceBuf(4).upload(np.zeros(1, np.uint32))
            for call in (1, 2):
                d_pay, d_pass, d_crc = c.DeviceBuf(frames * chk.out_frame_bytes), c.DeviceBuf(4 * frames), c.DeviceBuf(4 * frames)
                chk.run_dev(d_in.ptr, frames, d_pay.ptr, d_pass.ptr, d_crc.ptr, counter.ptr)
                payload = d_pay.download(np.uint8, frames * chk.out_frame_bytes).reshape(frames, -1)
                assert np.array_equal(d_pass.download(np.int32, frames), want_pass), (cs.name, cap, call)
                assert np.array_equal(d_crc.download(np.uint32, frames), want_crc), (cs.name, cap, call)
                assert np.array_equal(payload, cr.pack_records(want_payload)), (cs.name, cap, call)
                assert int(counter.download(np.uint32, 1)[0]) == call * n_bad, (cs.name, cap, call)
            pp, ps, pc = plain_chk.run(records)
            assert pp.tobytes() == payload.tobytes() and np.array_equal(ps, want_pass) and np.array_equal(pc, want_crc) and plain_chk.n_failed == n_bad
            print("crc %s cap %d: %d frames, %d failed, exact" % (cs.name, cap, frames, n_bad))


# ---------------------------------------------------------------- symbol mapper and demapper
def symmap(c):
    import symmap_ref as sm

    for cs in gc.cases_of("symmap"):
        f = cs.fmt
        if f["node"] == "map":
            m, E, P, G = f["m"], f["E"], f["P"], f["G"]
            table = sm.table_of(f["table"])[1]
            word = sm.noisy_points(sm.QPSK, P, 3) if P else None
            new = lambda: c.SymbolMapNode(m, table, E, word, G)  # noqa: E731
            plain = make(new)
            for cap in gc.CAPS:
                frames = cs.size(cap)
                node = make(new, cap)
                k = fields(node.kernel(frames))
                held(cs, cap, k, k["syms"], k["wg"])
                bits = np.random.default_rng(E + cap).integers(0, 2, (frames, E), dtype=np.uint8)
                records = sm.dirty_records(bits, 1)
                got = node.run(records)
                assert got.tobytes() == sm.ref_map(bits, m, table, word, G).tobytes(), (cs.name, cap)
                assert plain.run(records).tobytes() == got.tobytes(), (cs.name, cap)
                print("symmap %s cap %d: %d frames, exact" % (cs.name, cap, frames))
            continue
        F, fmt = f["F"], f["fmt"]
        m, table, given, split = sm.table_of(f["table"])
        new = lambda: c.DemapNode(m, given, F).set_llr_scale(0.6).set_output_format(fmt)  # noqa: E731
        plain = make(new)
        for cap in gc.CAPS:
            frames = cs.size(cap)
            node = make(new, cap)
            name = node.kernel(frames)
            k = fields(name)
            held(cs, cap, k, k["items"], k["wg"] // 64 if fmt == "bits" else k["wg"])
            assert ("form=table" in name) == (split is None), name
            z = sm.demap_input(table, frames * F, F + cap)
            got = node.run(z)
            if fmt == "llr":
                assert sm.same_floats(got, sm.ref_llr_records(z, table, F, 0.6)), (cs.name, cap)
            else:
                assert got.tobytes() == sm.ref_bits_records(z, table, F).tobytes(), (cs.name, cap)
            assert plain.run(z).tobytes() == got.tobytes(), (cs.name, cap)
            print("symmap %s cap %d: %d frames, exact" % (cs.name, cap, frames))


# ---------------------------------------------------------------- OFDM
def ofdm(c):
    import ofdm_ref as r

    for cs in gc.cases_of("ofdm"):
        f, mod = gc.OFDM_FORMATS[cs.fmt["format"]], cs.fmt["direction"] == "mod"
        args, kw = f.node_args()
        new = lambda: (c.OfdmModNode if mod else c.OfdmDemodNode)(*args, **kw)  # noqa: E731
        plain = make(new)
        for cap in gc.CAPS:
            frames = cs.size(cap)
            node = make(new, cap)
            k = fields(node.kernel(frames))
            held(cs, cap, k, k["items"], 1)
            z = r.data_values(f, frames)
            if mod:
                x, want, per, bound = z, r.ref_mod(f, z), f.sym_len, r.FFT_BOUND
            elif cs.fmt["format"] in gc.OFDM_TRAINING:      # training symbols that all differ
                x = r.training_case(gc.OFDM_TRAINING[cs.fmt["format"]], frames, cpe=True, rotate=True)[2]
                want, per, bound = r.ref_demod(f, x), f.D, r.TRAINING_BOUND
            else:
                x = r.through_channel(f, r.ref_mod(f, z), r.symbol_thetas(f))
                want, per, bound = r.ref_demod(f, x), f.D, r.CHANNEL_BOUND
            got = node.run(x)
            err = float(r.symbol_errors(got, want, per).max())
            print("ofdm %s cap %d: %d frames, %d items, worst symbol off by %.3e (bound %.3e)" % (cs.name, cap, frames, k["items"], err, bound))
            assert err <= bound, (cs.name, cap, err)
            assert plain.run(x).tobytes() == got.tobytes(), (cs.name, cap)


CHILDREN = dict(syncest=syncest, demod=demod, framesync=framesync, symsync=symsync, resample=resample, channelizer=channelizer, deframe=deframe,
                convcode=convcode, ratematch=ratematch, crc=crc, symmap=symmap, ofdm=ofdm)

if __name__ == "__main__":
    import comms_rs_amd

    assert comms_rs_amd.device_count() >= 1, "no MI355X visible"
    assert os.environ.get("COMMS_HIP_LIB", "").endswith("libcomms_hip_diag.so"), "the knob exists in the diagnostic build only"
    os.environ.pop(KNOB, None)
    CHILDREN[sys.argv[1]](comms_rs_amd)
    print("ok")
