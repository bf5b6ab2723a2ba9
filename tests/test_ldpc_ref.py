"""The LDPC reference (tests/ldpc_ref.py) held to the header's definition, and the inputs of tests/test_gpu_ldpc.py held to
their conditions.  No GPU.

Facts about the definition recorded here (not about any kernel), BPSK over AWGN, 20 iterations at most, seeds as below:
  make_base(12, 24, 27) at Es/N0 = 1 dB:  64 of 64 frames decode;  make_base(4, 24, 81) at 5.5 dB:  64 of 64 frames decode."""
import hashlib

import numpy as np
import pytest

import ldpc_ref as lr

ENCODER_FORMATS = [n for n, f in lr.FORMATS.items() if f.encoder]
# sha256 of the matrices of the formats A ... G and of the loop, and of every (format, kind)'s case, inputs, reference bits and
# statuses, taken before the builders and ref_decode gained their arguments
PINNED_BASES = "da248a6d3a2c9722baecff0c2bd56c2d42bf868d2e31918590f8e4f1f3a305aa"
PINNED_CASES = "d83251a386783310560f6d45809dae745de20f2f742011126afe74c9a7f7299c"


def scalar_decode(q, B, Z, max_iters, norm16):
    """The header's decoder, one frame, check by check and edge by edge: a second restatement."""
    B = np.asarray(B)
    mb, nb = B.shape
    P = [int(v) for v in q[: nb * Z]]
    rows = [[(j, int(B[i, j])) for j in range(nb) if B[i, j] >= 0] for i in range(mb)]
    R = {}
    for it in range(1, max_iters + 1):
        for i in range(mb):
            for z in range(Z):
                var = [j * Z + (z + b) % Z for j, b in rows[i]]
                Q = [P[v] - R.get((i, z, e), 0) for e, v in enumerate(var)]
                Qc = [max(-127, min(127, x)) for x in Q]
                mags = [abs(x) for x in Qc]
                m1 = min(mags)
                idx = mags.index(m1)
                m2 = min(m for e, m in enumerate(mags) if e != idx)
                par = 0
                for x in Qc:
                    par ^= x < 0
                for e, v in enumerate(var):
                    mag = (norm16 * (m2 if e == idx else m1)) >> 4
                    R[(i, z, e)] = -mag if par ^ (Qc[e] < 0) else mag
                    P[v] = Q[e] + R[(i, z, e)]
        x = [p < 0 for p in P]
        if all(sum(x[j * Z + (z + b) % Z] for j, b in rows[i]) % 2 == 0 for i in range(mb) for z in range(Z)):
            return np.array(x[: (nb - mb) * Z], np.uint8), it
    return np.array(x[: (nb - mb) * Z], np.uint8), -max_iters


@pytest.mark.parametrize("fmt", ENCODER_FORMATS + ["loop"])
def test_every_codeword_satisfies_the_dense_matrix(fmt):
    B, Z = (lr.loop_base(), lr.LOOP_Z) if fmt == "loop" else (lr.base_of(fmt), lr.FORMATS[fmt].Z)
    mb, nb = B.shape
    assert lr.encoder_structure(B) is not None
    u = np.random.default_rng(5).integers(0, 2, (4, (nb - mb) * Z), dtype=np.uint8)
    c = lr.ref_encode(u, B, Z)
    assert c.shape == (4, nb * Z) and np.array_equal(c[:, : u.shape[1]], u)               # systematic
    H = lr.dense_H(B, Z)
    assert not np.any((H.astype(np.int64) @ c.T.astype(np.int64)) & 1)
    assert np.any(c[:, u.shape[1]:])


@pytest.mark.parametrize("fmt", list(lr.FORMATS))
def test_edge_lists_are_the_rows_of_the_dense_matrix(fmt):
    f = lr.FORMATS[fmt]
    B = lr.base_of(fmt)
    H = lr.dense_H(B, f.Z)
    V = lr.variables(B, f.Z)
    assert H.shape == (f.mb * f.Z, f.nb * f.Z)
    for i, v in enumerate(V):
        assert 2 <= v.shape[0] <= lr.MAX_ROW
        assert all(np.all(np.diff(v[:, z] // f.Z) > 0) for z in range(f.Z))                # ascending columns
        for z in range(f.Z):
            assert np.array_equal(np.sort(v[:, z]), np.flatnonzero(H[i * f.Z + z]))
        assert np.unique(v).size == v.size                                                 # no variable twice in a block row
    if fmt == "E":
        assert max(v.shape[0] for v in V) == 32                                            # the sign-mask limit is met
    if fmt == "G":
        assert lr.encoder_structure(B) is None


def test_encoder_is_linear():
    B, Z = lr.base_of("B"), lr.FORMATS["B"].Z
    rng = np.random.default_rng(6)
    u, w = rng.integers(0, 2, (2, 3, 12 * Z), dtype=np.uint8)
    assert np.array_equal(lr.ref_encode(u ^ w, B, Z), lr.ref_encode(u, B, Z) ^ lr.ref_encode(w, B, Z))
    assert not np.any(lr.ref_encode(np.zeros((1, 12 * Z), np.uint8), B, Z))


@pytest.mark.parametrize("kind,qscale,max_iters,norm16", [("noisy", None, 20, 12), ("noisy", None, 2, 16), ("special", -2.5, 3, 12),
                                                          ("zeros", None, 20, 12)])
def test_vectorised_decoder_equals_the_scalar_restatement(kind, qscale, max_iters, norm16):
    cs = lr.make_case("A", kind, qscale=qscale, max_iters=max_iters, norm16=norm16)
    _, llr, bits, status = lr.case_data(cs)
    f = lr.FORMATS["A"]
    q = lr.ref_quantise(llr[:, : f.nb * f.Z], cs.qscale)
    for k in range(cs.frames):
        b, st = scalar_decode(q[k], lr.base_of("A"), f.Z, max_iters, norm16)
        assert st == status[k] and np.array_equal(b, bits[k]), (k, st, status[k])


def test_the_scalar_restatement_on_a_decoder_only_matrix():
    cs = lr.make_case("G", "noisy", frames=4, max_iters=5)
    _, llr, bits, status = lr.case_data(cs)
    f = lr.FORMATS["G"]
    q = lr.ref_quantise(llr[:, : f.nb * f.Z], cs.qscale)
    for k in range(cs.frames):
        b, st = scalar_decode(q[k], lr.base_of("G"), f.Z, 5, 12)
        assert st == status[k] and np.array_equal(b, bits[k])


@pytest.mark.parametrize("fmt", list(lr.FORMATS))
def test_all_ties_converge_at_once_to_zero_bits(fmt):
    _, llr, bits, status = lr.case_data(lr.make_case(fmt, "zeros"))
    assert not np.any(llr) and not np.any(bits) and np.all(status == 1)
    _, _, bits, status = lr.case_data(lr.make_case(fmt, "special", qscale=0.0))             # a zero scale is the same input
    assert not np.any(bits) and np.all(status == 1)


@pytest.mark.parametrize("fmt", list(lr.FORMATS))
def test_noisy_cases_meet_early_exits_late_exits_and_failures(fmt):
    """One launch holds frames that stop early, frames that stop late and -- with max_iters = 2 -- frames that fail.  Format F
    has two frames per call (its state is the largest): there the two statuses differ."""
    sent, llr, bits, status = lr.case_data(lr.make_case(fmt, "noisy"))
    _, _, _, status2 = lr.case_data(lr.make_case(fmt, "noisy", max_iters=2))
    print(fmt, sorted(set(status.tolist())), int(np.count_nonzero(status2 < 0)))
    assert len(set(status.tolist())) >= (2 if fmt == "F" else 3)
    assert np.any(status2 == -2)
    assert np.all((status2 == -2) | (status2 == status))                                   # a prefix of the same schedule
    if sent is not None:
        ok = status > 0
        assert np.any(np.all(bits[ok] == sent[ok], axis=1))                                # (short codes also converge to other codewords)
    _, wide, wbits, wstatus = lr.case_data(lr.make_case(fmt, "wide"))
    f = lr.FORMATS[fmt]
    assert wide.shape[1] == f.nb * f.Z + 37 and np.all(np.isnan(wide[:, f.nb * f.Z:]))


@pytest.mark.parametrize("fmt", list(lr.FORMATS))
def test_planted_errors_keep_the_stopping_test_busy(fmt):
    """With messages scaled by 1/16 a wrong bit at -127 survives every iteration: the reference never reports convergence for
    a frame with wrong bits, at any iteration limit, and does at once for the frame without.  At Z > 64 that includes the pairs
    whose unsatisfied checks sit 64 apart in every block row of their column (shown here on the dense matrix)."""
    f = lr.FORMATS[fmt]
    planted = lr.planted_bits(fmt)
    for max_iters in (1, 2, 20):
        _, llr, bits, status = lr.case_data(lr.make_case(fmt, "planted", max_iters=max_iters, norm16=1))
        assert llr.shape[0] == len(planted)
        for k, wrong in enumerate(planted):
            assert status[k] == (-max_iters if wrong else 1), (fmt, k, wrong, status[k])
            assert set(np.flatnonzero(bits[k]).tolist()) == {v for v in wrong if v < bits.shape[1]}
    _, _, bits, status = lr.case_data(lr.make_case(fmt, "planted"))                        # (at 0.75 most formats correct them)
    assert status[planted.index(())] == 1
    if f.Z > 64:
        H = lr.dense_H(lr.base_of(fmt), f.Z)
        paired = 0
        for wrong in planted:
            if len(wrong) == 2 and abs(wrong[0] - wrong[1]) == 64:
                x = np.zeros(H.shape[1], np.int64)
                x[list(wrong)] = 1
                bad = np.flatnonzero((H.astype(np.int64) @ x) & 1)
                rows = {}
                for chk in bad:
                    rows.setdefault(chk // f.Z, []).append(chk % f.Z)
                paired += all(len(z) == 2 and z[1] - z[0] == 64 for z in rows.values())
        assert paired >= 2, paired


def test_special_inputs_reach_the_clamp_and_the_erasure():
    cs = lr.make_case("B", "special", qscale=-2.5)
    _, llr, _, _ = lr.case_data(cs)
    q = lr.ref_quantise(llr, cs.qscale)
    assert np.any(np.isnan(llr)) and np.any(np.isinf(llr)) and {-127, 0, 127} <= set(np.unique(q).tolist())
    assert np.array_equal(lr.ref_quantise(np.array([0.5, 1.5, 2.5, -0.5, np.nan, np.inf, -np.inf], np.float32)), [0, 2, 2, 0, 0, 127, -127])


def test_the_loop_point_decodes_every_frame_from_raw_errors():
    sent, llr = lr.loop_model()
    coded = lr.ref_encode(sent, lr.loop_base(), lr.LOOP_Z)
    assert lr.LOOP_N % 32 == 0 and lr.LOOP_T % 32 == 0 and lr.LOOP_SYMS == lr.LOOP_N // 2
    raw = (llr < 0) != (coded == 1)
    bits, status = lr.ref_decode(lr.ref_quantise(llr, lr.LOOP_QSCALE), lr.loop_base(), lr.LOOP_Z, lr.LOOP_ITERS)
    print("Es/N0 %.1f dB: %d raw errors of %d, statuses %s" % (lr.LOOP_ESN0_DB, int(raw.sum()), raw.size, status.tolist()))
    assert np.all(raw.any(axis=1))
    assert np.all(status > 0) and np.array_equal(bits, sent)


@pytest.mark.parametrize("mb,nb,Z,esn0", [(12, 24, 27, 1.0), (4, 24, 81, 5.5)])
def test_the_definition_decodes(mb, nb, Z, esn0):
    """The two points the definition was accepted on: every one of 64 frames decodes within 20 iterations."""
    B = lr.make_base(mb, nb, Z, 3)
    rng = np.random.default_rng(4)
    u = rng.integers(0, 2, (64, (nb - mb) * Z), dtype=np.uint8)
    c = lr.ref_encode(u, B, Z)
    sigma2 = 0.5 / 10.0 ** (esn0 / 10.0)
    llr = (2.0 / sigma2 * ((1.0 - 2.0 * c) + np.sqrt(sigma2) * rng.standard_normal(c.shape))).astype(np.float32)
    bits, status = lr.ref_decode(lr.ref_quantise(llr, 4.0), B, Z, 20, 12)
    print(mb, nb, Z, esn0, sorted(set(status.tolist())))
    assert np.all(status > 0) and np.array_equal(bits, u)


# ------------------------------------------------------------------ the corner table (lr.CORNERS)
def properties_of(f, B):
    """Every property a corner format can be in the table for, recomputed from the matrix and the library's formulas."""
    deg = np.count_nonzero(B >= 0, axis=1)
    N, T = f.nb * f.Z, (f.nb - f.mb) * f.Z
    have = {"fpw=%d" % lr.frames_per_wg(f.mb, f.nb, f.Z), "Z=%d" % f.Z, "mb=%d" % f.mb, "nb=%d" % f.nb}
    have |= {"deg=%d" % d for d in (2, 32) if np.all(deg == d)}
    have |= {"Z>64"} if f.Z > 64 else set()
    have |= {"dec_second_round"} if lr.chunks(T) > 64 else set()
    have |= {"dec_partial_round"} if lr.chunks(T) > 64 and lr.chunks(T) % 64 else set()
    have |= {"dec_odd_words"} if lr.out_words(T) % 2 else set()
    have |= {"full_column"} if np.any(np.count_nonzero(B >= 0, axis=0) == f.mb) else set()
    if f.encoder:
        r, s, t = lr.encoder_structure(B)
        have |= {"r=1"} if r == 1 and f.mb >= 5 else set()
        have |= {"r=mb-2"} if r == f.mb - 2 and f.mb >= 5 else set()
        have |= {"s=0"} if s == 0 else set()
        have |= {"s=Z-1"} if s == f.Z - 1 else set()
        have |= {"t=0"} if t == 0 else set()
        have |= {"t=Z-1"} if t == f.Z - 1 else set()
        have |= {"enc_partial_round"} if 4097 <= N <= 8191 and lr.out_words(N) % 2 and lr.chunks(N) % 64 else set()
    return have


def test_corner_table_meets_its_properties():
    """Each corner format has the properties it is listed for, and the table as a whole has what the formats A ... G lack."""
    assert not set(lr.CORNERS) & set(lr.FORMATS)
    table = {}
    for name, f in lr.CORNERS.items():
        B = lr.base_of(name)
        deg = np.count_nonzero(B >= 0, axis=1)
        assert B.shape == (f.mb, f.nb) and B.min() >= -1 and B.max() < f.Z and deg.min() >= 2 and deg.max() <= lr.MAX_ROW
        assert (lr.encoder_structure(B) is not None) == f.encoder
        table[name] = properties_of(f, B)
        print(name, (f.mb, f.nb, f.Z), "frame_lds", lr.frame_lds(f.mb, f.nb, f.Z), "T", (f.nb - f.mb) * f.Z, "words", lr.out_words((f.nb - f.mb) * f.Z),
              "chunks", lr.chunks((f.nb - f.mb) * f.Z), sorted(f.props))
        assert set(f.props) <= table[name], (name, set(f.props) - table[name])
        frames = lr.NOISY[name][0]
        fpw = lr.frames_per_wg(f.mb, f.nb, f.Z)
        for n in (frames, len(lr.planted_bits(name))):                          # more than a workgroup holds, and no multiple of it
            assert n > fpw and n % fpw and (f.Z < 128 or n <= 12), (name, n, fpw)
        assert all(0 <= v < f.nb * f.Z for wrong in lr.planted_bits(name) for v in wrong)

    def some(*props, encoder=False):
        return any(set(props) <= have and lr.CORNERS[n].encoder == encoder for n, have in table.items())

    # the decoder's corners
    assert some("fpw=3", "dec_partial_round") and some("fpw=2") and some("fpw=4", "full_column", "mb=32")
    assert some("deg=32", "Z=65") and some("mb=1", "deg=32", "Z=127") and some("mb=1", "nb=2", "Z=2", "deg=2") and some("dec_odd_words")
    assert {lr.frames_per_wg(f.mb, f.nb, f.Z) for f in lr.FORMATS.values()} == {1, 4}       # what the formats A ... G leave
    # the encoder's
    assert some("r=1", encoder=True) and some("r=mb-2", encoder=True) and some("s=0", "t=Z-1", encoder=True) and some("s=Z-1", "t=0", encoder=True)
    assert some("Z=2", encoder=True) and some("Z=65", encoder=True) and some("enc_partial_round", encoder=True)
    # the figures the table was laid out on
    assert (lr.frames_per_wg(4, 64, 128), lr.chunks(60 * 128), lr.frames_per_wg(8, 64, 128), lr.chunks(56 * 128)) == (3, 120, 2, 112)
    assert (lr.frames_per_wg(32, 64, 128), lr.out_words(8 * 5080 // 8), lr.out_words(40 * 127)) == (1, 159, 159)
    assert set(lr.CORNER_NORMS.values()) == {5, 11} and lr.CORNERS[lr.CORNER_255].Z <= 8


def test_builders_take_what_they_drew():
    """The new arguments default to the draws: the formats A ... G and the loop's matrix are what they were."""
    for mb, nb, Z, seed in ((3, 5, 7, 11), (12, 24, 27, 12), (32, 64, 128, 16)):
        B = lr.make_base(mb, nb, Z, seed)
        r, s, t = lr.encoder_structure(B)
        assert np.array_equal(lr.make_base(mb, nb, Z, seed, r=r, s=s, t=t), B)
        other = lr.make_base(mb, nb, Z, seed, s=(s + 1) % Z)
        assert np.array_equal(other[:, : nb - mb], B[:, : nb - mb]) and lr.encoder_structure(other) == (r, (s + 1) % Z, t)
    digest = hashlib.sha256(b"".join(lr.base_of(n).tobytes() for n in lr.FORMATS) + lr.loop_base().tobytes()).hexdigest()
    assert digest == PINNED_BASES, digest
    g = hashlib.sha256()                                                        # every format and kind: inputs, bits, statuses
    for fmt in lr.FORMATS:
        for kind in lr.KINDS:
            cs = lr.make_case(fmt, kind, max_iters=2 if fmt == "F" else 20)
            _, llr, bits, status = lr.case_data(cs)
            for part in (repr(cs).encode(), llr.tobytes(), bits.tobytes(), status.tobytes(), repr(lr.planted_bits(fmt)).encode()):
                g.update(part)
    assert g.hexdigest() == PINNED_CASES, g.hexdigest()
    B = lr.random_base(5, 40, 9, 1, deg=[2, 32, 7, 2, 32], full=11)
    assert np.count_nonzero(B >= 0, axis=1).tolist() == [2, 32, 7, 2, 32] and np.all(B[:, 11] >= 0)


@pytest.mark.parametrize("fmt", list(lr.CORNERS))
def test_corner_codewords_and_edge_lists(fmt):
    f = lr.CORNERS[fmt]
    B = lr.base_of(fmt)
    H = lr.dense_H(B, f.Z)
    for i, v in enumerate(lr.variables(B, f.Z)):
        for z in range(f.Z):
            assert np.array_equal(np.sort(v[:, z]), np.flatnonzero(H[i * f.Z + z]))
    if f.encoder:
        u = np.random.default_rng(5).integers(0, 2, (3, (f.nb - f.mb) * f.Z), dtype=np.uint8)
        cw = lr.ref_encode(u, B, f.Z)
        assert not np.any((H.astype(np.int64) @ cw.T.astype(np.int64)) & 1) and np.array_equal(cw[:, : u.shape[1]], u)


@pytest.mark.parametrize("fmt", ["least", "encz2", "r1"])
def test_corner_decoder_equals_the_scalar_restatement(fmt):
    f = lr.CORNERS[fmt]
    for cs in (lr.make_case(fmt, "noisy", norm16=lr.CORNER_NORMS.get(fmt, 12)), lr.make_case(fmt, "planted", max_iters=3, norm16=1)):
        _, llr, bits, status = lr.case_data(cs)
        q = lr.ref_quantise(llr[:, : f.nb * f.Z], cs.qscale)
        for k in range(min(cs.frames, 5)):
            b, st = scalar_decode(q[k], lr.base_of(fmt), f.Z, cs.max_iters, cs.norm16)
            assert st == status[k] and np.array_equal(b, bits[k]), (fmt, k)


@pytest.mark.parametrize("fmt", list(lr.CORNERS))
def test_corner_noisy_cases_are_mixed(fmt):
    """A condition on the inputs, on the reference alone: at max_iters = 20 the frames of a corner format's noisy call take at
    least two statuses, one of them 2 or more, and -- from two block rows on -- one of them a failure.

    With ONE block row no status other than 1 and -max_iters exists, at any input: no variable is in two checks, so the second
    iteration's Q = P - R is the quantised input again, its messages and posteriors are the first iteration's, and a frame
    that has not converged after one iteration never does.  For the two formats with mb = 1 the call therefore holds both of
    these, a failure among them, and the test asserts that no third status occurs."""
    f = lr.CORNERS[fmt]
    _, _, _, status = lr.case_data(lr.make_case(fmt, "noisy"))
    _, _, _, status2 = lr.case_data(lr.make_case(fmt, "noisy", max_iters=2))
    print(fmt, status.tolist())
    seen = set(status.tolist())
    assert len(seen) >= 2
    if f.mb >= 2:
        assert max(seen) >= 2 and min(seen) == -20
    else:
        assert seen == {1, -20}
    assert np.all((status2 == -2) | (status2 == status))
    for kind in ("zeros", "special", "wide"):
        assert lr.make_case(fmt, kind).frames == lr.NOISY[fmt][0]


def test_the_255_iteration_case_never_clears():
    cs = lr.corner_cases(lr.CORNER_255, "planted")[-1]
    assert (cs.max_iters, cs.norm16) == (255, 1)
    _, _, bits, status = lr.case_data(cs)
    planted = lr.planted_bits(cs.fmt)
    print(planted, status.tolist())
    assert [s == -255 for s in status] == [bool(w) for w in planted] and np.count_nonzero(status == 1) == 1
    for k, wrong in enumerate(planted):
        assert set(np.flatnonzero(bits[k]).tolist()) == {v for v in wrong if v < bits.shape[1]}


def mutant_catches(rule, fmts):
    """[(case, frames that change)] over the max_iters = 20 cases of the formats: the reference under `rule` against itself."""
    caught = []
    for fmt in fmts:
        f = lr.CORNERS[fmt]
        for kind in lr.KINDS:
            for cs in lr.corner_cases(fmt, kind):
                if cs.max_iters != 20 or cs.norm16 == 16 or cs.qscale in (0.0, 0.03):
                    continue
                _, llr, bits, status = lr.case_data(cs)
                q = lr.ref_quantise(llr[:, : f.nb * f.Z], cs.qscale)
                mbits, mstatus = lr.ref_decode(q, lr.base_of(fmt), f.Z, cs.max_iters, cs.norm16, rules=(rule,))
                changed = np.flatnonzero(np.any(mbits != bits, axis=1) | (mstatus != status))
                if changed.size:
                    caught.append((cs, changed.tolist()))
    return caught


def test_corner_cases_catch_the_mutants():
    """Would the corner cases notice?  Mistakes a kernel could make, made in copies of the reference (ref_decode's rules=, the
    model of the packing, a shifted frame slot), each against the cases tests/test_gpu_ldpc.py runs; no library code is involved."""
    def names(caught):
        return sorted({"%s-%s(norm16=%d)" % (cs.fmt, cs.kind, cs.norm16) for cs, _ in caught})

    everything = list(lr.CORNERS)
    dense = [n for n in everything if "deg=32" in lr.CORNERS[n].props]
    tall = [n for n in everything if lr.CORNERS[n].Z > 64]
    for rule, fmts in (("idx_last", everything), ("no_clamp", everything), ("mask32", dense), ("xor_passes", tall)):
        caught = mutant_catches(rule, fmts)
        print(rule, "caught by", names(caught))
        if rule == "idx_last":
            # not a fault, at any input: two edges tie at the minimum only where m2 = m1, and then the message of the edge
            # called idx, (norm16 m2) >> 4, is every other edge's.  No case can see which of the tied edges idx names
            assert not caught
            continue
        assert caught, rule
        by_fmt = {cs.fmt for cs, _ in caught}
        if rule == "mask32":                                                # a full mask over two passes, and over one live lane
            assert {"fpw3", "z65", "mb1"} <= by_fmt
        if rule == "xor_passes":                                            # the lane-mate pairs, also at one live lane and at Z = 127
            planted = {cs.fmt for cs, _ in caught if cs.kind == "planted" and cs.norm16 == 1}
            assert {"z65", "mb1", "fpw3", "encz65", "enc5080"} <= planted, planted
        if rule == "no_clamp":                                              # the heaviest column leaves the clamp far behind
            assert "col32" in by_fmt
    # ld_pack: the model is the packing; with the first round's ballots in the second round's words the long records differ
    for fmt in everything:
        f = lr.CORNERS[fmt]
        T, N = (f.nb - f.mb) * f.Z, f.nb * f.Z
        seen = []
        for kind in lr.KINDS:
            _, _, bits, _ = lr.case_data(lr.make_case(fmt, kind, norm16=1 if kind == "planted" else 12))
            assert lr.pack_model(bits).tobytes() == lr.pack_records(bits).tobytes()
            if T > 4096:
                stale = lr.unpack_records(lr.pack_model(bits, stale=True).view(np.uint8), T)
                seen += [kind] * bool(np.any(stale != bits))
        if T > 4096:
            print("stale ballots in", fmt, "seen by", seen)
            assert len(seen) >= 3, (fmt, seen)
        if f.encoder:
            sent = np.random.default_rng(f.seed).integers(0, 2, (2, T), dtype=np.uint8)    # test_corner_encoder's draws
            coded = lr.ref_encode(sent, lr.base_of(fmt), f.Z)
            assert lr.pack_model(coded).tobytes() == lr.pack_records(coded).tobytes()
            if N > 4096:
                assert np.any(lr.unpack_records(lr.pack_model(coded, stale=True).view(np.uint8), N) != coded)
    # a wrong wave * frame_lds: frame k of a workgroup decoded from the LLRs of frame k - 1.  Every wave slot but the first
    # must hold, in some workgroup, a frame that does not decode as its neighbour does
    for fmt in everything:
        f = lr.CORNERS[fmt]
        fpw = lr.frames_per_wg(f.mb, f.nb, f.Z)
        for cs in (lr.make_case(fmt, "noisy"), lr.make_case(fmt, "planted", norm16=1)):
            _, _, bits, status = lr.case_data(cs)
            differs = np.any(bits[1:] != bits[:-1], axis=1) | (status[1:] != status[:-1])   # frame k against k - 1
            slots = {k % fpw for k in range(1, cs.frames) if differs[k - 1]}
            print("slot offset in %s-%s: %d of %d neighbours differ, wave slots %s" % (fmt, cs.kind, int(differs.sum()), differs.size, sorted(slots)))
            assert slots >= set(range(1, fpw)), (fmt, cs.kind, slots)
