"""The LDPC reference (tests/ldpc_ref.py) held to the header's definition, and the inputs of tests/test_gpu_ldpc.py held to
their conditions.  No GPU.

Facts about the definition recorded here (not about any kernel), BPSK over AWGN, 20 iterations at most, seeds as below:
  make_base(12, 24, 27) at Es/N0 = 1 dB:  64 of 64 frames decode;  make_base(4, 24, 81) at 5.5 dB:  64 of 64 frames decode."""
import numpy as np
import pytest

import ldpc_ref as lr

ENCODER_FORMATS = [n for n, f in lr.FORMATS.items() if f.encoder]


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
