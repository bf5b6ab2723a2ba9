"""The reference of the convolutional code (tests/viterbi_ref.py) checked against what does not depend on it: the known
impulse response, brute force over every codeword, the code's free distance, the quantiser's corner values -- and the noisy
point the GPU loop test runs at, pinned with tests/noise_ref.py's model of the generator.  No GPU."""
import hashlib
import itertools

import numpy as np
import pytest

import viterbi_ref as vr


def test_impulse_response_of_the_default_code():
    u = np.zeros((1, 7), np.uint8)
    u[0, 0] = 1
    coded = vr.ref_encode(u, 7, (0o171, 0o133), terminated=False).reshape(7, 2)
    assert coded[:, 0].tolist() == [1, 1, 1, 1, 0, 0, 1]
    assert coded[:, 1].tolist() == [1, 0, 1, 1, 0, 1, 1]
    # terminated: K - 1 more steps, which flush the register
    term = vr.ref_encode(u, 7, (0o171, 0o133), terminated=True)
    assert term.shape == (1, 2 * 13) and np.array_equal(term[0, :14], coded.reshape(-1)) and not np.any(term[0, 14:])


def test_encoder_is_the_register_of_the_header():
    """ref_encode (vectorised) against the register stepped bit by bit."""
    rng = np.random.default_rng(1)
    for (K, n), gens in vr.GENS.items():
        u = rng.integers(0, 2, (3, 41), dtype=np.uint8)
        for terminated in (True, False):
            got = vr.ref_encode(u, K, gens, terminated)
            for f in range(3):
                s, out = 0, []
                for b in list(u[f]) + [0] * (K - 1 if terminated else 0):
                    r = (int(b) << (K - 1)) | s
                    out += [bin(r & g).count("1") & 1 for g in gens]
                    s = r >> 1
                assert got[f].tolist() == out, (K, n, terminated)


@pytest.mark.parametrize("terminated", [True, False])
@pytest.mark.parametrize("K,n", sorted(vr.GENS))
def test_round_trip_without_noise(K, n, terminated):
    gens = vr.GENS[(K, n)]
    rng = np.random.default_rng(K * 10 + n)
    for T in (1, 2, K, 33, 200):
        u = rng.integers(0, 2, (4, T), dtype=np.uint8)
        coded = vr.ref_encode(u, K, gens, terminated)
        q = vr.ref_quantise(9.0 * (1.0 - 2.0 * coded.astype(np.float32)))
        bits, metric = vr.ref_decode(q, K, gens, T, terminated)
        assert np.array_equal(bits, u), (K, n, terminated, T)
        assert np.all(metric == 9 * coded.shape[1])                      # every coded bit agrees


@pytest.mark.parametrize("terminated", [True, False])
@pytest.mark.parametrize("n", [2, 3])
def test_final_metric_is_the_maximum_over_all_codewords(n, terminated):
    K, gens = 3, vr.GENS[(3, n)]
    rng = np.random.default_rng(5 + n)
    for T in range(1, 9):
        steps = vr.n_steps(T, K, terminated)
        for _ in range(6):
            q = rng.integers(-127, 128, n * steps)
            bits, metric = vr.ref_decode(q[None, :], K, gens, T, terminated)
            best, words = vr.brute_force_metric(q, K, gens, T, terminated)
            assert int(metric[0]) == best, (n, terminated, T)
            assert any(np.array_equal(bits[0], w) for w in words), (n, terminated, T)


def test_four_sign_flips_always_decode_at_K7():
    """d_free = 10 for (171, 133): any 4 flipped coded bits of equal magnitude leave the sent word strictly the best."""
    K, gens, T = 7, vr.GENS[(7, 2)], 48
    rng = np.random.default_rng(7)
    patterns = 300
    u = rng.integers(0, 2, (patterns, T), dtype=np.uint8)
    coded = vr.ref_encode(u, K, gens, True)
    llr = 10.0 * (1.0 - 2.0 * coded.astype(np.float32))
    for f in range(patterns):
        at = rng.choice(coded.shape[1], 4, replace=False) if f % 3 else rng.integers(0, coded.shape[1] - 4) + np.arange(4)   # scattered, and bursts
        llr[f, at] *= -1
    bits, metric = vr.ref_decode(vr.ref_quantise(llr), K, gens, T, True)
    assert np.array_equal(bits, u)
    assert np.all(metric == 10 * (coded.shape[1] - 8))


def test_quantiser_corner_values():
    f = np.float32
    x = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 0.5, 1.5, 2.5, -0.5, -1.5, 126.5, 127.5, -127.5, 127.49, 1e30, -3e38], f)
    assert vr.ref_quantise(x).tolist() == [0, 127, -127, 0, 0, 0, 2, 2, 0, -2, 126, 127, -127, 127, 127, -127]
    for qs in (0.25, 8.0, -3.0):
        edge = np.array([127.5 / qs, -127.5 / qs, 127.0 / qs, 0.5 / qs, 1.5 / qs], f)
        want = np.clip(np.rint(edge * f(qs)), -127, 127).astype(int).tolist()
        assert vr.ref_quantise(edge, qs).tolist() == want and abs(want[0]) == 127
    assert vr.ref_quantise(np.array([np.inf], f), 0.0).tolist() == [0]     # inf * 0 is NaN: an erasure
    assert vr.ref_quantise(np.array([3e38], f), 3e38).tolist() == [127]    # the product overflows to inf


def test_ties_and_erasures():
    """All-zero LLRs: every comparison is a tie, b = 0 everywhere; the decoder returns zeros and metric 0."""
    for (K, n), gens in vr.GENS.items():
        for terminated in (True, False):
            steps = vr.n_steps(20, K, terminated)
            bits, metric = vr.ref_decode(np.zeros((2, n * steps), np.int32), K, gens, 20, terminated)
            assert not np.any(bits) and not np.any(metric)


def test_record_size_helpers():
    assert [vr.record_bytes(b) for b in (1, 8, 9, 32, 33, 64, 65, 524)] == [4, 4, 4, 4, 8, 8, 12, 68]
    assert vr.n_steps(256, 7, True) == 262 and vr.n_steps(256, 7, False) == 256
    bits = np.random.default_rng(3).integers(0, 2, (5, 77), dtype=np.uint8)
    rec = vr.pack_records(bits)
    assert rec.shape == (5, 12) and np.array_equal(vr.unpack_records(rec, 77), bits)
    assert not np.any(rec[:, 10:]) and not np.any(np.unpackbits(rec, axis=1, bitorder="little")[:, 77:])
    assert rec[0, 0] & 1 == bits[0, 0]                                      # LSB first
    assert vr.LOOP_SYMS == 272 and vr.LOOP_F * 2 == vr.LOOP_CODED == vr.LOOP_N * vr.LOOP_STEPS


def test_shared_cases_are_what_the_gpu_tests_assume():
    for K in (3, 4, 5, 6, 7):
        counts = vr.step_counts(K)
        assert {1, 2, K - 1, K, 63, 64, 65, 127, 128, 129, 1000, vr.LDS_STEPS, vr.LDS_STEPS + 1} == set(counts)
    # the noisy input is noisy enough that the decoder itself errs: the GPU is compared with ref_decode, not with the sent bits
    cs = vr.make_case(7, 2, True, 1000, 3, "noisy")
    sent, llr, bits, _ = vr.case_data(cs)
    assert np.count_nonzero(bits != sent) > 0
    cs = vr.make_case(5, 3, False, 129, 2, "wide")
    _, llr, _, _ = vr.case_data(cs)
    assert llr.shape[1] > cs.n * cs.steps and np.all(np.isnan(llr[:, cs.n * cs.steps:]))


def test_the_noisy_point_of_the_device_loop():
    """At LOOP_SEED and LOOP_ESN0_DB the channel makes hard-decision errors in the coded bits and the decoder removes all of
    them -- with the generator's model; the GPU test asserts the same on the LLRs the device produced."""
    sent, llr = vr.loop_model()
    coded = vr.ref_encode(sent, vr.LOOP_K, vr.LOOP_GENS, True)
    hard = (llr < 0).astype(np.uint8)
    raw = int(np.count_nonzero(hard != coded))
    bits, _ = vr.ref_decode(vr.ref_quantise(llr, vr.LOOP_QSCALE), vr.LOOP_K, vr.LOOP_GENS, vr.LOOP_T, True)
    print("Es/N0 %.1f dB, sigma %.4f: %d raw errors of %d coded bits, %d decoded errors of %d"
          % (vr.LOOP_ESN0_DB, vr.LOOP_SIGMA, raw, coded.size, int(np.count_nonzero(bits != sent)), sent.size))
    assert raw > 0.01 * coded.size                                         # every frame's hard decisions are wrong somewhere
    assert all(np.any(hard[f] != coded[f]) for f in range(vr.LOOP_FRAMES))
    assert np.array_equal(bits, sent)
    assert np.count_nonzero(np.abs(np.rint(llr * np.float32(vr.LOOP_QSCALE))) > 127) < 0.01 * llr.size   # the clamp is rare


# ------------------------------------------------------------------ generators off the one set per (K, n) (vr.GEN_CORNERS)
ALL_SETS = [(K, n, name, gens) for (K, n), sets in sorted(vr.GEN_CORNERS.items()) for name, gens in sets]


def test_generator_corners_are_what_they_are_named():
    assert sorted(vr.GEN_CORNERS) == [(K, n) for K in range(3, 8) for n in (2, 3)]
    for (K, n), sets in vr.GEN_CORNERS.items():
        top, ones = 1 << (K - 1), (1 << K) - 1
        by = dict(sets)
        assert len(by) == len(sets) == 7 and all(len(g) == n and all(0 < x <= ones for x in g) for g in by.values())
        assert not by["input_clear"][0] & top and all(x & top for x in by["input_clear"][1:])
        assert not by["oldest_clear"][0] & 1 and any(x & 1 for x in by["oldest_clear"][1:])
        assert not any(x & 1 for x in by["oldest_clear_all"])
        assert by["single_and_ones"][:2] == (top, ones) and all(bin(x).count("1") == 1 for x in by["single_and_ones"][2:])
        assert len(set(by["equal"])) == 1
        assert by["random0"] != by["random1"]
        # without the oldest bit in any generator the two branches into a state carry the same coded bits
        _, sign = vr.trellis(K, by["oldest_clear_all"])
        assert np.array_equal(sign[0], sign[1])
        _, sign = vr.trellis(K, vr.GENS[(K, n)])
        assert not np.array_equal(sign[0], sign[1])
    # the default argument is the table's set, and the seed of a case does not depend on the generators
    cs = vr.make_case(5, 2, True, 65, 3, "noisy")
    assert cs == vr.make_case(5, 2, True, 65, 3, "noisy", gens=vr.GENS[(5, 2)]) and cs.gens == vr.GENS[(5, 2)]
    other = vr.make_case(5, 2, True, 65, 3, "noisy", gens=(0o22, 0o34))
    assert np.array_equal(vr.case_input(cs)[0], vr.case_input(other)[0]) and not np.array_equal(vr.case_input(cs)[1], vr.case_input(other)[1])


def test_pinned_cases_are_unchanged():
    """sha256 over cases, sent bits, inputs, reference bits and metrics, taken before make_case and ref_decode gained arguments."""
    g = hashlib.sha256()
    for K, n, t, steps, frames, kind in ((7, 2, True, 300, 3, "noisy"), (5, 3, False, 129, 2, "wide"), (3, 2, False, 65, 3, "special"),
                                         (7, 3, True, 64, 1, "zeros")):
        cs = vr.make_case(K, n, t, steps, frames, kind)
        sent, llr, bits, metric = vr.case_data(cs)
        for part in (repr(tuple(cs)).encode(), sent.tobytes(), llr.tobytes(), bits.tobytes(), metric.tobytes()):
            g.update(part)
    assert g.hexdigest() == "c942a9931abfbe5efe1b2f8248dcdd3d09c3f64f086964d99a9c5239d7c76c84", g.hexdigest()


@pytest.mark.parametrize("K,n", sorted(vr.GEN_CORNERS))
def test_generator_corners_against_brute_force_and_the_register(K, n):
    """Every set, both endings, T <= 10: the final metric is the maximum over all codewords, the decoded word attains it, and
    the encoder is the register stepped bit by bit.  Inputs with few levels, so that many candidates tie."""
    rng = np.random.default_rng(100 * K + n)
    for name, gens in vr.GEN_CORNERS[(K, n)]:
        for terminated in (True, False):
            u = rng.integers(0, 2, (2, 23), dtype=np.uint8)
            got = vr.ref_encode(u, K, gens, terminated)
            for f in range(2):
                s, out = 0, []
                for b in list(u[f]) + [0] * (K - 1 if terminated else 0):
                    r = (int(b) << (K - 1)) | s
                    out += [bin(r & g).count("1") & 1 for g in gens]
                    s = r >> 1
                assert got[f].tolist() == out, (K, n, name, terminated)
            for T in (1, 2, 5, 10):
                steps = vr.n_steps(T, K, terminated)
                for levels in (128, 2):
                    q = rng.integers(-levels + 1, levels, n * steps)
                    bits, metric = vr.ref_decode(q[None, :], K, gens, T, terminated)
                    best, words = vr.brute_force_metric(q, K, gens, T, terminated)
                    assert int(metric[0]) == best, (K, n, name, terminated, T)
                    assert any(np.array_equal(bits[0], w) for w in words), (K, n, name, terminated, T)


@pytest.mark.parametrize("rule", vr.RULES)
def test_generator_corners_catch_the_tie_mutants(rule):
    """b = 1 on equal candidates, and the highest state among equal final metrics, made in copies of the reference: in every K
    some corner case of tests/test_gpu_viterbi.py changes bits or its metric."""
    for K in range(3, 8):
        caught = []
        for n in (2, 3):
            for name, gens in vr.GEN_CORNERS[(K, n)]:
                for terminated in (True, False):
                    for steps in (K, 65):
                        ref = vr.corner_data(K, n, gens, terminated, steps)
                        mut = vr.corner_data(K, n, gens, terminated, steps, (rule,))
                        caught += ["%d-%s-%s-%d-%s" % (n, name, "term" if terminated else "trunc", steps, cs.kind)
                                   for (cs, _, bits, metric), (_, _, mbits, mmetric) in zip(ref, mut)
                                   if not (np.array_equal(bits, mbits) and np.array_equal(metric, mmetric))]
        kinds = sorted({c.rsplit("-", 1)[1] for c in caught})
        print(rule, "K = %d: %d cases, kinds %s, e.g. %s" % (K, len(caught), kinds, caught[:3]))
        assert caught, (rule, K)
        assert any(c.endswith("zeros") for c in caught)
