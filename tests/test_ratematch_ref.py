"""The reference of the rate matching (tests/ratematch_ref.py) checked against what does not depend on it: the interleaver's
literal definition, the inverse property, the round trip through the Viterbi reference at every usual rate -- and the noisy
point the GPU loop test runs at, pinned with tests/noise_ref.py's model of the generator.  No GPU."""
import numpy as np
import pytest

import ratematch_ref as rr
import viterbi_ref as vr

RATES = [name for name in rr.PATTERNS if name != "none"]


def test_closed_form_interleaver_is_the_definition():
    for E in range(1, 71):
        for C in range(2, E + 1):
            want = rr.interleave_by_definition(E, C)
            assert np.array_equal(rr.interleave_closed_form(E, C), want), (E, C)
            assert np.array_equal(np.sort(want), np.arange(E))
    # a few by hand: 7 bits in 3 columns are the rows 012 / 345 / 6, read 0 3 6 1 4 2 5
    assert rr.interleave_closed_form(7, 3).tolist() == [0, 3, 6, 1, 4, 2, 5]
    assert rr.interleave_closed_form(6, 6).tolist() == list(range(6))          # one row
    assert rr.interleave_closed_form(6, 2).tolist() == [0, 2, 4, 1, 3, 5]


def test_patterns_have_their_rates():
    for name, kept, period in (("2/3", 3, 4), ("3/4", 4, 6), ("5/6", 6, 10), ("7/8", 8, 14)):
        p = rr.PATTERNS[name]
        assert len(p) == period and sum(p) == kept                              # period / 2 information bits in `kept` sent ones
        assert rr.n_tx_bits(10 * period, p) == 10 * kept
    assert rr.kept_positions(8, rr.PATTERNS["3/4"]).tolist() == [0, 1, 3, 4, 6, 7]
    assert rr.n_tx_bits(140, None) == 140 and rr.LOOP_E == 350 and rr.LOOP_RECORD == 44 and rr.LOOP_F * 2 == rr.LOOP_E


@pytest.mark.parametrize("name", list(rr.PATTERNS))
def test_inv_inverts_src_and_rx_undoes_tx(name):
    pattern = rr.PATTERNS[name]
    for N in rr.coded_lengths(pattern):
        E = rr.n_tx_bits(N, pattern)
        for j, (cols, perm) in enumerate(rr.interleavers(E, N)):
            src, inv = rr.build_map(N, pattern, cols, perm)
            assert src.size == E and np.array_equal(np.sort(src), rr.kept_positions(N, pattern))
            assert np.array_equal(inv[src], np.arange(E)) and np.count_nonzero(inv < 0) == N - E
            assert np.array_equal(src[inv[inv >= 0]], np.flatnonzero(inv >= 0))
            scr = rr.scramble_bits(E, N) if j % 2 else None
            bits = np.random.default_rng(N + j).integers(0, 2, (2, N), dtype=np.uint8)
            tx = rr.ref_tx(bits, src, scr)
            # the channel without noise: +1.0 for a 0, -1.0 for a 1; the dematched signs are the coded bits, erasures +0.0
            llr = (1.0 - 2.0 * tx).astype(np.float32)
            back = rr.ref_rx(llr.view(np.uint32), src, N, scr)
            kept = inv >= 0
            assert np.array_equal(back[:, kept] >> 31, bits[:, kept]) and not np.any(back[:, ~kept])
            assert np.all((back[:, kept] & 0x7FFFFFFF) == np.float32(1.0).view(np.uint32))


def test_special_values_pass_with_only_the_sign_changed():
    N, pattern = 140, rr.PATTERNS["3/4"]
    E = rr.n_tx_bits(N, pattern)
    src, inv = rr.build_map(N, pattern, 17)
    scr = rr.scramble_bits(E, 5)
    words = rr.llr_words(3, E + 9, E, 11)
    assert set(rr.SPECIAL.tolist()) <= set(words[:, :E].reshape(-1).tolist())
    out = rr.ref_rx(words, src, N, scr)
    assert np.array_equal(out[:, src] ^ (scr.astype(np.uint32) << 31), words[:, :E])
    assert not np.any(out[:, inv < 0])


@pytest.mark.parametrize("T", [1, 5, 64, 250, 1000])
@pytest.mark.parametrize("name", RATES)
def test_punctured_round_trip_without_noise(name, T):
    """encode -> map -> +-1 -> ref_rx -> quantise -> decode returns the sent bits at every usual rate, 17 columns."""
    pattern = rr.PATTERNS[name]
    sent = np.random.default_rng(T).integers(0, 2, (3, T), dtype=np.uint8)
    coded = vr.ref_encode(sent, 7, vr.GENS[(7, 2)], True)
    N = coded.shape[1]
    src, _ = rr.build_map(N, pattern, 17)
    scr = rr.scramble_bits(src.size, T)
    llr = (1.0 - 2.0 * rr.ref_tx(coded, src, scr)).astype(np.float32)
    dem = rr.ref_rx(llr.view(np.uint32), src, N, scr).view(np.float32)
    bits, _ = vr.ref_decode(vr.ref_quantise(dem, 8), 7, vr.GENS[(7, 2)], T, True)
    assert np.array_equal(bits, sent), (name, T, int(np.count_nonzero(bits != sent)))


def test_shared_cases_are_what_the_gpu_tests_assume():
    for name, pattern in rr.PATTERNS.items():
        lengths = rr.coded_lengths(pattern)
        assert {1, 14, 140, 2012} & set(lengths) >= ({14, 140, 2012} if pattern else {1, 14, 140, 2012})
        assert {rr.n_tx_bits(N, pattern) for N in lengths} >= {1, 31, 32, 33, 63, 64, 65}
        if pattern:
            assert sum(1 for N in lengths if pattern[(N - 1) % len(pattern)] == 0) >= 3        # last positions punctured
    assert rr.cols_of(65) == [0, 2, 5, 65] and rr.cols_of(33) == [0, 2, 3, 33] and rr.cols_of(1) == [0]
    for E in (31, 32, 33, 63, 64, 65, 105):
        rems = {C: E - (-(-E // C) - 1) * C for C in rr.cols_of(E) if C}
        assert 1 in rems.values() and rems[E] == E
        assert E == 31 or any(rem == C for C, rem in rems.items() if C < E)      # 31 is prime: only the one row is full
    assert rr.record_bytes(rr.LOOP_E) == 44 and rr.LOOP_SYMS == 176


def test_the_noisy_point_of_the_device_loop():
    """At LOOP_SEED and LOOP_ESN0_DB, rate 3/4 with 17 columns and the PRNS scramble: the channel makes hard-decision errors
    in every frame's transmitted bits and the decoder behind ref_rx removes all of them -- with the generator's model; the
    GPU test asserts the same on the LLRs the device produced."""
    sent, coded, llr, scr = rr.loop_model()
    src, inv = rr.build_map(rr.LOOP_CODED, rr.LOOP_PATTERN, rr.LOOP_COLS)
    tx = rr.ref_tx(coded, src, scr)
    hard = (llr < 0).astype(np.uint8)
    raw = np.count_nonzero(hard != tx, axis=1)
    dem = rr.ref_rx(llr.view(np.uint32), src, rr.LOOP_CODED, scr).view(np.float32)
    bits, _ = vr.ref_decode(vr.ref_quantise(dem, rr.LOOP_QSCALE), rr.LOOP_K, rr.LOOP_GENS, rr.LOOP_T, True)
    print("Es/N0 %.1f dB, sigma %.4f: raw errors per frame %s of %d transmitted bits, %d decoded errors of %d"
          % (rr.LOOP_ESN0_DB, rr.LOOP_SIGMA, raw.tolist(), rr.LOOP_E, int(np.count_nonzero(bits != sent)), sent.size))
    assert np.all(raw > 0) and raw.sum() > 0.01 * tx.size                   # every frame's hard decisions are wrong somewhere
    assert np.array_equal(bits, sent)
    assert not np.any(dem[:, inv < 0]) and np.count_nonzero(inv < 0) == rr.LOOP_CODED - rr.LOOP_E
    assert np.count_nonzero(np.abs(np.rint(llr * np.float32(rr.LOOP_QSCALE))) > 127) == 0     # nothing on the clamp
    # the hard decisions alone, descrambled and put back in place, are not the codeword of the sent bits
    assert all(np.any((dem[f] < 0)[inv >= 0] != (coded[f] == 1)[inv >= 0]) for f in range(rr.LOOP_FRAMES))
