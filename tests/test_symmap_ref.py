"""The symbol mapper's and soft demapper's reference (tests/symmap_ref.py) held to its own claims, the host-side tables of the
library against it, the per-axis identities the demapper's second kernel form rests on against the brute-force definition on
the adversarial input set, and the argument refusals of both creates (which never reach a device).  No GPU."""
import ctypes as C

import numpy as np
import pytest

import symmap_ref as sr

N_ADVERSARIAL = 200_000


@pytest.fixture(scope="module")
def c():
    import comms_rs_amd as c

    return c


# ------------------------------------------------------------------ tables
def test_reference_tables_are_gray_and_start_from_digital_rs():
    assert np.array_equal(sr.qam_table(1), sr.BPSK) and np.array_equal(sr.qam_table(2), sr.QPSK)
    assert np.array_equal(sr.psk_table(1), sr.BPSK)                           # imaginary part exactly 0
    assert np.array_equal(sr.psk_table(2, np.sqrt(2.0)), sr.QPSK)
    for m in (2, 4, 6, 8):
        t = sr.qam_table(m)
        assert sr.nearest_neighbours_differ_in_one_bit(t) and len(set(t.tolist())) == 1 << m
        k = m // 2
        assert t[0] == (2 ** k - 1) * (1 + 1j) and set(t.real.tolist()) == set(range(-(2 ** k - 1), 2 ** k, 2))
    for m in (1, 2, 3, 4):
        t = sr.psk_table(m, 3.0)
        assert sr.nearest_neighbours_differ_in_one_bit(t) and len(set(t.tolist())) == 1 << m
        assert np.max(np.abs(np.abs(t.astype(np.complex128)) - 3.0)) < 3e-7
        assert set((-t).tolist()) == set(t.tolist())                           # exactly symmetric
    assert sr.qam_table(4, 0.25)[5] == np.complex64(0.25 * (1 + 1j))           # value 5 = 01 | 01: rank 1 on both axes


def test_library_tables_equal_the_reference(c):
    for m in (1, 2, 4, 6, 8):
        for scale in (1.0, 0.5, 1 / np.sqrt(10.0), 3.7e-3):
            assert c.qam_table(m, scale).tobytes() == sr.qam_table(m, scale).tobytes(), (m, scale)
    for m in (1, 2, 3, 4):
        for scale in (1.0, np.sqrt(2.0), 0.123):
            assert c.psk_table(m, scale).tobytes() == sr.psk_table(m, scale).tobytes(), (m, scale)
    assert c.psk_table(2, np.sqrt(2.0)).tobytes() == sr.QPSK.tobytes()
    for fn, bad in ((c.qam_table, (0, 3, 5, 7, 9, -1)), (c.psk_table, (0, 5, 8, -1))):
        for m in bad:
            with pytest.raises(c.CommsError) as e:
                fn(m)
            assert e.value.code == c.COMMS_ERR_ARG
        with pytest.raises(c.CommsError):
            fn(2, float("nan"))
    assert c.lib().comms_constellation_qam(2, 1.0, None) == c.COMMS_ERR_ARG


def test_the_splits_the_tests_expect_are_the_contracts():
    for name, (m, table, split) in sr.tables().items():
        m, full, _, _ = sr.table_of(name)
        got = sr.find_split(full)
        if split is None:
            assert got is None, name
        else:
            assert got is not None and (got[0], m - got[0]) == split, (name, got)
            assert np.array_equal(sr.separable_table(got[1], got[2]), full)


# ------------------------------------------------------------------ the mapper's reference
def test_ref_map_is_the_definition_bit_by_bit():
    rng = np.random.default_rng(1)
    for m, E in ((3, 10), (5, 33), (8, 7), (1, 5)):
        table = sr.random_table(m, m)
        bits = rng.integers(0, 2, (3, E), dtype=np.uint8)
        word = np.array([1 + 2j, -3j], np.complex64)
        got = sr.ref_map(bits, m, table, word, 2)
        F = -(-E // m)
        assert got.shape == (3, 2 + F + 2) and np.all(got[:, :2] == word) and np.all(got[:, 2 + F:] == 0)
        for f in range(3):
            for j in range(F):
                v = sum(int(bits[f, j * m + b]) << b for b in range(m) if j * m + b < E)
                assert got[f, 2 + j] == table[v]
    dirty = sr.dirty_records(bits, 5)
    assert np.array_equal(sr.unpack_records(dirty, 5), bits) and dirty.shape == (3, 4)
    assert np.unpackbits(dirty, axis=1, bitorder="little")[:, 5:].sum() > 40


# ------------------------------------------------------------------ the demapper's reference
def test_reference_at_two_bits_is_the_deframers_rule():
    """With digital.rs's QPSK table the LLRs are (4 s z.re, 4 s z.im) up to rounding, and the index is the sign pair."""
    z = sr.noisy_points(sr.QPSK, 500, 1, sigma=0.5)
    llr = sr.ref_llr(z, sr.QPSK, 0.75)
    assert np.max(np.abs(llr[:, 0] - 3.0 * z.real)) < 1e-5 and np.max(np.abs(llr[:, 1] - 3.0 * z.imag)) < 1e-5
    assert np.array_equal(sr.ref_index(z, sr.QPSK), (z.real < 0) | ((z.imag < 0) << 1))
    nan = np.array([complex(np.nan, 1), complex(1, np.nan), complex(np.inf, 0)], np.complex64)
    assert sr.ref_index(nan, sr.QPSK).tolist()[:2] == [0, 0] and np.all(np.isnan(sr.ref_llr(nan, sr.QPSK)[:2]))
    assert sr.same_floats(np.array([np.nan, 1.0], np.float32), np.array([-np.nan, 1.0], np.float32))
    assert not sr.same_floats(np.array([0.0], np.float32), np.array([-0.0], np.float32))


def test_llr_signs_agree_with_the_hard_decision():
    for name in ("8psk", "64qam", "rand5", "sep32"):
        m, table, _, _ = sr.table_of(name)
        z = sr.demap_input(table, 4000, 9)
        llr, v = sr.ref_llr(z, table), sr.ref_index(z, table)
        bit = (v[:, None] >> np.arange(m)) & 1
        assert np.all(bit[llr > 0] == 0) and np.all(bit[llr < 0] == 1), name


def test_a_distance_is_nan_for_one_point_only_if_for_all():
    """What lets the table form use an IEEE minimum in place of the strict-replace scan."""
    for name in ("8psk", "256qam", "rand8"):
        _, table, _, _ = sr.table_of(name)
        d = sr.distances(sr.adversarial(table, 20000, 4), table)
        nan = np.isnan(d)
        assert np.all(nan.any(axis=1) == nan.all(axis=1)) and nan.any() and np.isinf(d).any()
        with np.errstate(all="ignore"):
            assert sr.same_floats(np.fmin.reduce(d, axis=1), sr._scan_min(d)[0])


SPLITS = [(1, 1), (2, 2), (3, 3), (4, 4), (2, 3), (0, 3), (3, 0), (3, 2)]


def _split_table(mI, mQ):
    if (mI, mQ) == (3, 2):                                                     # random levels, not Gray
        rng = np.random.default_rng(32)
        return sr.separable_table(rng.normal(size=8), rng.normal(size=4))
    if mI == mQ:
        return sr.qam_table(2 * mI, 1.0 if mI < 4 else 1 / 16.0)
    gray = lambda k: [float((1 << k) - 1 - 2 * sr.gray_rank(g)) for g in range(1 << k)]  # noqa: E731
    return sr.separable_table(gray(mI), gray(mQ))


@pytest.mark.parametrize("mI,mQ", SPLITS)
def test_per_axis_identities_equal_the_brute_force_on_the_adversarial_set(mI, mQ):
    table = _split_table(mI, mQ)
    z = sr.adversarial(table, N_ADVERSARIAL, 100 * mI + mQ)
    assert np.isnan(z.real).any() and np.isinf(z.imag).any() and (np.abs(z) > 1e6).any() and (np.abs(z) < 1e-6).any()
    pI, pQ = table.real[: 1 << mI].copy(), table.imag[np.arange(1 << mQ) << mI].copy()
    assert np.array_equal(sr.separable_table(pI, pQ), table)
    assert sr.same_floats(sr.axis_llr(z, mI, pI, pQ, 0.37), sr.ref_llr(z, table, 0.37))
    want = sr.ref_index(z, table)
    assert np.array_equal(sr.axis_index(z, mI, pI, pQ), want)
    if mI and mQ:
        wrong = int(np.count_nonzero(sr.naive_axis_index(z, mI, pI, pQ) != want))
        print("split (%d,%d): the naive per-axis argmin differs in %d of %d" % (mI, mQ, wrong, z.size))
        assert wrong > 0, "the adversarial set no longer catches a naive per-axis argmin"


# ------------------------------------------------------------------ refusals, on the CPU
def test_creates_refuse_bad_arguments_before_the_device(c):
    lib = c.lib()
    pts = np.zeros(256, np.complex64)
    pts[:] = np.arange(256) + 1j
    p = pts.ctypes.data_as(C.c_void_p)
    nan8 = pts[:8].copy()
    nan8[5] = complex(1.0, np.nan)
    inf8 = pts[:8].copy()
    inf8[7] = complex(-np.inf, 0.0)
    word = np.ones(513, np.complex64).ctypes.data_as(C.c_void_p)
    # (m, table, E, word, P, G)
    bad_map = [(0, p, 8, None, 0, 0), (9, p, 8, None, 0, 0), (-1, p, 8, None, 0, 0), (3, None, 8, None, 0, 0),
               (3, nan8.ctypes.data_as(C.c_void_p), 8, None, 0, 0), (3, inf8.ctypes.data_as(C.c_void_p), 8, None, 0, 0),
               (4, p, 0, None, 0, 0), (4, p, (1 << 20) + 1, None, 0, 0), (4, p, 8, word, 513, 0), (4, p, 8, None, 1, 0),
               (4, p, 8, None, 0, (1 << 16) + 1)]
    for args in bad_map:
        h = C.c_void_p(0xDEAD)
        assert lib.comms_symmap_create(*args, 0, C.byref(h)) == c.COMMS_ERR_ARG, args
        assert not h.value
    assert lib.comms_symmap_create(4, p, 8, None, 0, 0, 0, None) == c.COMMS_ERR_ARG
    # (m, table, F, flags)
    bad_demap = [(0, p, 8, 0), (9, p, 8, 0), (3, None, 8, 0), (3, nan8.ctypes.data_as(C.c_void_p), 8, 0), (4, p, 0, 0),
                 (4, p, (1 << 20) + 1, 0), (4, p, 8, 2), (4, p, 8, 3), (4, p, 8, -1)]
    for args in bad_demap:
        h = C.c_void_p(0xDEAD)
        assert lib.comms_demap_create(*args, 0, C.byref(h)) == c.COMMS_ERR_ARG, args
        assert not h.value
    assert "COMMS_DEMAP_TABLE" in lib.comms_last_error().decode()
    assert lib.comms_demap_create(4, p, 8, 0, 0, None) == c.COMMS_ERR_ARG
    for fn in (lib.comms_symmap_in_frame_bytes, lib.comms_symmap_out_frame_syms, lib.comms_demap_in_frame_bytes, lib.comms_demap_out_frame_bytes):
        assert fn(None) == 0
    assert lib.comms_demap_set_output_format(None, c._lib.SYM_LLR) == c.COMMS_ERR_ARG
    assert lib.comms_demap_set_llr_scale(None, 1.0) == c.COMMS_ERR_ARG
    assert lib.comms_symmap_set_timer(None, None) == c.COMMS_ERR_ARG and lib.comms_demap_set_timer(None, None) == c.COMMS_ERR_ARG
    with pytest.raises(c.CommsError) as e:
        c.SymbolMapNode(3, None, 8)
    assert e.value.code == c.COMMS_ERR_ARG
    with pytest.raises(c.CommsError) as e:
        c.DemapNode(9, None, 8)
    assert e.value.code == c.COMMS_ERR_ARG
    with pytest.raises(ValueError):
        c.DemapNode(3, pts[:4], 8)


def test_demap_lengths_reach_the_word_seams():
    for m in range(1, 9):
        Fs = sr.demap_lengths(m)
        assert 1 in Fs and any(F * m % 32 for F in Fs) and any(F > 64 for F in Fs)
        rem = {F * m % 32 for F in Fs}
        assert any(r >= 32 - m for r in rem) and any(0 < r <= m for r in rem), (m, Fs)   # just below and just above a word


# ------------------------------------------------------------------ the coded link's noise level
def test_the_reference_chain_decodes_every_frame_at_the_links_noise_level():
    """The point of tests/test_gpu_symmap.py's coded link: with an ideal synchroniser (the gain and rotation divided out) the
    reference chain passes every frame's CRC at LINK_SIGMA, and raw symbol decisions at that level are not all right, so the
    decoder has work to do."""
    f = sr.link_format()
    assert f["E"] % sr.LINK_M != 0 and f["F"] * sr.LINK_M > f["E"]              # the last symbol carries padding bits
    payload, framed, coded, sent, sym = sr.link_transmit()
    assert sym.shape == (sr.LINK_FRAMES, f["rec"]) and 24 <= sr.LINK_FRAMES <= 60 and sr.LINK_T == 100
    y = sr.link_channel(sym).reshape(sr.LINK_FRAMES, -1)
    P = sr.LINK_WORD.size
    z = (y[:, P: P + f["F"]].astype(np.complex128) / sr.LINK_GAIN).astype(np.complex64)
    llr, words, decoded, (got, passed, crc) = sr.link_receive(z)
    assert passed.all() and np.array_equal(got, payload) and np.array_equal(decoded, framed)
    hard = sr.unpack_records(sr.ref_bits_records(z.ravel(), sr.qam_table(sr.LINK_M), f["F"]), f["E"])
    assert 0 < np.count_nonzero(hard != sent) < sent.size // 50
