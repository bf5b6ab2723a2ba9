"""CPU checks of tests/rx_ref.py, the reference the GPU receive tests compare against: it inverts tests/tx_ref.py's
mapping on exact constellation points, and its ties, signed zeros, NaN and Inf follow the rule of include/comms_hip.h."""
import numpy as np
import pytest

import rx_ref as r
import tx_ref as t


@pytest.mark.parametrize("name", sorted(r.TABLES))
@pytest.mark.parametrize("n_sym", [1, 7, 8, 9, 63, 64, 65, 1000])
def test_inverts_tx_mapping(name, n_sym):
    k, table = r.TABLES[name]
    rng = np.random.default_rng(n_sym)
    packed = t.pack(rng.integers(0, 2, n_sym * k))
    sym = t.map_bits(packed, n_sym, k, table)
    assert np.array_equal(r.sym_to_bits(sym, k, table), packed)
    # ... at any positive amplitude, for these tables
    for amp in (1e-3, 0.37, 3.0, 1e4):
        assert np.array_equal(r.sym_to_bits(sym * np.float32(amp), k, table), packed), amp


def test_default_tables_are_digital_rs():
    assert np.array_equal(r.default_table(1), np.array([t.BPSK[0, 0], t.BPSK[1, 0]], np.complex64))
    assert np.array_equal(r.default_table(2), (t.QPSK[:, 0] + 1j * t.QPSK[:, 1]).astype(np.complex64))


def test_pack_tail_bits_are_zero():
    assert r.pack([1], 1).tolist() == [1]
    assert r.pack([3, 3, 3], 2).tolist() == [0x3F]
    assert r.pack(np.ones(9, np.int64), 1).tolist() == [0xFF, 0x01]


def test_ties_go_to_the_lowest_index():
    # BPSK: the decision line re = 0, at any imaginary part
    y = np.array([0, 1j, -1j, 5j], np.complex64)
    assert r.decide(y, r.BPSK_DEF).tolist() == [0, 0, 0, 0]
    assert r.decide(y, r.BPSK_EX).tolist() == [0, 0, 0, 0]
    # QPSK: on one axis's line the other axis decides; the origin ties all four points
    q = np.array([0, 0.5j, -0.5j, 0.5, -0.5], np.complex64)
    assert r.decide(q, r.QPSK_DEF).tolist() == [0, 0, 2, 0, 1]
    assert r.decide(q, r.QPSK_EX).tolist() == [0, 2, 0, 1, 0]
    # a table with a repeated point: the first copy
    assert r.decide(np.array([2 + 0j], np.complex64), np.array([1, 1, -1, -1], np.complex64)).tolist() == [0]


def test_signed_zero_and_tiny_values():
    y = np.array([complex(-0.0, 0.0), complex(0.0, -0.0), complex(-0.0, -0.0)], np.complex64)
    assert r.decide(y, r.BPSK_DEF).tolist() == [0, 0, 0]
    assert r.decide(y, r.QPSK_DEF).tolist() == [0, 0, 0]
    # subnormal and tiny components: 1 -+ y rounds to 1 in f32, so the distances tie and index 0 wins
    tiny = np.array([-1e-45, -1e-40, -2.0 ** -26, -2.0 ** -20], np.float32).astype(np.complex64)
    assert r.decide(tiny, r.BPSK_DEF).tolist() == [0, 0, 0, 1]


def test_nan_and_inf():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    y = np.array([complex(nan, 0), complex(0, nan), complex(-1, nan), complex(inf, 0), complex(-inf, 0),
                  complex(-1, inf), complex(-3e38, 0)], np.complex64)
    # NaN: every distance NaN -> 0; an infinite component: both distances +Inf -> a tie -> 0; -3e38: the squares overflow
    assert r.decide(y, r.BPSK_DEF).tolist() == [0, 0, 0, 0, 0, 0, 0]
    assert r.decide(y, r.QPSK_DEF).tolist() == [0, 0, 0, 0, 0, 0, 0]
    # large but with y -+ 1 still apart in f32: the sign; beyond about 2^24, y -+ 1 round to the same value: a tie
    assert r.decide(np.array([-1e5, 1e5j - 1e5], np.complex64), r.QPSK_DEF).tolist() == [1, 1]
    assert r.decide(np.array([-1e18, 1e18j - 1e18], np.complex64), r.QPSK_DEF).tolist() == [0, 0]


def test_bit_errors_ref():
    a = np.array([0xFF, 0x0F], np.uint8)
    b = np.array([0x00, 0xFF], np.uint8)
    assert r.bit_errors(a, b, 16) == 12
    assert r.bit_errors(a, b, 12) == 8
    assert r.bit_errors(a, b, 3) == 3
