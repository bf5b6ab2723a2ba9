"""CPU tests of the transmit front end's reference (tests/tx_ref.py) and of the new C ABI's argument rules that
hold without a GPU: PRNS create refusals, the modulators' None rule, no CPU fallback."""
import json
import os

import numpy as np
import pytest

import oracle
import tx_ref as t

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# maximal in this shift convention (found by the order test below; the GPU tests use it for skip(2^32 - 1))
MAX32 = 0xD04FBB5A
PRIMES_2_32_M1 = (3, 5, 17, 257, 65537)


@pytest.fixture(scope="module")
def dkats():
    with open(os.path.join(ROOT, "tests", "golden", "digital_kats.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def c():
    import __graft_entry__ as g

    g.build()
    import comms_rs_amd as c

    return c


# ------------------------------------------------------------------ PrnGen reference
def test_prns_reference_matches_the_oracle_at_8_bits():
    rng = np.random.default_rng(3)
    for _ in range(60):
        mask, state = int(rng.integers(0, 256)), int(rng.integers(0, 256))
        want, st = oracle.prns_u8(mask, state, 300)
        got, st2 = t.prns_serial(mask, state, 300, 8)
        assert np.array_equal(got, want) and st2 == int(st), (mask, state)


def test_prns_reference_known_answers(kats):
    k = kats["prbs7"]
    bits, _ = t.prns_serial(k["poly_mask"], k["state"], len(k["expected"]), 8)
    assert bits.tolist() == k["expected"]
    assert t.step(0xC0, 0xFF, 8)[0] == 1  # prns.rs:59-62 doctest
    k8 = kats["prns8"]
    seen, s = set(), k8["state"]
    for _ in range(k8["distinct_states"]):
        seen.add(s)
        s = t.step(k8["poly_mask"], s, 8)[1]
    assert len(seen) == k8["distinct_states"] and s == k8["state"]


@pytest.mark.parametrize("w", t.WIDTHS)
def test_jump_equals_serial_stepping(w):
    rng = np.random.default_rng(w)
    mask = int(rng.integers(0, 1 << 62)) & t.wmask(w) | (1 << (w - 1))
    state = int(rng.integers(1, 1 << 62)) & t.wmask(w)
    j = t.Jump(mask, w)
    for n in (0, 1, 2, 7, 63, 64, 65, 1000, 4097, 99999):
        _, s = t.prns_serial(mask, state, n, w)
        assert j.skip(state, n) == s, n
    for a, b in ((3, 5), (1000, 12345), (1 << 40, 77), ((1 << 63) + 5, (1 << 62) + 9)):
        assert j.skip(j.skip(state, a), b) == j.skip(state, a + b)


@pytest.mark.parametrize("w", t.WIDTHS)
def test_vectorised_reference_equals_serial(w):
    rng = np.random.default_rng(100 + w)
    mask = int(rng.integers(0, 1 << 62)) & t.wmask(w)
    state = int(rng.integers(1, 1 << 62)) & t.wmask(w)
    for n in (1, 7, 8, 63, 64, 65, 4095, 20000):
        bits, _ = t.prns_serial(mask, state, n, w)
        packed = t.prns_packed(mask, state, n, w, streams=37)
        assert packed.size == (n + 7) // 8
        assert np.array_equal(packed, t.pack(bits)), n


def test_a_maximal_32_bit_mask():
    assert t.is_maximal(MAX32, 32, PRIMES_2_32_M1)
    assert not t.is_maximal(0x80000001, 32, PRIMES_2_32_M1)
    j = t.Jump(MAX32, 32)
    assert j.skip(0x1234567, (1 << 32) - 1) == 0x1234567


# ------------------------------------------------------------------ digital.rs reference
def test_modulator_reference_on_the_known_answers(dkats):
    for v, want in dkats["bpsk_bit"]["cases"]:
        assert t.bpsk_bit_mod(v).tolist() == want
    for v, want in dkats["qpsk_bit"]["cases"]:
        assert t.qpsk_bit_mod(v).tolist() == want
    assert t.bpsk_bit_mod(2) is None and t.qpsk_bit_mod(4) is None
    for b, want in dkats["bpsk_byte"]["cases"]:
        assert t.bpsk_byte_mod([b]).tolist() == want
    for b, want in dkats["qpsk_byte"]["cases"]:
        assert t.qpsk_byte_mod([b]).tolist() == want


def test_bits_mapping_rule():
    # v = next k stream bits, first bit = LSB; packed LSB first
    packed = np.array([0b10110100], np.uint8)
    assert t.map_bits(packed, 8, 1, [0, 1]).real.tolist() == [0, 0, 1, 0, 1, 1, 0, 1]
    assert t.map_bits(packed, 4, 2, [0, 1, 2, 3]).real.tolist() == [0, 1, 3, 2]


# ------------------------------------------------------------------ C ABI without a GPU
def test_new_creates_fail_without_a_device(c):
    if c.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(c.CommsError) as e:
        c.PrnsNode(0xC0, 0x01)
    assert e.value.code == c.COMMS_ERR_DEVICE
    for fn in (c.bpsk_byte_mod, c.qpsk_byte_mod, c.bpsk_bit_mod, c.qpsk_bit_mod):
        with pytest.raises(c.CommsError) as e:
            fn(np.zeros(16, np.uint8))
        assert e.value.code == c.COMMS_ERR_DEVICE


@pytest.mark.parametrize("mask,state,width", [(0xC0, 1, 7), (0xC0, 1, 0), (0xC0, 1, 128), (0x1C0, 1, 8), (0xC0, 0x100, 8),
                                              (1 << 16, 1, 16), (1, 1 << 32, 32)])
def test_prns_create_refuses_bad_arguments(c, mask, state, width):
    with pytest.raises(c.CommsError) as e:
        c.PrnsNode(mask, state, width)
    assert e.value.code == c.COMMS_ERR_ARG


def test_bit_modulators_refuse_values_the_reference_maps_to_none(c):
    for fn, bad in ((c.bpsk_bit_mod, 2), (c.qpsk_bit_mod, 4), (c.qpsk_bit_mod, 255)):
        with pytest.raises(c.CommsError) as e:
            fn(np.array([0, 1, bad], np.uint8))
        assert e.value.code == c.COMMS_ERR_ARG and "None" in str(e.value)


def test_pulse_input_format_refuses_bad_arguments_on_a_null_handle(c):
    from comms_rs_amd._lib import lib

    assert lib().comms_pulse_set_input_format(None, 1, 1, None) == c.COMMS_ERR_ARG
