"""The reference of the frame check (tests/crc_ref.py) against what is known about CRCs independently of it: the catalogue's
check values, the residue property, error detection; and the conditions on the inputs that tests/test_gpu_crc.py relies on,
the noisy point of the device loop among them.  No GPU."""
import zlib

import numpy as np
import pytest

import crc_ref as cr
import ratematch_ref as rr


def reverse(v, W):
    return int(format(v, "0%db" % W)[::-1], 2)


@pytest.mark.parametrize("name", list(cr.CATALOGUE))
def test_catalogue_check_values(name):
    p, msb_first, crc, tail = cr.CATALOGUE[name]
    bits = cr.string_bits(cr.CHECK_STRING, msb_first)
    assert cr.crc_bits(bits, p) == crc
    assert int(cr.ref_crc(bits[None, :], p)[0]) == crc                      # the vectorised register is the same register
    if name in cr.REVERSED:
        assert reverse(crc, p.W) == cr.REVERSED[name]
    record = cr.pack_records(cr.ref_attach(bits[None, :], p))[0]
    assert record.size == cr.record_bytes(72 + p.W) and not record[(72 + p.W + 7) // 8:].any()
    if tail is not None:
        assert bytes(record[: 9 + len(tail)]) == cr.CHECK_STRING + tail
    if name == "CRC-32":                                                    # the Ethernet FCS: zlib's crc32, sent low byte first
        assert bytes(record[9:13]) == zlib.crc32(cr.CHECK_STRING).to_bytes(4, "little")
        data = bytes(np.random.default_rng(5).integers(0, 256, 333, dtype=np.uint8))
        rec = cr.pack_records(cr.ref_attach(cr.string_bits(data, False)[None, :], p))[0]
        assert bytes(rec[333:337]) == zlib.crc32(data).to_bytes(4, "little")


@pytest.mark.parametrize("name", list(cr.CATALOGUE))
def test_residue_is_one_constant_for_every_payload(name):
    """The register (xorout = 0) over payload + CRC does not depend on the payload: 0 where init = 0 and xorout = 0."""
    p = cr.CATALOGUE[name][0]
    rng = np.random.default_rng(p.W)
    residues = set()
    for T in (1, 7, 32, 100, 257):
        frame = cr.ref_attach(rng.integers(0, 2, (3, T), dtype=np.uint8), p)
        residues |= {cr.crc_bits(f, p, xorout=0) for f in frame}
    assert len(residues) == 1, residues
    want = {"CRC-32": 0xC704DD7B, "X-25": 0x1D0F}
    if name in want:
        assert residues == {want[name]}
    if p.init == 0 and p.xorout == 0:
        assert residues == {0}


def test_every_single_bit_flip_is_detected():
    for name in ("CRC-32", "X-25", "CRC24A", "CRC-8", "CRC-5/USB"):
        p = cr.CATALOGUE[name][0]
        T = 100 - p.W
        frame = cr.ref_attach(np.random.default_rng(1).integers(0, 2, (1, T), dtype=np.uint8), p)
        flipped = np.repeat(frame, 100, axis=0) ^ np.eye(100, dtype=np.uint8)
        _, passed, _ = cr.ref_check(flipped, p, T)
        assert not passed.any(), (name, np.flatnonzero(passed))
        assert cr.ref_check(frame, p, T)[1].all()


def test_shared_cases_are_what_the_gpu_tests_assume():
    groups = set()
    for W in cr.WIDTHS:
        p = cr.SHAPE_PARAMS[W]
        assert p.W == W and max(p.poly, p.init, p.xorout) < (1 << W)
        lengths = cr.payload_lengths(W)
        assert {1, 7, 8, 31, 32, 33, 63 * 32, 64 * 32 - W, 64 * 32, 65 * 32 + 3, (1 << 16) - W} <= set(lengths)
        for k in (1, 2, 3):
            assert {32 * k - W + d for d in (-1, 0, 1) if 32 * k - W + d >= 1} <= set(lengths)
        groups |= {cr.group_of(T) for T in lengths}
        counts = {n for i, T in enumerate(lengths) for n in cr.frame_counts(T, i)}
        assert {1, 2, 3, 4, 5} <= counts
        assert any(n % (64 // cr.group_of(T)) for i, T in enumerate(lengths) for n in cr.frame_counts(T, i) if cr.group_of(T) < 64)
    assert groups == {1, 2, 4, 8, 16, 32, 64}
    assert cr.group_of(64 * 32) == 64 and cr.group_of(65 * 32 + 3) == 64 and cr.group_of(33) == 2 and cr.group_of(32) == 1
    assert any(p.init for p in cr.SHAPE_PARAMS.values()) and any(not p.init for p in cr.SHAPE_PARAMS.values())


def test_the_noisy_point_of_the_device_loop():
    """The loop of tests/test_gpu_crc.py with the generator's f64 model: 32 frames, noise seed 2026.  At ratematch_ref's clean
    point every frame passes; at Es/N0 = 4 dB with qscale 2 both outcomes occur, 19 pass and 13 fail, and pass coincides with
    equality of the decoded and the sent frame in all 32; 5 dB gives 30 of 32."""
    assert (cr.LOOP_FRAMES, cr.LOOP_SEED, cr.LOOP_T + cr.LOOP_CRC.W) == (32, 2026, rr.LOOP_T)
    assert cr.LOOP_CRC == cr.Params(24, 0x864CFB, 0, 0) and cr.LOOP_NOISY == (4.0, 2.0) and cr.LOOP_CLEAN == (rr.LOOP_ESN0_DB, rr.LOOP_QSCALE)
    seen = {}
    for point in (cr.LOOP_CLEAN, cr.LOOP_NOISY, cr.LOOP_MIDDLE):
        payload, sent, llr = cr.loop_model(point)
        bits, got_payload, passed, crc = cr.loop_decode(llr, point)
        same = np.all(bits == sent, axis=1)
        print("Es/N0 %.1f dB, qscale %.1f: %d of %d frames pass, %d equal the sent frame" % (point + (passed.sum(), passed.size, same.sum())))
        assert np.array_equal(passed == 1, same)
        assert np.array_equal(got_payload[same], payload[same])
        assert np.count_nonzero(np.abs(np.rint(llr * np.float32(point.qscale))) > 127) == 0      # nothing on the clamp
        seen[point] = int(passed.sum())
    assert seen == {cr.LOOP_CLEAN: 32, cr.LOOP_NOISY: 19, cr.LOOP_MIDDLE: 30}
    assert min(seen[cr.LOOP_NOISY], 32 - seen[cr.LOOP_NOISY]) >= 32 // 4     # what the GPU test asserts, with margin for rounding
