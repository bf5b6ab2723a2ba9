"""Reference of the frame check of include/comms_hip.h ("frame check (CRC)"): test infrastructure, no GPU.  It is the bit-serial
register of the header comment, written from it and from nothing else, so the kernels -- which never run that register -- are
held to it bit for bit.

  crc_bits     one frame's bits in stream order -> crc, by the register as the header states it
  ref_crc      unpacked bits (frames, T) -> crc (frames,) uint32: the same register over every frame at once
  ref_attach   (frames, T) -> (frames, T + W): bit T + i is bit W-1-i of crc
  ref_check    (frames, >= T + W) -> (payload (frames, T), passed (frames,) int32, crc (frames,) uint32)
and the catalogue, the shapes and the noisy loop the CPU and GPU tests share.  Records are viterbi_ref's."""
import functools
from collections import namedtuple

import numpy as np

import noise_ref
import ratematch_ref as rr
import tx_ref
import viterbi_ref as vr
from viterbi_ref import pack_records, record_bytes, unpack_records  # noqa: F401

MAX_BITS = 1 << 16        # T + W at most
WG = 256                  # lanes per workgroup ("wg=" of kernel())
MAX_GROUP = 64

Params = namedtuple("Params", "W poly init xorout")
CHECK_STRING = b"123456789"
# name -> (parameters, bytes fed MSB first?, crc, the bytes that follow the nine in the attached record or None)
CATALOGUE = {
    "CRC-32": (Params(32, 0x04C11DB7, 0xFFFFFFFF, 0xFFFFFFFF), False, 0x649C2FD3, bytes([0x26, 0x39, 0xF4, 0xCB])),
    "X-25": (Params(16, 0x1021, 0xFFFF, 0xFFFF), False, 0x7609, bytes([0x6E, 0x90])),
    "KERMIT": (Params(16, 0x1021, 0, 0), False, 0x9184, None),
    "CCITT-FALSE": (Params(16, 0x1021, 0xFFFF, 0), True, 0x29B1, None),
    "CRC24A": (Params(24, 0x864CFB, 0, 0), True, 0xCDE703, None),
    "CRC24B": (Params(24, 0x800063, 0, 0), True, 0x23EF52, None),
    "CRC-8": (Params(8, 0x07, 0, 0), True, 0xF4, None),
    "CRC-5/USB": (Params(5, 0x05, 0x1F, 0x1F), False, 0x13, None),
}
# the values the catalogues print for the entries that are defined reflected: the crc above, bit-reversed over W bits
REVERSED = {"CRC-32": 0xCBF43926, "X-25": 0x906E, "KERMIT": 0x2189, "CRC-5/USB": 0x19}


def crc_bits(bits, p, xorout=None):
    """The register of the header, one bit at a time; xorout overrides the parameter set's (0: the raw register)."""
    W, poly, reg, _ = p
    for b in bits:
        top = ((reg >> (W - 1)) & 1) ^ int(b)
        reg = (reg << 1) % (1 << W)
        if top:
            reg ^= poly
    return reg ^ (p.xorout if xorout is None else xorout)


def ref_crc(bits, p):
    """(frames, T) 0 / 1 -> (frames,) uint32."""
    bits = np.asarray(bits, np.uint8)
    W, poly, init, xorout = p
    reg = np.full(bits.shape[0], init, np.uint64)
    mask = np.uint64((1 << W) - 1)
    for i in range(bits.shape[1]):
        top = ((reg >> np.uint64(W - 1)) & np.uint64(1)) ^ bits[:, i].astype(np.uint64)
        reg = ((reg << np.uint64(1)) & mask) ^ (top * np.uint64(poly))
    return (reg ^ np.uint64(xorout)).astype(np.uint32)


def crc_to_bits(crc, W):
    """(frames,) -> (frames, W): column i is bit W-1-i."""
    crc = np.asarray(crc, np.uint64)
    return np.stack([(crc >> np.uint64(W - 1 - i)) & np.uint64(1) for i in range(W)], axis=1).astype(np.uint8)


def ref_attach(bits, p):
    bits = np.asarray(bits, np.uint8)
    return np.concatenate([bits, crc_to_bits(ref_crc(bits, p), p.W)], axis=1)


def ref_check(bits, p, T):
    bits = np.asarray(bits, np.uint8)
    crc = ref_crc(bits[:, :T], p)
    passed = np.all(bits[:, T: T + p.W] == crc_to_bits(crc, p.W), axis=1).astype(np.int32)
    return bits[:, :T].copy(), passed, crc


def string_bits(data, msb_first):
    return np.unpackbits(np.frombuffer(data, np.uint8), bitorder="big" if msb_first else "little")


def group_of(T):
    """Lanes per frame: the smallest power of two >= the words of a payload record, at most 64 ("group=" of kernel())."""
    words, g = (T + 31) // 32, 1
    while g < words and g < MAX_GROUP:
        g *= 2
    return g


# ------------------------------------------------------------------ shapes and inputs shared by the tests
WIDTHS = (1, 5, 8, 16, 24, 32)
SHAPE_PARAMS = {1: Params(1, 1, 1, 0), 5: Params(5, 0x05, 0x1F, 0x1F), 8: Params(8, 0x07, 0x5A, 0), 16: Params(16, 0x1021, 0xFFFF, 0xFFFF),
                24: Params(24, 0x864CFB, 0, 0), 32: Params(32, 0x04C11DB7, 0xFFFFFFFF, 0xFFFFFFFF)}


def payload_lengths(W):
    """Word seams of the payload and of the attached bits (the CRC ends on a word boundary, one short, one over), every group
    size 1 ... 64, the second Horner round, and the limit."""
    t = {1, 7, 8, 31, 32, 33, 63 * 32, 64 * 32 - W, 64 * 32, 65 * 32 + 3, MAX_BITS - W}
    for k in (1, 2, 3):
        t |= {32 * k - W - 1, 32 * k - W, 32 * k - W + 1}
    t |= {32 * w - 5 for w in (3, 4, 7, 8, 13, 16, 29, 32)}          # 3 ... 32 words: groups 4, 8, 16, 32 at and below full
    return sorted(x for x in t if x >= 1 and x + W <= MAX_BITS)


def frame_counts(T, i):
    """1 ... 5 frames, and where several frames share a wave an odd count that leaves its last group partly empty."""
    per_wave = 64 // group_of(T)
    if T > 4096:
        return (1 + i % 2,)
    return (1 + i % 5, per_wave + 3) if per_wave > 1 else (1 + i % 5,)


def dirty_payload(frames, T, seed):
    """(bits (frames, T), payload records with every bit from T on set)."""
    bits = np.random.default_rng(seed).integers(0, 2, (frames, T), dtype=np.uint8)
    return bits, pack_records(bits) | ~pack_records(np.ones((frames, T), np.uint8))


# ------------------------------------------------------------------ the checked loop on the device, and its model
# PRNS payload -> CRC attach -> encoder -> rate match (ratematch_ref's loop format) -> QPSK -> AWGN -> deframer (LLR) -> rate
# dematch -> decoder -> CRC check.  The payload is one PRNS stream, T bits per frame: the source writes frame after frame, each
# to the start of its record, and what a record holds behind its T bits is not payload -- the attach node ignores it.
LOOP_CRC = CATALOGUE["CRC24A"][0]
LOOP_T = rr.LOOP_T - LOOP_CRC.W                          # 232 payload bits: the encoder sees rr.LOOP_T
LOOP_FRAMES = 32
LOOP_PRNS = rr.LOOP_PRNS
LOOP_SEED = 2026
LOOP_RECORD = record_bytes(LOOP_T)                       # 32 bytes, of which the source writes 29
LoopPoint = namedtuple("LoopPoint", "esn0_db qscale")
LOOP_CLEAN = LoopPoint(rr.LOOP_ESN0_DB, rr.LOOP_QSCALE)  # every frame decodes
LOOP_NOISY = LoopPoint(4.0, 2.0)                         # frames fail: |L| is near 5 +- 4.5, 2 L stays off the clamp
LOOP_MIDDLE = LoopPoint(5.0, 2.0)


def loop_sigma(point):
    return float(np.sqrt(10.0 ** (-point.esn0_db / 10.0)))


def loop_payload():
    """The PRNS bits of the loop as (frames, T) 0 / 1."""
    mask, state, w = LOOP_PRNS
    n = LOOP_FRAMES * LOOP_T
    return tx_ref.unpack(tx_ref.prns_packed(mask, state, n, w), n).reshape(LOOP_FRAMES, LOOP_T).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def loop_model(point):
    """(payload bits, sent frame bits (frames, rr.LOOP_T), LLR records (frames, E) f32) with tests/noise_ref.py's model of the
    generator, in f64."""
    payload = loop_payload()
    sent = ref_attach(payload, LOOP_CRC)
    coded = vr.ref_encode(sent, rr.LOOP_K, rr.LOOP_GENS, True)
    src, _ = rr.build_map(rr.LOOP_CODED, rr.LOOP_PATTERN, rr.LOOP_COLS)
    _, scr = rr.loop_scramble()
    records = pack_records(rr.ref_tx(coded, src, scr))
    x, _ = noise_ref.map_symbols(np.unpackbits(records.reshape(-1), bitorder="little"), 2, noise_ref.QPSK)
    sigma = loop_sigma(point)
    y = noise_ref.Source(LOOP_SEED).awgn(x, sigma).reshape(LOOP_FRAMES, rr.LOOP_SYMS)[:, :rr.LOOP_F]
    llr = np.empty((LOOP_FRAMES, rr.LOOP_E), np.float64)
    llr[:, 0::2] = 4.0 * (0.5 / sigma ** 2) * y.real
    llr[:, 1::2] = 4.0 * (0.5 / sigma ** 2) * y.imag
    llr = llr.astype(np.float32)
    for a in (payload, sent, llr):
        a.setflags(write=False)
    return payload, sent, llr


def loop_decode(llr, point):
    """LLR records (frames, E) f32 -> (decoded frame bits (frames, rr.LOOP_T), payload, passed, crc) by the references."""
    src, _ = rr.build_map(rr.LOOP_CODED, rr.LOOP_PATTERN, rr.LOOP_COLS)
    _, scr = rr.loop_scramble()
    dem = rr.ref_rx(np.asarray(llr, np.float32).view(np.uint32), src, rr.LOOP_CODED, scr).view(np.float32)
    bits, _ = vr.ref_decode(vr.ref_quantise(dem, point.qscale), rr.LOOP_K, rr.LOOP_GENS, rr.LOOP_T, True)
    return (bits,) + ref_check(bits, LOOP_CRC, LOOP_T)
