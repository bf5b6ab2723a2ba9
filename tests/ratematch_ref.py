"""numpy reference of the rate matching of include/comms_hip.h ("rate matching"): test infrastructure, no GPU.  Only bits and
words move, so the kernels are held to it bit for bit.

  build_map   (n_coded, pattern, cols, perm) -> (src (E,), inv (n_coded,) with -1 where punctured): src[k] = kept[pi[k]]
  ref_tx      unpacked coded bits (frames, N) -> transmitted bits (frames, E): in[src[k]] ^ scramble[k]
  ref_rx      uint32 views of f32 records (frames, >= E) -> (frames, N) uint32: 0 (+0.0f) where punctured, else in[inv[i]] with
              bit 31 toggled where scramble bit inv[i] is 1
and the seam constants, the case lists and the punctured loop the CPU and GPU tests share."""
import functools

import numpy as np

import noise_ref
import tx_ref
import viterbi_ref as vr
from viterbi_ref import pack_records, record_bytes, unpack_records  # noqa: F401  (the record rules are the code's)

MAX_CODED = 3 << 16
MAX_PATTERN = 256
LDS_SEAM = 2048           # table entries staged in LDS at most (E on transmit, N on receive): "seam=" of kernel()
WG = 256                  # lanes per workgroup ("wg=")
SIGN = np.uint32(0x80000000)
# the usual patterns of the K = 7 (171, 133) code, in coded-stream order t * n + j
PATTERNS = {
    "none": None,
    "2/3": (1, 1, 0, 1),
    "3/4": (1, 1, 0, 1, 1, 0),
    "5/6": (1, 1, 0, 1, 1, 0, 0, 1, 1, 0),
    "7/8": (1, 1, 0, 1, 0, 1, 0, 1, 1, 0, 0, 1, 1, 0),
}


def kept_positions(n_coded, pattern):
    i = np.arange(int(n_coded))
    if pattern is None:
        return i
    p = np.asarray(pattern, np.uint8)
    return i[p[i % p.size] == 1]


def n_tx_bits(n_coded, pattern):
    return int(kept_positions(n_coded, pattern).size)


def interleave_by_definition(E, C):
    """pi of the pruned block interleaver, literally: write the E bits into rows of C cells, read the columns, skip the cells
    past the last bit."""
    R = -(-E // C)
    cells = np.full(R * C, -1, np.int64)
    cells[:E] = np.arange(E)
    order = cells.reshape(R, C).T.reshape(-1)
    return order[order >= 0]


def interleave_closed_form(E, C):
    """The same by the header's closed form: the bit of cell (r, c) leaves at k = c R - max(0, c - rem) + r.  (C > E is one
    row read left to right, the identity; the library refuses it.)"""
    R = -(-E // C)
    rem = E - (R - 1) * C
    m = np.arange(E)
    r, c = m // C, m % C
    pi = np.empty(E, np.int64)
    pi[c * R - np.maximum(0, c - rem) + r] = m
    return pi


def build_map(n_coded, pattern=None, cols=0, perm=None):
    kept = kept_positions(n_coded, pattern)
    E = kept.size
    assert E >= 1
    if perm is not None:
        assert cols == 0
        pi = np.asarray(perm, np.int64)
        assert np.array_equal(np.sort(pi), np.arange(E))
    elif cols <= 1:
        pi = np.arange(E)
    else:
        pi = interleave_closed_form(E, cols)
    src = kept[pi].astype(np.uint32)
    inv = np.full(int(n_coded), -1, np.int32)
    inv[src] = np.arange(E, dtype=np.int32)
    return src, inv


def ref_tx(bits, src, scramble=None):
    """bits (frames, >= N) 0 / 1, scramble (E,) 0 / 1 or None -> (frames, E)."""
    out = np.asarray(bits, np.uint8)[:, src]
    return out if scramble is None else out ^ np.asarray(scramble, np.uint8)[None, : src.size]


def ref_rx(words, src, n_coded, scramble=None):
    """words (frames, >= E) uint32 -> (frames, n_coded) uint32."""
    w = np.asarray(words, np.uint32)[:, : src.size]
    if scramble is not None:
        w = w ^ (np.asarray(scramble, np.uint32)[None, : src.size] << np.uint32(31))
    out = np.zeros((w.shape[0], int(n_coded)), np.uint32)
    out[:, src] = w
    return out


# ------------------------------------------------------------------ shapes shared by the tests
def cols_of(E):
    """The interleaver widths of the issue for E transmitted bits: none, 2, one row, a C with rem = 1, a C with rem = C
    (0 < C < E), as far as they exist and are allowed (2 <= C <= E)."""
    out = [0]
    if E >= 2:
        out += [2, E]
    rem1 = [C for C in range(2, E) if (E - 1) % C == 0]
    full = [C for C in range(2, E) if E % C == 0]
    for found in (rem1, full):
        if found:
            out.append(found[0])
    return sorted(set(out))


def coded_lengths(pattern):
    """N of the issue -- 1, 14, 140, 2012 -- then an N for every E in {1, 31, 32, 33, 63, 64, 65} under this pattern (the
    smallest), and lengths whose last positions are punctured."""
    out = [1, 14, 140, 2012]
    for E in (1, 31, 32, 33, 63, 64, 65):
        N = 1
        while n_tx_bits(N, pattern) < E:
            N += 1
        out.append(N)
    for base in (14, 140, 2012) if pattern is not None else ():   # the next lengths that end on punctured positions
        N = base
        while pattern[(N - 1) % len(pattern)] == 1:
            N += 1
        out.append(N)
    return [N for N in sorted(set(out)) if n_tx_bits(N, pattern) >= 1]


def interleavers(E, seed):
    """(cols, perm) of every interleaver form for E bits: the widths of cols_of, the reversed and a seeded random perm."""
    forms = [(C, None) for C in cols_of(E)]
    forms.append((0, np.arange(E - 1, -1, -1, dtype=np.uint32)))
    forms.append((0, np.random.default_rng(seed).permutation(E).astype(np.uint32)))
    return forms


def scramble_bits(E, seed):
    return np.random.default_rng(1000 + seed).integers(0, 2, E, dtype=np.uint8)


def pack_bits(bits):
    """(E,) 0 / 1 -> ceil(E / 8) bytes, LSB first: the `scramble` argument."""
    return np.packbits(np.asarray(bits, np.uint8), bitorder="little")


SPECIAL = np.array([0x7FC00000, 0xFFC00001, 0x7FA12345, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x00000001, 0x807FFFFF,
                    0x00800000, 0x7F7FFFFF, 0xBF800000], np.uint32)   # NaNs with payloads, +-inf, +-0, denormals, ordinary values


def llr_words(frames, record, E, seed):
    """Receive records as uint32: random finite values with SPECIAL sprinkled over the used part, NaN behind it."""
    rng = np.random.default_rng(seed)
    x = (8.0 * rng.standard_normal((frames, record))).astype(np.float32).view(np.uint32).copy()
    hit = rng.random((frames, E)) < 0.25
    x[:, :E][hit] = SPECIAL[rng.integers(0, SPECIAL.size, int(hit.sum()))]
    x[:, E:] = 0x7FC00BAD
    return x


# ------------------------------------------------------------------ the punctured loop on the device, and its model
# PRNS bits -> encoder -> rate match (3/4, 17 columns, PRNS scramble) -> QPSK -> AWGN -> deframer (LLR) -> rate dematch ->
# decoder.  A frame's transmitted record (padding included) is modulated whole; the deframer's synthetic detection of frame f
# sits at symbol f * LOOP_SYMS with corr = 1, and its LOOP_F payload symbols carry exactly the E transmitted bits.
LOOP_K, LOOP_T, LOOP_FRAMES = vr.LOOP_K, vr.LOOP_T, vr.LOOP_FRAMES
LOOP_GENS = vr.LOOP_GENS
LOOP_CODED = vr.LOOP_CODED                              # N = 524
LOOP_PATTERN = PATTERNS["3/4"]
LOOP_COLS = 17
LOOP_E = n_tx_bits(LOOP_CODED, LOOP_PATTERN)            # 350 transmitted bits
LOOP_RECORD = record_bytes(LOOP_E)                      # 44 bytes
LOOP_SYMS = 4 * LOOP_RECORD                             # 176 QPSK symbols per record
LOOP_F = LOOP_E // 2                                    # 175 payload symbols
LOOP_PRNS = vr.LOOP_PRNS
LOOP_SCRAMBLE_PRNS = (0x80200003, 0x1234ABCD, 32)       # mask, state, width of the scrambling sequence
LOOP_SEED = 2025
LOOP_ESN0_DB = 7.0                                      # Es / N0 = 1 / sigma^2 (unit components), as in tests/viterbi_ref.py
LOOP_SIGMA = float(np.sqrt(10.0 ** (-LOOP_ESN0_DB / 10.0)))
LOOP_LLR_SCALE = 0.5 / LOOP_SIGMA ** 2                  # the deframer's s = 1 / (2 sigma^2): L = 2 z / sigma^2
LOOP_QSCALE = 4.0                                       # |L| is near 10 +- 4.5 and below 26 at this seed: 4 L stays off the clamp


def loop_scramble():
    """The E scramble bits of the loop, packed (the `scramble` argument) and as 0 / 1."""
    mask, state, w = LOOP_SCRAMBLE_PRNS
    packed = tx_ref.prns_packed(mask, state, LOOP_E, w)
    return packed, tx_ref.unpack(packed, LOOP_E).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def loop_model():
    """(sent bits, coded bits, received LLR records (frames, E) f32, scramble bits) with tests/noise_ref.py's model of the
    generator, in f64."""
    sent = vr.loop_bits()
    coded = vr.ref_encode(sent, LOOP_K, LOOP_GENS, True)
    src, _ = build_map(LOOP_CODED, LOOP_PATTERN, LOOP_COLS)
    _, scr = loop_scramble()
    records = pack_records(ref_tx(coded, src, scr))
    stream_bits = np.unpackbits(records.reshape(-1), bitorder="little")
    x, _ = noise_ref.map_symbols(stream_bits, 2, noise_ref.QPSK)
    y = noise_ref.Source(LOOP_SEED).awgn(x, LOOP_SIGMA).reshape(LOOP_FRAMES, LOOP_SYMS)[:, :LOOP_F]
    llr = np.empty((LOOP_FRAMES, LOOP_E), np.float64)
    llr[:, 0::2] = 4.0 * LOOP_LLR_SCALE * y.real
    llr[:, 1::2] = 4.0 * LOOP_LLR_SCALE * y.imag
    llr = llr.astype(np.float32)
    for a in (sent, coded, llr, scr):
        a.setflags(write=False)
    return sent, coded, llr, scr
