"""numpy reference of the convolutional code of include/comms_hip.h ("convolutional code", "Viterbi decoder"): test
infrastructure, no GPU.  Everything after ref_quantise is integer arithmetic, so the kernels are held to it bit for bit.

  ref_encode    bits (frames, T) -> coded bits (frames, n * steps):  r_t = (u_t << (K-1)) | s_t, bit j = parity(r_t & g_j)
  ref_quantise  f32 LLRs -> q = clamp(rint(L * qscale), -127, 127), NaN -> 0
  ref_decode    q (frames, n * steps) -> (bits (frames, T), final metric (frames,)) by the add-compare-select and traceback
                rules of the header, every frame at once
and the shapes, inputs and the noisy loop the CPU and GPU tests share."""
import functools
import itertools
from collections import namedtuple

import numpy as np

import noise_ref
import tx_ref

TERMINATED, TRUNCATED = 0, 1
MAX_STEPS = 1 << 16
LDS_STEPS = 2048          # the seam the library states in comms_viterbi_get_kernel ("seam=")
WAVES = 4                 # waves per workgroup ("waves=")
# one code per (K, n): generators in the header's convention (the input bit meets bit K-1 of g)
GENS = {(3, 2): (0o7, 0o5), (3, 3): (0o7, 0o7, 0o5), (4, 2): (0o17, 0o13), (4, 3): (0o13, 0o15, 0o17), (5, 2): (0o23, 0o35),
        (5, 3): (0o25, 0o33, 0o37), (6, 2): (0o53, 0o75), (6, 3): (0o47, 0o53, 0o75), (7, 2): (0o171, 0o133),
        (7, 3): (0o171, 0o133, 0o165)}


def record_bytes(bits):
    """ceil(bits / 8) rounded up to a multiple of 4."""
    return ((int(bits) + 7) // 8 + 3) // 4 * 4


def n_steps(T, K, terminated):
    return int(T) + (K - 1 if terminated else 0)


def pack_records(bits):
    """(frames, b) 0 / 1 -> (frames, record_bytes(b)) uint8, LSB first, padding 0."""
    bits = np.asarray(bits, np.uint8)
    out = np.zeros((bits.shape[0], record_bytes(bits.shape[1])), np.uint8)
    packed = np.packbits(bits, axis=1, bitorder="little")
    out[:, : packed.shape[1]] = packed
    return out


def unpack_records(records, b):
    return np.unpackbits(np.asarray(records, np.uint8), axis=1, bitorder="little")[:, :b]


def ref_encode(bits, K, gens, terminated=True):
    u = np.asarray(bits, np.uint8)
    frames, T = u.shape
    steps = n_steps(T, K, terminated)
    pad = np.zeros((frames, K - 1 + steps), np.uint8)      # pad[:, t + e] = u_{t - (K-1) + e}: bit e of r_t
    pad[:, K - 1: K - 1 + T] = u
    out = np.zeros((frames, steps, len(gens)), np.uint8)
    for j, g in enumerate(gens):
        for e in range(K):
            if (g >> e) & 1:
                out[:, :, j] ^= pad[:, e: e + steps]
    return out.reshape(frames, steps * len(gens))


def ref_quantise(llr, qscale=1.0):
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.asarray(llr, np.float32) * np.float32(qscale)           # one f32 product
        r = np.rint(x)                                                  # halves to even
    r = np.where(np.isnan(x), np.float32(0), r)
    return np.clip(r, -127, 127).astype(np.int32)


@functools.lru_cache(maxsize=None)
def trellis(K, gens):
    """from[b][s'], sign[b][j][s'] = 1 - 2 c."""
    S = 1 << (K - 1)
    sp = np.arange(S)
    u = sp >> (K - 2)
    frm = np.stack([((sp << 1) | b) & (S - 1) for b in (0, 1)])
    sign = np.zeros((2, len(gens), S), np.int64)
    for b in (0, 1):
        r = (u << (K - 1)) | frm[b]
        for j, g in enumerate(gens):
            c = np.array([bin(int(v) & g).count("1") & 1 for v in r])
            sign[b, j] = 1 - 2 * c
    return frm, sign


RULES = ("ge", "highest")


def ref_decode(q, K, gens, T, terminated=True, rules=()):
    """`rules` names deliberate departures from the header's tie rules, for the tests that ask whether the shared cases would
    see them (tests/test_viterbi_ref.py): "ge" takes b = 1 on equal candidates, "highest" ends a truncated frame in the
    highest state among equal final metrics.  No rule is the definition."""
    assert set(rules) <= set(RULES)
    q = np.asarray(q, np.int64)
    frames = q.shape[0]
    n, S = len(gens), 1 << (K - 1)
    steps = n_steps(T, K, terminated)
    assert q.shape[1] >= n * steps and steps <= MAX_STEPS
    frm, sign = trellis(K, tuple(gens))
    M = np.full((frames, S), -(1 << 30), np.int64)
    M[:, 0] = 0
    D = np.zeros((steps, frames, S), bool)
    qs = q[:, : n * steps].reshape(frames, steps, n)
    for t in range(steps):
        qt = qs[:, t, :]
        c0 = M[:, frm[0]] + qt @ sign[0]
        c1 = M[:, frm[1]] + qt @ sign[1]
        D[t] = c1 >= c0 if "ge" in rules else c1 > c0                    # b = 1 only when strictly greater
        M = np.where(D[t], c1, c0)
    assert np.all(np.abs(M) < (1 << 31))
    s = np.zeros(frames, np.int64) if terminated else np.argmax(M, axis=1)   # argmax: the lowest index among equals
    if "highest" in rules and not terminated:
        s = S - 1 - np.argmax(M[:, ::-1], axis=1)
    metric = M[np.arange(frames), s].astype(np.int32)
    bits = np.zeros((frames, steps), np.uint8)
    rows = np.arange(frames)
    for t in range(steps - 1, -1, -1):
        bits[:, t] = s >> (K - 2)
        s = ((s << 1) | D[t][rows, s]) & (S - 1)
    return bits[:, :T], metric


def brute_force_metric(q, K, gens, T, terminated=True):
    """max over all 2^T codewords of sum q (1 - 2 c), one frame; and the set of information words that attain it."""
    words = np.array(list(itertools.product((0, 1), repeat=T)), np.uint8)
    coded = ref_encode(words, K, gens, terminated).astype(np.int64)
    corr = (1 - 2 * coded) @ np.asarray(q, np.int64)[: coded.shape[1]]
    best = int(corr.max())
    return best, words[corr == best]


# ------------------------------------------------------------------ shapes and inputs shared by the tests
def step_counts(K):
    """Block seams (64 steps), the LDS / workspace seam and its two sides, short frames."""
    return sorted({1, 2, K - 1, K, 63, 64, 65, 127, 128, 129, 1000, LDS_STEPS, LDS_STEPS + 1})


Case = namedtuple("Case", "K n gens terminated T steps frames kind record_llrs qscale")
KINDS = ("noisy", "zeros", "special", "wide")


def make_case(K, n, terminated, steps, frames, kind, qscale=1.0, gens=None):
    T = steps - (K - 1 if terminated else 0)
    assert T >= 1
    record = n * steps + (37 if kind == "wide" else 0)
    gens = GENS[(K, n)] if gens is None else tuple(int(g) for g in gens)
    assert len(gens) == n and all(0 < g < (1 << K) for g in gens)
    return Case(K, n, gens, terminated, T, steps, frames, kind, record, qscale)


def case_input(cs):
    """(sent bits, LLR records f32 (frames, record_llrs)) of a case: the seed does not depend on the generators."""
    rng = np.random.default_rng(hash((cs.K, cs.n, cs.terminated, cs.steps, cs.frames, KINDS.index(cs.kind))) & 0xFFFFFFFF)
    sent = rng.integers(0, 2, (cs.frames, cs.T), dtype=np.uint8)
    coded = ref_encode(sent, cs.K, cs.gens, cs.terminated)
    used = cs.n * cs.steps
    llr = np.zeros((cs.frames, cs.record_llrs), np.float32)
    if cs.kind in ("noisy", "wide"):        # +-20 with noise of the same size: the decoder itself errs on long frames
        llr[:, :used] = (20.0 * (1.0 - 2.0 * coded) + 24.0 * rng.standard_normal(coded.shape)).astype(np.float32)
        llr[:, used:] = np.nan
    elif cs.kind == "special":
        llr[:, :used] = (30.0 * (1.0 - 2.0 * coded) + 40.0 * rng.standard_normal(coded.shape)).astype(np.float32)
        special = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 126.5, 127.5, -127.5, 0.5, 1.5, 2.5, -0.5, -0.0, 3e38], np.float32)
        hit = rng.random((cs.frames, used)) < 0.2
        llr[:, :used][hit] = special[rng.integers(0, special.size, int(hit.sum()))]
    return sent, llr


@functools.lru_cache(maxsize=None)
def case_data(cs):
    """(sent bits, LLR records f32 (frames, record_llrs), reference bits, reference metrics) of a case; fixed by the case."""
    sent, llr = case_input(cs)
    q = ref_quantise(llr[:, : cs.n * cs.steps], cs.qscale)
    bits, metric = ref_decode(q, cs.K, cs.gens, cs.T, cs.terminated)
    for a in (sent, llr, bits, metric):
        a.setflags(write=False)
    return sent, llr, bits, metric


# ------------------------------------------------------------------ generators off the one set per (K, n)
def _gen_corners(K, n):
    """The sets the tie rules decide most bits in: a generator without the input bit; one without the oldest register bit;
    every generator without it (both predecessors of a state then emit the same coded bits: the compare ties whenever their
    metrics do); a single bit beside all ones; one generator n times; two seeded random sets."""
    base, top, ones = GENS[(K, n)], 1 << (K - 1), (1 << K) - 1
    sets = [("input_clear", (base[0] & ~top,) + base[1:]), ("oldest_clear", (base[0] & ~1,) + base[1:]),
            ("oldest_clear_all", tuple(g & ~1 for g in base)), ("single_and_ones", (top, ones, 1)[:n]), ("equal", (base[0],) * n)]
    for i in range(2):
        rng = np.random.default_rng([K, n, i])
        sets.append(("random%d" % i, tuple(int(g) for g in rng.integers(1, ones + 1, n))))
    return sets


GEN_CORNERS = {(K, n): _gen_corners(K, n) for K in range(3, 8) for n in (2, 3)}
CORNER_KINDS, CORNER_FRAMES = ("noisy", "zeros", "special"), 3


def corner_steps(K):
    """A short frame, two block seams, the workspace form."""
    return (K, 65, 129, LDS_STEPS + 1)


@functools.lru_cache(maxsize=None)
def corner_data(K, n, gens, terminated, steps, rules=()):
    """[(case, LLR records, reference bits, reference metrics)] per kind of CORNER_KINDS: the cases are make_case's and the
    inputs case_input's; the kinds' frames go through ref_decode together, which decodes frame by frame."""
    cases = [make_case(K, n, terminated, steps, CORNER_FRAMES, kind, gens=gens) for kind in CORNER_KINDS]
    llrs = [case_input(cs)[1] for cs in cases]
    q = np.concatenate([ref_quantise(llr[:, : n * steps]) for llr in llrs])
    bits, metric = ref_decode(q, K, gens, cases[0].T, terminated, rules)
    return [(cs, llr, bits[CORNER_FRAMES * i: CORNER_FRAMES * (i + 1)], metric[CORNER_FRAMES * i: CORNER_FRAMES * (i + 1)])
            for i, (cs, llr) in enumerate(zip(cases, llrs))]


# ------------------------------------------------------------------ the loop on the device, and its model
# PRNS bits -> encoder -> QPSK -> AWGN -> deframer (LLR) -> decoder.  A frame's coded record (padding included) is modulated
# whole; the deframer's synthetic detection of frame f sits at symbol f * LOOP_SYMS with corr = 1, so the payload is the
# LOOP_F symbols that carry the n * steps coded bits and its LLR record is the decoder's input as it stands.
LOOP_K, LOOP_N, LOOP_T, LOOP_FRAMES = 7, 2, 256, 8
LOOP_GENS = GENS[(7, 2)]
LOOP_STEPS = LOOP_T + LOOP_K - 1                        # 262
LOOP_CODED = LOOP_N * LOOP_STEPS                        # 524 coded bits
LOOP_RECORD = record_bytes(LOOP_CODED)                  # 68 bytes
LOOP_SYMS = 4 * LOOP_RECORD                             # 272 QPSK symbols per record
LOOP_F = LOOP_CODED // 2                                # 262 payload symbols
LOOP_PRNS = (0x80200003, 0xACE1ACE1, 32)                # mask, state, width
LOOP_SEED = 2024
LOOP_ESN0_DB = 5.0                                      # Es = 2 (unit components), N0 = 2 sigma^2: Es / N0 = 1 / sigma^2
LOOP_SIGMA = float(np.sqrt(10.0 ** (-LOOP_ESN0_DB / 10.0)))
LOOP_LLR_SCALE = 0.5 / LOOP_SIGMA ** 2                  # the deframer's s = 1 / (2 sigma^2): L = 2 z / sigma^2
LOOP_QSCALE = 8.0                                       # |L| is near 6.3 +- 3.6: 8 L stays below 127 but for the rarest values


def loop_bits():
    """The PRNS bits of the loop as (frames, T) 0 / 1."""
    mask, state, w = LOOP_PRNS
    packed = tx_ref.prns_packed(mask, state, LOOP_FRAMES * LOOP_T, w)
    return tx_ref.unpack(packed, LOOP_FRAMES * LOOP_T).reshape(LOOP_FRAMES, LOOP_T).astype(np.uint8)


def loop_model():
    """(sent bits, model LLRs (frames, LOOP_CODED) f32) with tests/noise_ref.py's model of the generator, in f64."""
    sent = loop_bits()
    records = pack_records(ref_encode(sent, LOOP_K, LOOP_GENS, True))
    stream_bits = np.unpackbits(records.reshape(-1), bitorder="little")
    x, _ = noise_ref.map_symbols(stream_bits, 2, noise_ref.QPSK)
    y = noise_ref.Source(LOOP_SEED).awgn(x, LOOP_SIGMA).reshape(LOOP_FRAMES, LOOP_SYMS)[:, :LOOP_F]
    llr = np.empty((LOOP_FRAMES, LOOP_CODED), np.float64)
    llr[:, 0::2] = 4.0 * LOOP_LLR_SCALE * y.real
    llr[:, 1::2] = 4.0 * LOOP_LLR_SCALE * y.imag
    return sent, llr.astype(np.float32)
