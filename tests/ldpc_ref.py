"""numpy reference of the LDPC code of include/comms_hip.h ("LDPC code", "LDPC encoder", "LDPC decoder"): test
infrastructure, no GPU.  Everything after ref_quantise is integer arithmetic with a fixed schedule, so the kernels are held to
it bit for bit and status for status.

  make_base     a seeded base matrix of the encoder's form (dual-diagonal parity part); random_base: any matrix in the limits
  edges         per block row the columns and shifts of its entries >= 0, in ascending column order
  dense_H       the M x N parity-check matrix from shifted identities: an independent restatement of the entry rule
  ref_encode    information bits (frames, T) -> coded bits (frames, N) by the header's rule
  ref_decode    q (frames, N) -> (bits (frames, T), status (frames,)): layered normalised min-sum, every frame and z at once
and the formats, inputs and the noisy loop the CPU and GPU tests share.  Records, quantisation and packing are
tests/viterbi_ref.py's."""
import functools
from collections import namedtuple

import numpy as np

import noise_ref
import tx_ref
from viterbi_ref import pack_records, record_bytes, ref_quantise, unpack_records  # noqa: F401  (the tests take them from here)

MAX_MB, MAX_NB, MAX_Z, MAX_ROW = 32, 64, 128, 32


# ------------------------------------------------------------------ base matrices
def make_base(mb, nb, Z, seed, colw=3, r=None, s=None, t=None):
    """(mb, nb) int16 of the encoder's form: every information column has min(colw, mb) random rows and shifts, every row at
    least 2 information entries; column kb has s in rows 0 and mb-1 and t in a middle row r; then the double diagonal of 0.
    r, s and t are drawn unless given (the draws are made either way: the rest of the matrix does not depend on them)."""
    assert 3 <= mb <= MAX_MB and mb < nb <= MAX_NB and 2 <= Z <= MAX_Z
    rng = np.random.default_rng(seed)
    kb = nb - mb
    B = np.full((mb, nb), -1, np.int16)
    for j in range(kb):
        rows = rng.choice(mb, size=min(colw, mb), replace=False)
        B[rows, j] = rng.integers(0, Z, rows.size)
    for i in range(mb):
        while np.count_nonzero(B[i, :kb] >= 0) < 2:
            free = np.flatnonzero(B[i, :kb] < 0)
            B[i, rng.choice(free)] = rng.integers(0, Z)
    drawn = int(rng.integers(1, mb - 1)), int(rng.integers(0, Z)), int(rng.integers(0, Z))
    r, s, t = (d if given is None else int(given) for given, d in zip((r, s, t), drawn))
    assert 1 <= r <= mb - 2 and 0 <= s < Z and 0 <= t < Z
    B[0, kb] = B[mb - 1, kb] = s
    B[r, kb] = t
    for i in range(mb - 1):
        B[i, kb + 1 + i] = B[i + 1, kb + 1 + i] = 0
    assert np.all(np.count_nonzero(B >= 0, axis=1) <= MAX_ROW)
    return B


def random_base(mb, nb, Z, seed, deg=None, full=None):
    """Any matrix within the limits, without the encoder's structure: 2 ... 6 entries per row at random columns; or `deg`
    entries (one number, or one per row, up to 32); with `full`, column `full` has an entry in every block row."""
    assert 1 <= mb <= MAX_MB and mb < nb <= MAX_NB and 2 <= Z <= MAX_Z
    rng = np.random.default_rng(seed)
    B = np.full((mb, nb), -1, np.int16)
    for i in range(mb):
        d = int(rng.integers(2, min(nb, 6) + 1)) if deg is None else int(deg if np.isscalar(deg) else deg[i])
        assert 2 <= d <= min(nb, MAX_ROW)
        if full is None:
            cols = rng.choice(nb, size=d, replace=False)
        else:
            others = np.delete(np.arange(nb), full)
            cols = np.concatenate([[full], rng.choice(others, size=d - 1, replace=False)])
        B[i, cols] = rng.integers(0, Z, cols.size)
    return B


def edges(B):
    """[(columns, shifts)] per block row, ascending columns."""
    B = np.asarray(B)
    return [(np.flatnonzero(row >= 0), row[row >= 0].astype(np.int64)) for row in B]


def variables(B, Z):
    """Per block row V (deg, Z): the variable that edge e of check z touches."""
    z = np.arange(Z)
    return [cols[:, None] * Z + (z[None, :] + sh[:, None]) % Z for cols, sh in edges(B)]


def dense_H(B, Z):
    """(mb Z, nb Z) uint8 from blocks: entry b is the identity with its ones moved b columns to the right, cyclically."""
    B = np.asarray(B)
    mb, nb = B.shape
    H = np.zeros((mb * Z, nb * Z), np.uint8)
    eye = np.eye(Z, dtype=np.uint8)
    for i in range(mb):
        for j in range(nb):
            if B[i, j] >= 0:
                H[i * Z:(i + 1) * Z, j * Z:(j + 1) * Z] = np.roll(eye, int(B[i, j]), axis=1)
    return H


def encoder_structure(B):
    """(r, s, t) of a matrix of the encoder's form, or None."""
    B = np.asarray(B)
    mb, nb = B.shape
    kb = nb - mb
    if mb < 3:
        return None
    rows = np.flatnonzero(B[:, kb] >= 0)
    if rows.size != 3 or rows[0] != 0 or rows[2] != mb - 1 or B[0, kb] != B[mb - 1, kb]:
        return None
    for i in range(mb - 1):
        col = B[:, kb + 1 + i]
        if list(np.flatnonzero(col >= 0)) != [i, i + 1] or col[i] != 0 or col[i + 1] != 0:
            return None
    return int(rows[1]), int(B[0, kb]), int(B[rows[1], kb])


# ------------------------------------------------------------------ the encoder
def ref_encode(bits, B, Z):
    """lambda_i[z] = XOR_{j < kb, B[i][j] >= 0} u[j Z + (z + B[i][j]) mod Z];  p_0[(z + t) mod Z] = XOR_i lambda_i[z];
    p_1[z] = lambda_0[z] ^ p_0[(z + s) mod Z];  p_{i+1}[z] = lambda_i[z] ^ p_i[z] ^ (i == r ? p_0[(z + t) mod Z] : 0)."""
    B = np.asarray(B)
    mb, nb = B.shape
    kb = nb - mb
    r, s, t = encoder_structure(B)
    u = np.asarray(bits, np.uint8)
    frames = u.shape[0]
    assert u.shape[1] == kb * Z
    z = np.arange(Z)
    lam = np.zeros((mb, frames, Z), np.uint8)
    for i in range(mb):
        for j in range(kb):
            if B[i, j] >= 0:
                lam[i] ^= u[:, j * Z + (z + int(B[i, j])) % Z]
    p = np.zeros((mb, frames, Z), np.uint8)
    p[0][:, (z + t) % Z] = np.bitwise_xor.reduce(lam, axis=0)
    p[1] = lam[0] ^ p[0][:, (z + s) % Z]
    for i in range(1, mb - 1):
        p[i + 1] = lam[i] ^ p[i]
        if i == r:
            p[i + 1] ^= p[0][:, (z + t) % Z]
    return np.concatenate([u] + [p[i] for i in range(mb)], axis=1)


# ------------------------------------------------------------------ the decoder
RULES = ("idx_last", "no_clamp", "mask32", "xor_passes")


def ref_decode(q, B, Z, max_iters=20, norm16=12, rules=()):
    """Layered normalised min-sum of the header on quantised LLRs q (frames, >= N): (bits (frames, T) uint8, status int32).
    `rules` names deliberate departures from the header, each a mistake a kernel could make, for the tests that ask whether
    the shared cases would see it (tests/test_ldpc_ref.py); no rule is the definition:
      idx_last    idx is the LAST edge at the minimum         no_clamp    |Q| is not clamped at 127
      mask32      a row of 32 edges flips no sign when its parity is odd (a sign mask built by a 32-bit shift by 32)
      xor_passes  the stopping test XORs the parities of checks z and z + 64 (one lane's two passes) where it must OR them"""
    assert set(rules) <= set(RULES)
    B = np.asarray(B)
    mb, nb = B.shape
    N, T = nb * Z, (nb - mb) * Z
    V = variables(B, Z)
    P = np.asarray(q, np.int64)[:, :N].copy()
    frames = P.shape[0]
    R = [np.zeros((frames,) + v.shape, np.int64) for v in V]
    status = np.full(frames, -int(max_iters), np.int32)
    act = np.arange(frames)
    for it in range(1, int(max_iters) + 1):
        if act.size == 0:
            break
        for i, v in enumerate(V):
            deg = v.shape[0]
            Q = P[act][:, v] - R[i][act]                                     # (act, deg, Z)
            Qc = Q if "no_clamp" in rules else np.clip(Q, -127, 127)
            a = np.abs(Qc)
            idx = np.argmin(a, axis=1)                                       # the first edge that attains the minimum
            if "idx_last" in rules:
                idx = deg - 1 - np.argmin(a[:, ::-1], axis=1)
            m1 = np.min(a, axis=1)
            first = np.arange(deg)[None, :, None] == idx[:, None, :]
            m2 = np.min(np.where(first, 1 << 20, a), axis=1)
            neg = Qc < 0
            par = np.bitwise_xor.reduce(neg, axis=1)
            if "mask32" in rules and deg == 32:
                par = np.zeros_like(par)
            mag = (int(norm16) * np.where(first, m2[:, None, :], m1[:, None, :])) >> 4
            Rn = np.where(par[:, None, :] ^ neg, -mag, mag)
            R[i][act] = Rn
            Pa = P[act]
            Pa[:, v] = Q + Rn
            P[act] = Pa
        x = P[act] < 0
        ok = np.ones(act.size, bool)
        for v in V:
            odd = np.bitwise_xor.reduce(x[:, v], axis=1)                     # (act, Z)
            if "xor_passes" in rules and Z > 64:
                odd = odd[:, :64] ^ np.pad(odd[:, 64:], ((0, 0), (0, 128 - Z)))
            ok &= ~np.any(odd, axis=1)
        status[act[ok]] = it
        act = act[~ok]
    assert rules or np.all(np.abs(P) <= 127 * 33)
    return (P[:, :T] < 0).astype(np.uint8), status


# ------------------------------------------------------------------ formats and inputs shared by the tests
Format = namedtuple("Format", "name mb nb Z seed encoder")
FORMATS = {f.name: f for f in (
    Format("A", 3, 5, 7, 11, True),          # the smallest mb the encoder takes, a fraction of a wave, records with padding bits
    Format("B", 12, 24, 27, 12, True),       # the 648-bit shape
    Format("C", 4, 24, 81, 13, True),        # two passes per layer, a ragged second pass, long rows
    Format("D", 6, 12, 64, 14, True),        # exactly one wave
    Format("E", 3, 32, 8, 15, True),         # a row of exactly 32 edges: the sign-mask limit
    Format("F", 32, 64, 128, 16, True),      # every limit at once, the largest LDS state
    Format("G", 5, 9, 33, 17, False),        # no encoder structure: decoder only
)}
# frames of a "noisy" call, its Es/N0 in dB (BPSK, LLR = 2 y / sigma^2) and the scale of its quantiser: chosen in
# tests/test_ldpc_ref.py's terms -- early exits, late exits and failures meet in one call (F has 2 frames: they differ)
NOISY = {"A": (24, 0.5, 4.0), "B": (24, -0.5, 4.0), "C": (24, 2.5, 2.0), "D": (24, -0.5, 4.0), "E": (24, 3.5, 2.0), "F": (2, -0.5, 4.0),
         "G": (24, 0.5, 4.0)}
NOISY_SEED = {"A": 0, "B": 0, "C": 0, "D": 0, "E": 0, "F": 0, "G": 0}


# ------------------------------------------------------------------ the corner table: shapes off the formats above
# The library's own sizes (ldpc.hip: comms_ldpcdec_create, ld_pack), restated: what decides the workgroup and the packing.
WG_LDS, MAX_WAVES = 64 * 1024, 4


def frame_lds(mb, nb, Z):
    """Bytes of LDS of one frame in the decoder: P as int16, padded to 8, and one 8-byte record per check."""
    return (2 * nb * Z + 7) // 8 * 8 + 8 * mb * Z


def frames_per_wg(mb, nb, Z):
    """As many frames as fit 64 KiB beside the edge table (128 bytes per block row), 1 ... 4: the waves of a workgroup."""
    return max(1, min(MAX_WAVES, (WG_LDS - 128 * mb) // frame_lds(mb, nb, Z)))


def out_words(bits):
    return record_bytes(bits) // 4


def chunks(bits):
    """64-bit ballots of a record: a lane keeps one, the wave stores after chunk 63 (one full round) and after the last."""
    return (out_words(bits) + 1) // 2


def pack_model(bits, stale=False):
    """ld_pack restated lane by lane: (frames, b) 0 / 1 -> (frames, out_words(b)) uint32.  stale=True is the mistake the
    second round invites: a lane keeps only the ballot of chunk == lane, so words of later rounds repeat the first round's."""
    bits = np.asarray(bits, np.uint8)
    frames, b = bits.shape
    words, n = out_words(b), chunks(b)
    padded = np.zeros((frames, 64 * n), np.uint8)
    padded[:, :b] = bits
    out = np.zeros((frames, words), np.uint32)
    keep = np.zeros((frames, 64), np.uint64)
    weights = np.uint64(1) << np.arange(64, dtype=np.uint64)
    for c in range(n):
        ballot = (padded[:, 64 * c: 64 * c + 64].astype(np.uint64) * weights).sum(axis=1, dtype=np.uint64)
        if not stale or c < 64:
            keep[:, c & 63] = ballot
        if (c & 63) == 63 or c + 1 == n:
            for lane in range(64):
                w = 2 * ((c & ~63) + lane)
                if w < words:
                    out[:, w] = (keep[:, lane] & np.uint64(0xFFFFFFFF)).astype(np.uint32)
                if w + 1 < words:
                    out[:, w + 1] = (keep[:, lane] >> np.uint64(32)).astype(np.uint32)
    return out


# name, shape, seed, encoder form?, the builder's arguments, and the properties the format is in the table for: every one of
# them is recomputed from the matrix and the formulas above by tests/test_ldpc_ref.py (test_corner_table_meets_its_properties)
Corner = namedtuple("Corner", "name mb nb Z seed encoder build props")
CORNERS = {f.name: f for f in (
    # decoder only (random_base)
    Corner("fpw3", 4, 64, 128, 31, False, dict(deg=32), ("fpw=3", "deg=32", "Z>64", "dec_partial_round")),   # T = 7680: 120 chunks
    Corner("fpw2", 8, 64, 128, 32, False, dict(), ("fpw=2", "Z>64", "dec_second_round")),                   # T = 7168: 112 chunks
    Corner("z65", 2, 64, 65, 33, False, dict(deg=32), ("fpw=4", "deg=32", "Z=65", "mb=2")),             # second pass: one live lane
    Corner("mb1", 1, 33, 127, 34, False, dict(deg=32), ("deg=32", "Z=127", "mb=1", "dec_odd_words")),     # T = 4064: 127 words
    Corner("least", 1, 2, 2, 35, False, dict(deg=2), ("deg=2", "Z=2", "mb=1", "nb=2", "dec_odd_words")),     # every limit at its minimum
    Corner("col32", 32, 40, 16, 36, False, dict(full=3), ("fpw=4", "full_column", "mb=32")),                 # a variable in 32 layers
    # encoder and decoder (make_base)
    Corner("r1", 5, 12, 27, 41, True, dict(r=1, s=0, t=26), ("r=1", "s=0", "t=Z-1")),
    Corner("rlast", 6, 14, 33, 42, True, dict(r=4, s=32, t=0), ("r=mb-2", "s=Z-1", "t=0")),
    Corner("encz2", 4, 10, 2, 43, True, dict(), ("Z=2",)),
    Corner("encz65", 4, 12, 65, 44, True, dict(), ("Z=65",)),
    Corner("enc5080", 8, 40, 127, 45, True, dict(), ("Z=127", "enc_partial_round")),                          # N = 5080: 159 words
)}
ENCODER_CORNERS = [n for n, f in CORNERS.items() if f.encoder]
# as NOISY: frames (more than a workgroup holds and no multiple of it), Es/N0 in dB, quantiser scale.  Dense rows do not
# converge at the formats' Es/N0, so each point is placed where its call is mixed (test_corner_noisy_cases_are_mixed)
NOISY.update({"fpw3": (7, 5.0, 2.0), "fpw2": (5, 5.0, 4.0), "z65": (9, 6.0, 2.0), "mb1": (9, 5.5, 2.0), "least": (9, -5.5, 4.0),
              "col32": (9, -2.0, 4.0), "r1": (9, -1.0, 4.0), "rlast": (9, -1.0, 4.0), "encz2": (9, -2.0, 4.0), "encz65": (9, 0.0, 4.0),
              "enc5080": (7, 2.0, 4.0)})
NOISY_SEED.update({"fpw3": 2, "fpw2": 2, "z65": 0, "mb1": 2, "least": 2, "col32": 1, "r1": 0, "rlast": 1, "encz2": 1, "encz65": 1, "enc5080": 2})
# the further message scales, and the longest run: planted errors that 255 iterations at norm16 = 1 never clear (Z = 2: cheap)
CORNER_NORMS = {"z65": 5, "rlast": 11}
CORNER_255 = "encz2"


def format_of(name):
    return FORMATS[name] if name in FORMATS else CORNERS[name]


@functools.lru_cache(maxsize=None)
def base_of(name):
    f = format_of(name)
    if name in CORNERS:
        B = (make_base if f.encoder else random_base)(f.mb, f.nb, f.Z, f.seed, **f.build)
    else:
        B = make_base(f.mb, f.nb, f.Z, f.seed) if f.encoder else random_base(f.mb, f.nb, f.Z, f.seed)
    B.setflags(write=False)
    return B


Case = namedtuple("Case", "fmt frames kind record_llrs qscale max_iters norm16")
KINDS = ("noisy", "zeros", "special", "wide", "planted")


def planted_bits(fmt):
    """Per frame the coded bits of the all-zero codeword that arrive wrong (-127 among +127): inputs aimed at the stopping test.
    One wrong bit, two in one block column, two in different block columns, two parity bits, none -- and, for Z > 64, pairs
    (v, (v + 64) mod Z) of block column 0: both wrong bits meet every block row of that column in checks 64 apart, the two
    checks one lane holds in its two passes, for every v at Z = 128 and for the v that do not wrap at Z = 81; two pairs on the
    double diagonal, whose shifts are 0, do so at any Z > 64.  The corner formats have corner_planted's frames."""
    if fmt in CORNERS:
        return corner_planted(fmt)
    f = FORMATS[fmt]
    Z, T = f.Z, (f.nb - f.mb) * f.Z
    frames = [(5 % Z,), (1, 1 + Z // 2), (2, Z + 3), (T + 1, T + Z - 1), ()]
    if Z > 64:
        frames += [(v, (v + 64) % Z) for v in range(0, Z, 1 if Z < 100 else 8)]
        frames += [((f.nb - f.mb - 1) * Z + 5, (f.nb - f.mb - 1) * Z + 69)]
        diag = (f.nb - f.mb + 1) * Z             # the first column of the double diagonal: both its shifts are 0, nothing wraps
        frames += [(diag + v, diag + v + 64) for v in (0, Z - 65)]
    return frames


def lane_mates(B, Z, most=3):
    """Pairs of variables (v, w) of one block column whose unsatisfied checks are z and z + 64 of the same block row, in every
    block row the column has an entry in: the two checks one lane holds in its two passes.  Found from the matrix, for any
    shifts: with entry b the checks of variable j Z + a and of its partner 64 further on (mod Z) are (a - b) mod Z and that
    plus 64 mod Z, lane mates when the first is below Z - 64."""
    B = np.asarray(B)
    pairs = []
    for j in range(B.shape[1]):
        shifts = B[:, j][B[:, j] >= 0].astype(int)
        for a in range(Z if shifts.size and Z > 64 else 0):
            if all(min((a - b) % Z, (a + 64 - b) % Z) < Z - 64 and abs((a - b) % Z - (a + 64 - b) % Z) == 64 for b in shifts):
                pairs.append((j * Z + a, j * Z + (a + 64) % Z))
                break
        if len(pairs) == most:
            break
    return pairs


def corner_planted(fmt):
    """planted_bits for a corner format: the same five kinds of frame with every index inside the (possibly tiny) word, for
    Z > 64 up to three lane_mates pairs, and single wrong bits until the count is more than a workgroup holds and no multiple of it."""
    f = CORNERS[fmt]
    Z, N, T = f.Z, f.nb * f.Z, (f.nb - f.mb) * f.Z
    frames = [(5 % Z,), (1, 1 + max(Z // 2, 1)), (2 % Z, Z + 3 % Z), (T + 1, T + Z - 1), ()]
    frames = [tuple(sorted({v % N for v in wrong})) for wrong in frames]
    frames += [tuple(sorted(p)) for p in lane_mates(base_of(fmt), Z)]
    fpw = frames_per_wg(f.mb, f.nb, Z)
    while len(frames) <= fpw or len(frames) % fpw == 0:
        frames.append(((7 * len(frames)) % N,))
    return frames


def make_case(fmt, kind, frames=None, qscale=None, max_iters=20, norm16=12):
    f = format_of(fmt)
    N = f.nb * f.Z
    n_noisy, _, q_noisy = NOISY[fmt]
    if kind == "planted":
        assert frames is None
        frames = len(planted_bits(fmt))
    few = n_noisy if fmt in CORNERS else min(n_noisy, 3)                    # a corner call never fits one workgroup
    frames = (n_noisy if kind in ("noisy", "wide") else few) if frames is None else frames
    qscale = (q_noisy if kind in ("noisy", "wide") else 1.0) if qscale is None else qscale
    return Case(fmt, frames, kind, N + (37 if kind == "wide" else 0), float(qscale), max_iters, norm16)


def corner_cases(fmt, kind):
    """The cases of one corner format and kind, for the GPU test and for the tests that ask what these cases can see: the
    formats' iteration limits and scales, the format's further scale, norm16 = 1 under planted errors (255 iterations once),
    quantiser scales that move the clamp under the special values."""
    norms = (12, 16) + ((CORNER_NORMS[fmt],) if fmt in CORNER_NORMS else ())
    cases = [make_case(fmt, kind, max_iters=it, norm16=nm) for it in (1, 2, 20) for nm in norms]
    if kind == "planted":
        cases += [make_case(fmt, kind, max_iters=it, norm16=1) for it in (1, 2, 20) + ((255,) if fmt == CORNER_255 else ())]
    if kind == "special":
        cases += [make_case(fmt, kind, qscale=qs) for qs in (-2.5, 0.0, 0.03)]
    return cases


@functools.lru_cache(maxsize=None)
def case_input(fmt, frames, kind):
    """(sent bits or None, LLR records f32 (frames, record_llrs)); fixed by the format, the frame count and the kind."""
    f = format_of(fmt)
    B, Z = base_of(fmt), f.Z
    N, T = f.nb * Z, (f.nb - f.mb) * Z
    rng = np.random.default_rng([f.seed, frames, KINDS.index(kind), NOISY_SEED[fmt]])
    sent = rng.integers(0, 2, (frames, T), dtype=np.uint8)
    coded = ref_encode(sent, B, Z) if f.encoder else np.zeros((frames, N), np.uint8)   # G: the all-zero word is a codeword
    llr = np.zeros((frames, N + (37 if kind == "wide" else 0)), np.float32)
    _, esn0, _ = NOISY[fmt]
    sigma2 = 0.5 / 10.0 ** (esn0 / 10.0)
    noisy = (2.0 / sigma2 * ((1.0 - 2.0 * coded) + np.sqrt(sigma2) * rng.standard_normal(coded.shape))).astype(np.float32)
    if kind in ("noisy", "wide"):
        llr[:, :N] = noisy
        llr[:, N:] = np.nan
    elif kind == "special":
        llr[:, :N] = noisy * np.float32(6.0)
        special = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 126.5, 127.5, -127.5, 0.5, 1.5, 2.5, -0.5, -0.0, 3e38], np.float32)
        hit = rng.random((frames, N)) < 0.2
        llr[:, :N][hit] = special[rng.integers(0, special.size, int(hit.sum()))]
    elif kind == "planted":
        sent = np.zeros((frames, T), np.uint8)
        llr[:] = 127.0
        for k, wrong in enumerate(planted_bits(fmt)):
            llr[k, list(wrong)] = -127.0
    if not f.encoder:
        sent = None
    for a in (sent, llr):
        if a is not None:
            a.setflags(write=False)
    return sent, llr


@functools.lru_cache(maxsize=None)
def case_data(cs):
    """(sent bits or None, LLR records, reference bits, reference status) of a case; fixed by the case."""
    f = format_of(cs.fmt)
    sent, llr = case_input(cs.fmt, cs.frames, cs.kind)
    q = ref_quantise(llr[:, : f.nb * f.Z], cs.qscale)
    bits, status = ref_decode(q, base_of(cs.fmt), f.Z, cs.max_iters, cs.norm16)
    bits.setflags(write=False)
    status.setflags(write=False)
    return sent, llr, bits, status


# ------------------------------------------------------------------ the loop on the device, and its model
# PRNS bits -> encoder -> QPSK -> AWGN -> deframer (LLR) -> decoder at (12, 24, 32): N = 768 and T = 384 are multiples of 32, so
# no record has padding, a frame is N / 2 QPSK symbols, and the deframer's LLR record is the decoder's input as it stands.
LOOP_MB, LOOP_NB, LOOP_Z, LOOP_BASE_SEED, LOOP_FRAMES = 12, 24, 32, 21, 8
LOOP_N, LOOP_T = LOOP_NB * LOOP_Z, (LOOP_NB - LOOP_MB) * LOOP_Z
LOOP_RECORD = record_bytes(LOOP_N)                      # 96 bytes
LOOP_SYMS = 4 * LOOP_RECORD                             # 384 QPSK symbols per record, all of them payload
LOOP_PRNS = (0x80200003, 0xACE1ACE1, 32)                # mask, state, width
LOOP_SEED = 2025
LOOP_ESN0_DB = 4.5                                      # Es = 2 (unit components), N0 = 2 sigma^2: Es / N0 = 1 / sigma^2
LOOP_SIGMA = float(np.sqrt(10.0 ** (-LOOP_ESN0_DB / 10.0)))
LOOP_LLR_SCALE = 0.5 / LOOP_SIGMA ** 2                  # the deframer's s = 1 / (2 sigma^2): L = 2 z / sigma^2
LOOP_QSCALE = 8.0
LOOP_ITERS = 20


@functools.lru_cache(maxsize=None)
def loop_base():
    B = make_base(LOOP_MB, LOOP_NB, LOOP_Z, LOOP_BASE_SEED)
    B.setflags(write=False)
    return B


def loop_bits():
    """The PRNS bits of the loop as (frames, T) 0 / 1."""
    mask, state, w = LOOP_PRNS
    packed = tx_ref.prns_packed(mask, state, LOOP_FRAMES * LOOP_T, w)
    return tx_ref.unpack(packed, LOOP_FRAMES * LOOP_T).reshape(LOOP_FRAMES, LOOP_T).astype(np.uint8)


def loop_model():
    """(sent bits, model LLRs (frames, N) f32) with tests/noise_ref.py's model of the generator, in f64."""
    sent = loop_bits()
    records = pack_records(ref_encode(sent, loop_base(), LOOP_Z))
    stream_bits = np.unpackbits(records.reshape(-1), bitorder="little")
    x, _ = noise_ref.map_symbols(stream_bits, 2, noise_ref.QPSK)
    y = noise_ref.Source(LOOP_SEED).awgn(x, LOOP_SIGMA).reshape(LOOP_FRAMES, LOOP_SYMS)
    llr = np.empty((LOOP_FRAMES, LOOP_N), np.float64)
    llr[:, 0::2] = 4.0 * LOOP_LLR_SCALE * y.real
    llr[:, 1::2] = 4.0 * LOOP_LLR_SCALE * y.imag
    return sent, llr.astype(np.float32)
