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
def make_base(mb, nb, Z, seed, colw=3):
    """(mb, nb) int16 of the encoder's form: every information column has min(colw, mb) random rows and shifts, every row at
    least 2 information entries; column kb has s in rows 0 and mb-1 and t in a middle row r; then the double diagonal of 0."""
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
    r = int(rng.integers(1, mb - 1))
    s, t = int(rng.integers(0, Z)), int(rng.integers(0, Z))
    B[0, kb] = B[mb - 1, kb] = s
    B[r, kb] = t
    for i in range(mb - 1):
        B[i, kb + 1 + i] = B[i + 1, kb + 1 + i] = 0
    assert np.all(np.count_nonzero(B >= 0, axis=1) <= MAX_ROW)
    return B


def random_base(mb, nb, Z, seed):
    """Any matrix within the limits, without the encoder's structure: 2 ... 6 entries per row at random columns."""
    assert 1 <= mb <= MAX_MB and mb < nb <= MAX_NB and 2 <= Z <= MAX_Z
    rng = np.random.default_rng(seed)
    B = np.full((mb, nb), -1, np.int16)
    for i in range(mb):
        cols = rng.choice(nb, size=int(rng.integers(2, min(nb, 6) + 1)), replace=False)
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
def ref_decode(q, B, Z, max_iters=20, norm16=12):
    """Layered normalised min-sum of the header on quantised LLRs q (frames, >= N): (bits (frames, T) uint8, status int32)."""
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
            Qc = np.clip(Q, -127, 127)
            a = np.abs(Qc)
            idx = np.argmin(a, axis=1)                                       # the first edge that attains the minimum
            m1 = np.min(a, axis=1)
            first = np.arange(deg)[None, :, None] == idx[:, None, :]
            m2 = np.min(np.where(first, 1 << 20, a), axis=1)
            neg = Qc < 0
            par = np.bitwise_xor.reduce(neg, axis=1)
            mag = (int(norm16) * np.where(first, m2[:, None, :], m1[:, None, :])) >> 4
            Rn = np.where(par[:, None, :] ^ neg, -mag, mag)
            R[i][act] = Rn
            Pa = P[act]
            Pa[:, v] = Q + Rn
            P[act] = Pa
        x = P[act] < 0
        ok = np.ones(act.size, bool)
        for v in V:
            ok &= ~np.any(np.bitwise_xor.reduce(x[:, v], axis=1), axis=1)
        status[act[ok]] = it
        act = act[~ok]
    assert np.all(np.abs(P) <= 127 * 33)
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


@functools.lru_cache(maxsize=None)
def base_of(name):
    f = FORMATS[name]
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
    double diagonal, whose shifts are 0, do so at any Z > 64."""
    f = FORMATS[fmt]
    Z, T = f.Z, (f.nb - f.mb) * f.Z
    frames = [(5 % Z,), (1, 1 + Z // 2), (2, Z + 3), (T + 1, T + Z - 1), ()]
    if Z > 64:
        frames += [(v, (v + 64) % Z) for v in range(0, Z, 1 if Z < 100 else 8)]
        frames += [((f.nb - f.mb - 1) * Z + 5, (f.nb - f.mb - 1) * Z + 69)]
        diag = (f.nb - f.mb + 1) * Z             # the first column of the double diagonal: both its shifts are 0, nothing wraps
        frames += [(diag + v, diag + v + 64) for v in (0, Z - 65)]
    return frames


def make_case(fmt, kind, frames=None, qscale=None, max_iters=20, norm16=12):
    f = FORMATS[fmt]
    N = f.nb * f.Z
    n_noisy, _, q_noisy = NOISY[fmt]
    if kind == "planted":
        assert frames is None
        frames = len(planted_bits(fmt))
    frames = (n_noisy if kind in ("noisy", "wide") else min(n_noisy, 3)) if frames is None else frames
    qscale = (q_noisy if kind in ("noisy", "wide") else 1.0) if qscale is None else qscale
    return Case(fmt, frames, kind, N + (37 if kind == "wide" else 0), float(qscale), max_iters, norm16)


@functools.lru_cache(maxsize=None)
def case_input(fmt, frames, kind):
    """(sent bits or None, LLR records f32 (frames, record_llrs)); fixed by the format, the frame count and the kind."""
    f = FORMATS[fmt]
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
    f = FORMATS[cs.fmt]
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
