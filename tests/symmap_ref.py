"""Numpy restatement of the symbol mapper's and the soft demapper's definitions (include/comms_hip.h, "symbol mapper and soft
demapper"): the tables, the table copy of the mapper, and the BRUTE-FORCE decision and max-log rule over all 2^m points, every
f32 operation rounded on its own.  There is no per-axis shortcut in ref_bits / ref_llr; the per-axis identities the kernels
use are restated separately (axis_llr, axis_index, naive_axis_index) so that tests/test_symmap_ref.py can hold them to the
brute force.  Shared by the CPU and the GPU tests; the shapes, tables and inputs of both are defined here."""
import functools

import numpy as np

MAX_BITS = 8
MAX_E = 1 << 20
MAX_F = 1 << 20
MAX_WORD = 512
MAX_GAP = 1 << 16
WG = 256                  # lanes per workgroup ("wg=" of kernel())
GRID_CAP = 8 * 256        # no persistent grid of the library exceeds eight workgroups on each of 256 CUs
f32 = np.float32

BPSK = np.array([1, -1], np.complex64)
QPSK = np.array([1 + 1j, -1 + 1j, 1 - 1j, -1 - 1j], np.complex64)
# cos of 0, 1, 2, 3, 4 sixteenths of a turn: the first-octant values every PSK point is made of
_C16 = (1.0, 0.92387953251128674, 0.70710678118654757, 0.38268343236508977, 0.0)


def record_bytes(bits):
    """ceil(bits / 8) rounded up to a multiple of 4."""
    return ((int(bits) + 7) // 8 + 3) // 4 * 4


def pack_records(bits):
    """(frames, b) 0 / 1 -> (frames, record_bytes(b)) uint8, LSB first, padding 0."""
    bits = np.asarray(bits, np.uint8)
    out = np.zeros((bits.shape[0], record_bytes(bits.shape[1])), np.uint8)
    packed = np.packbits(bits, axis=1, bitorder="little")
    out[:, : packed.shape[1]] = packed
    return out


def unpack_records(records, b):
    return np.unpackbits(np.asarray(records, np.uint8), axis=1, bitorder="little")[:, :b]


# ------------------------------------------------------------------ tables
def gray_rank(g):
    r = 0
    while g:
        r ^= g
        g >>= 1
    return r


def _c64(re, im):
    return (np.asarray(re, np.float64).astype(f32) + 1j * np.asarray(im, np.float64).astype(f32)).astype(np.complex64)


def qam_table(m, scale=1.0):
    if m == 1:
        return _c64([scale, -scale], [0.0, 0.0])
    assert m in (2, 4, 6, 8)
    k = m // 2
    top = (1 << k) - 1
    level = [(top - 2 * gray_rank(g)) * float(scale) for g in range(1 << k)]
    return _c64([level[v & top] for v in range(1 << m)], [level[v >> k] for v in range(1 << m)])


def _cos16(t):
    t &= 15
    if t > 8:
        t = 16 - t
    return -_C16[8 - t] if t > 4 else _C16[t]


def psk_table(m, scale=1.0):
    assert 1 <= m <= 4
    step, phi = 16 >> m, (2 if m == 2 else 0)
    t = [gray_rank(v) * step + phi for v in range(1 << m)]
    return _c64([float(scale) * _cos16(a) for a in t], [float(scale) * _cos16(a - 4) for a in t])


def default_table(m):
    return {1: BPSK, 2: QPSK}[m]


def nearest_neighbours_differ_in_one_bit(table):
    """Every pair of points at the table's minimum distance has indices one bit apart."""
    c = np.asarray(table, np.complex128)
    d = np.abs(c[:, None] - c[None, :])
    np.fill_diagonal(d, np.inf)
    near = np.argwhere(d <= d.min() * (1 + 1e-6))
    return all(bin(int(a) ^ int(b)).count("1") == 1 for a, b in near) and near.size > 0


def random_table(m, seed):
    """2^m finite points with no structure: no split is separable."""
    rng = np.random.default_rng(seed)
    return _c64(rng.normal(size=1 << m), rng.normal(size=1 << m))


def separable_table(pI, pQ):
    """c[v] = (pI[v & (len(pI) - 1)], pQ[v >> log2(len(pI))])."""
    pI, pQ = np.asarray(pI, f32), np.asarray(pQ, f32)
    v = np.arange(pI.size * pQ.size)
    return _c64(pI[v & (pI.size - 1)], pQ[v // pI.size])


def find_split(table):
    """The contract's choice: (mI, pI, pQ) of the separable split with the smallest 2^mI + 2^mQ (the lowest mI on a tie), or
    None."""
    c = np.asarray(table, np.complex64)
    m = c.size.bit_length() - 1
    v = np.arange(c.size)
    best = None
    for k in range(m + 1):
        nI = 1 << k
        if np.array_equal(c.real, c.real[v & (nI - 1)]) and np.array_equal(c.imag, c.imag[(v >> k) << k]):
            cost = nI + (c.size >> k)
            if best is None or cost < best[0]:
                best = (cost, k, c.real[:nI].copy(), c.imag[(np.arange(c.size >> k)) << k].copy())
    return None if best is None else best[1:]


# ------------------------------------------------------------------ the mapper
def ref_map(bits, m, table, word=None, gap=0):
    """bits (frames, E) 0 / 1 -> (frames, P + F + G) complex64: the word, table[v] of every m-bit field (bits beyond E read as
    0), gap zeros."""
    bits = np.asarray(bits, np.uint8)
    frames, E = bits.shape
    F = -(-E // m)
    padded = np.zeros((frames, F * m), np.uint8)
    padded[:, :E] = bits
    v = (padded.reshape(frames, F, m).astype(np.int64) << np.arange(m)).sum(axis=2)
    word = np.zeros(0, np.complex64) if word is None else np.asarray(word, np.complex64)
    out = np.zeros((frames, word.size + F + gap), np.complex64)
    out[:, : word.size] = word
    out[:, word.size: word.size + F] = np.asarray(table, np.complex64)[v]
    return out


def dirty_records(bits, seed):
    """pack_records(bits) with every bit at and beyond E set at random: the mapper must ignore them."""
    bits = np.asarray(bits, np.uint8)
    frames, E = bits.shape
    full = np.random.default_rng(seed).integers(0, 2, (frames, 8 * record_bytes(E)), dtype=np.uint8)
    full[:, E:] |= (np.arange(full.shape[1] - E) % 3 != 1).astype(np.uint8)      # mostly ones, so that a leak shows
    full[:, :E] = bits
    return np.packbits(full, axis=1, bitorder="little")


# ------------------------------------------------------------------ the demapper, by brute force
def distances(z, table):
    """d[n, i] = fl(fl(dx dx) + fl(dy dy)), dx = fl(z.re - c_i.re): (n, 2^m) float32."""
    z = np.asarray(z, np.complex64).ravel()
    c = np.asarray(table, np.complex64)
    with np.errstate(all="ignore"):
        dx = z.real.astype(f32)[:, None] - c.real.astype(f32)[None, :]
        dy = z.imag.astype(f32)[:, None] - c.imag.astype(f32)[None, :]
        return (dx * dx).astype(f32) + (dy * dy).astype(f32)


def _scan_min(d):
    """Minimum along axis 1 by the definition's scan: ascending, replaced on a strictly smaller value only (a NaN stays)."""
    best = d[:, 0].copy()
    idx = np.zeros(d.shape[0], np.int64)
    for i in range(1, d.shape[1]):
        with np.errstate(invalid="ignore"):
            less = d[:, i] < best
        best = np.where(less, d[:, i], best)
        idx = np.where(less, i, idx)
    return best, idx


def ref_index(z, table):
    """(n,) int64: the index of the minimum distance, ties to the lowest index, NaN to 0."""
    return _scan_min(distances(z, table))[1]


def ref_llr(z, table, scale=1.0):
    """(n, m) float32: L_b = fl(s fl(D1_b - D0_b))."""
    c = np.asarray(table, np.complex64)
    m = c.size.bit_length() - 1
    d = distances(z, c)
    out = np.zeros((d.shape[0], m), f32)
    i = np.arange(c.size)
    with np.errstate(all="ignore"):
        for b in range(m):
            d0, _ = _scan_min(d[:, ((i >> b) & 1) == 0])
            d1, _ = _scan_min(d[:, ((i >> b) & 1) == 1])
            out[:, b] = f32(scale) * (d1 - d0).astype(f32)
    return out


def ref_bits_records(z, table, F):
    """z (frames * F,) -> (frames, record_bytes(F m)) uint8: the BITS records."""
    c = np.asarray(table, np.complex64)
    m = c.size.bit_length() - 1
    v = ref_index(z, c).reshape(-1, F)
    bits = ((v[:, :, None] >> np.arange(m)) & 1).astype(np.uint8).reshape(v.shape[0], F * m)
    return pack_records(bits)


def ref_llr_records(z, table, F, scale=1.0):
    c = np.asarray(table, np.complex64)
    m = c.size.bit_length() - 1
    return ref_llr(z, c, scale).reshape(-1, F * m)


def same_floats(a, b):
    """Equality as uint32, NaN matching NaN by position."""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


# ------------------------------------------------------------------ the per-axis identities (what demap_axis_kernel computes)
def _axis_sq(z, p):
    with np.errstate(all="ignore"):
        d = np.asarray(z, f32)[:, None] - np.asarray(p, f32)[None, :]
        return (d * d).astype(f32)


def _fmin(a):
    """IEEE minimum along axis 1 (NaN only where every operand is NaN) -- what fminf gives."""
    with np.errstate(all="ignore"):
        return np.fmin.reduce(a, axis=1)


def axis_llr(z, mI, pI, pQ, scale=1.0):
    z = np.asarray(z, np.complex64).ravel()
    a, b = _axis_sq(z.real, pI), _axis_sq(z.imag, pQ)
    amin, bmin = _fmin(a), _fmin(b)
    mQ = len(pQ).bit_length() - 1
    out = np.zeros((z.size, mI + mQ), f32)
    with np.errstate(all="ignore"):
        for k in range(mI):
            sel = (np.arange(len(pI)) >> k) & 1
            out[:, k] = f32(scale) * ((_fmin(a[:, sel == 1]) + bmin).astype(f32) - (_fmin(a[:, sel == 0]) + bmin).astype(f32)).astype(f32)
        for k in range(mQ):
            sel = (np.arange(len(pQ)) >> k) & 1
            out[:, mI + k] = f32(scale) * ((amin + _fmin(b[:, sel == 1])).astype(f32) - (amin + _fmin(b[:, sel == 0])).astype(f32)).astype(f32)
    return out


def axis_index(z, mI, pI, pQ):
    """D = fl(a_min + b_min); j* the lowest j with fl(a_min + b_j) == D; i* the lowest i with fl(a_i + b_j*) == D."""
    z = np.asarray(z, np.complex64).ravel()
    a, b = _axis_sq(z.real, pI), _axis_sq(z.imag, pQ)
    with np.errstate(all="ignore"):
        amin, bmin = _fmin(a), _fmin(b)
        D = (amin + bmin).astype(f32)
        hit_j = (amin[:, None] + b).astype(f32) == D[:, None]
        js = np.argmax(hit_j, axis=1)                                           # the first True; 0 where there is none (NaN)
        bs = b[np.arange(z.size), js]
        hit_i = (a + bs[:, None]).astype(f32) == D[:, None]
        i_s = np.argmax(hit_i, axis=1)
    return np.where(np.isnan(D), 0, i_s | (js << mI))


def naive_axis_index(z, mI, pI, pQ):
    """The per-axis argmin, which is NOT the definition's index."""
    z = np.asarray(z, np.complex64).ravel()
    return _scan_min(_axis_sq(z.real, pI))[1] | (_scan_min(_axis_sq(z.imag, pQ))[1] << mI)


# ------------------------------------------------------------------ inputs
def adversarial(table, n, seed):
    """n symbols of the kind on which a careless demapper goes wrong: magnitudes over e^+-20, midpoints between points (exact
    ties and near ties), points scaled by 2^10 ... 2^29 (distances that round together), NaN, +-inf, +-0 and subnormals."""
    c = np.asarray(table, np.complex64)
    rng = np.random.default_rng(seed)
    k = n // 8
    parts = []
    mag = np.exp(rng.uniform(-20, 20, k))
    parts.append(mag * np.exp(2j * np.pi * rng.uniform(size=k)))
    i, j = rng.integers(0, c.size, k), rng.integers(0, c.size, k)
    mid = (c[i].astype(np.complex128) + c[j].astype(np.complex128)) / 2
    parts.append(mid)                                                           # midpoints: ties
    parts.append(mid + rng.normal(size=k) * 1e-7 + 1j * rng.normal(size=k) * 1e-7)
    parts.append(c[rng.integers(0, c.size, k)].astype(np.complex128) * (2.0 ** rng.integers(10, 30, k)))
    parts.append(c.real[rng.integers(0, c.size, k)] * (2.0 ** rng.integers(10, 30, k)) + 1j * c.imag[rng.integers(0, c.size, k)])
    parts.append(c[rng.integers(0, c.size, k)] + (rng.normal(size=k) + 1j * rng.normal(size=k)) * 0.3 * np.abs(c).max() / np.sqrt(c.size))
    grid = rng.integers(-40, 41, k) / 8.0 + 1j * rng.integers(-40, 41, k) / 8.0   # a coarse lattice: many exact ties
    parts.append(grid * max(float(np.abs(c).max()), 1e-30) / 4.0)
    z = np.concatenate(parts).astype(np.complex64)
    sub = np.float32(1e-45)
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, sub, -sub, 3e-39, 1.0, -1.0, 3e38, -3e38], f32)
    re, im = np.meshgrid(special, special)
    sp = np.empty(re.size, np.complex64)
    sp.real, sp.imag = re.ravel(), im.ravel()                                   # (re + 1j * im would turn inf + j nan into nan)
    out = np.concatenate([z, np.resize(sp, n - z.size)]) if n - z.size > 0 else z[:n]
    return np.ascontiguousarray(out[rng.permutation(out.size)], np.complex64)


def noisy_points(table, n, seed, sigma=0.25):
    c = np.asarray(table, np.complex64)
    rng = np.random.default_rng(seed)
    step = np.abs(c).max() / np.sqrt(c.size)
    return (c[rng.integers(0, c.size, n)] + sigma * step * (rng.normal(size=n) + 1j * rng.normal(size=n))).astype(np.complex64)


def demap_input(table, n, seed):
    """Half noisy table points, half the adversarial set."""
    return np.concatenate([noisy_points(table, n - n // 2, seed), adversarial(table, n // 2, seed + 1)])


@functools.lru_cache(maxsize=None)
def tables():
    """name -> (m, table or None for digital.rs's, the split (mI, mQ) the library must choose or None for the table form)."""
    rng = np.random.default_rng(77)
    levels8 = np.sort(rng.normal(size=8)).astype(f32)
    return {
        "bpsk": (1, None, (1, 0)),
        "qpsk": (2, None, (1, 1)),
        "8psk": (3, psk_table(3), None),
        "16qam": (4, qam_table(4), (2, 2)),
        "64qam": (6, qam_table(6, 0.5), (3, 3)),
        "256qam": (8, qam_table(8), (4, 4)),
        "rand3": (3, random_table(3, 3), None),
        "rand5": (5, random_table(5, 5), None),
        "rand8": (8, random_table(8, 8), None),
        "sep32": (5, separable_table(rng.permutation(8).astype(f32) - 3.5, [0.75, -2.0, 2.5, -0.25]), (3, 2)),   # not Gray
        "re8": (3, separable_table(levels8, [0.25]), (3, 0)),
        "im8": (3, separable_table([-0.5], levels8), (0, 3)),
    }


def table_of(name):
    m, t, split = tables()[name]
    return m, (default_table(m) if t is None else t), t, split


def demap_lengths(m):
    """F: one symbol; F m no multiple of 32; F m one below and one above a multiple of 32 where m allows it (otherwise the
    nearest F on either side); more than one 64-symbol chunk."""
    want = {1, 67}
    for target in (63, 65, 31 + 32 * m, 33 + 32 * m):
        want.add(max(1, target // m))
        want.add(-(-target // m))
    return sorted(want)


# ------------------------------------------------------------------ the coded link of tests/test_gpu_symmap.py
# CRC-24 -> K = 7 encoder -> rate 3/4 matcher -> 16-QAM mapper behind a 13-symbol word; noise and a constant rotation on the
# host; frame synchroniser -> deframer (C32, normalising) -> demapper -> dematcher -> Viterbi -> CRC check
LINK_FRAMES = 40
LINK_T = 100                                    # information bits per frame
LINK_M = 4
LINK_GAP = 5
LINK_SIGMA = 0.32                               # per component at the table's scale (minimum distance 2): chosen on the CPU,
LINK_SEED = 2027                                # test_symmap_ref.py decodes every frame of the reference chain at it
LINK_GAIN = 0.35 * np.exp(0.9j)                 # the channel's constant gain and rotation
LINK_QSCALE = 0.5                               # |L| = |D1 - D0| / (2 sigma^2) reaches about 80: q stays mostly off the clamp
LINK_WORD = (3.0 * np.array([1, 1, 1, 1, 1, -1, -1, 1, 1, -1, 1, -1, 1])).astype(np.complex64)   # Barker 13 at the outer level
LINK_THRESHOLD, LINK_GUARD = 0.8, 12


def link_format():
    import crc_ref as cr
    import ratematch_ref as rr
    import viterbi_ref as vr

    p = cr.CATALOGUE["CRC24A"][0]
    info = LINK_T + p.W                                                     # 124 bits into the encoder
    N = 2 * vr.n_steps(info, 7, True)                                       # 260 coded bits
    pattern = rr.PATTERNS["3/4"]
    src, _ = rr.build_map(N, pattern)
    E = src.size
    F = -(-E // LINK_M)
    return dict(p=p, info=info, N=N, pattern=pattern, src=src, E=E, F=F, rec=LINK_WORD.size + F + LINK_GAP)


def link_transmit():
    """The transmit side on the references: payload bits, framed bits, coded bits, matched bits, symbols (frames, rec)."""
    import crc_ref as cr
    import ratematch_ref as rr
    import viterbi_ref as vr

    f = link_format()
    payload = np.random.default_rng(LINK_SEED).integers(0, 2, (LINK_FRAMES, LINK_T), dtype=np.uint8)
    framed = cr.ref_attach(payload, f["p"])
    coded = vr.ref_encode(framed, 7, vr.GENS[(7, 2)])
    sent = rr.ref_tx(coded, f["src"])
    sym = ref_map(sent, LINK_M, qam_table(LINK_M), LINK_WORD, LINK_GAP)
    return payload, framed, coded, sent, sym


def link_channel(sym):
    """The stream the receiver sees: the frames back to back, the gain and rotation, then the seeded noise (scaled by |gain|, so
    that it is LINK_SIGMA at the table's scale once the deframer has normalised)."""
    rng = np.random.default_rng(LINK_SEED + 1)
    x = np.asarray(sym, np.complex64).ravel().astype(np.complex128) * LINK_GAIN
    noise = LINK_SIGMA * abs(LINK_GAIN) * (rng.normal(size=x.size) + 1j * rng.normal(size=x.size))
    return (x + noise).astype(np.complex64)


def link_receive(z):
    """The receive side behind the deframer on the references: z (frames, F) complex64 -> llr, dematched words, decoded bits,
    (payload, passed, crc)."""
    import crc_ref as cr
    import ratematch_ref as rr
    import viterbi_ref as vr

    f = link_format()
    llr = ref_llr_records(np.asarray(z, np.complex64).ravel(), qam_table(LINK_M), f["F"], 0.5 / LINK_SIGMA ** 2)
    words = rr.ref_rx(llr.view(np.uint32), f["src"], f["N"])
    decoded, _ = vr.ref_decode(vr.ref_quantise(words.view(np.float32), LINK_QSCALE), 7, vr.GENS[(7, 2)], f["info"])
    return llr, words, decoded, cr.ref_check(decoded, f["p"], LINK_T)
