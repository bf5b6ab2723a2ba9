"""Reference of the seeded noise source and the AWGN node (include/comms_hip.h, "seeded noise source"): numpy, f64
arithmetic from the integer words.  Written from the contract, not from the kernels:

  block b of (seed, stream) = Philox4x32-10, key (seed lo32, seed hi32), counter (b lo32, b hi32, stream lo32, stream hi32)
  -> stream words 4b ... 4b+3; a Source holds a position in words and the four draw kinds consume from it.

Also the small BPSK / QPSK links the bit-error-rate tests compare with.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
MASK64 = (1 << 64) - 1


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (or ints), key: two ints -> four uint32 arrays."""
    c = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) for x in ctr]
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    for _ in range(10):
        p0 = c[0] * np.uint64(M0)  # 32 x 32 -> 64 bit, exact in uint64
        p1 = c[2] * np.uint64(M1)
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK32)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK32)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return [x.astype(np.uint32) for x in c]


def words(seed, stream, pos, n):
    """Stream words pos ... pos + n - 1 (uint32)."""
    pos, n = int(pos) & MASK64, int(n)
    if n == 0:
        return np.zeros(0, np.uint32)
    b0, b1 = pos >> 2, (pos + n + 3) >> 2
    b = (np.arange(b1 - b0, dtype=np.uint64) + np.uint64(b0)) & np.uint64((1 << 62) - 1)  # word 2^64 - 1 is followed by word 0
    out = philox4x32_10([b & np.uint64(MASK32), b >> np.uint64(32), int(stream) & MASK32, (int(stream) >> 32) & MASK32],
                        [int(seed) & MASK32, (int(seed) >> 32) & MASK32])
    w = np.stack(out, 1).reshape(-1)
    off = pos - (b0 << 2)
    return w[off:off + n]


def _u24(w):
    return (w >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


def std_normal_at(seed, stream, pos, n):
    """f64 standard normal values at stream words pos ... pos + n - 1 (the pair rule of the contract)."""
    pos, n = int(pos), int(n)
    p0 = pos & ~1
    m = ((pos + n + 1) & ~1) - p0
    w = words(seed, stream, p0, m)
    a, b = w[0::2], w[1::2]
    u1 = ((a >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = _u24(b)
    r = np.sqrt(-2.0 * np.log(u1))
    z = np.empty(m, np.float64)
    z[0::2] = r * np.cos(2.0 * np.pi * u2)
    z[1::2] = r * np.sin(2.0 * np.pi * u2)
    return z[pos - p0:pos - p0 + n]


class Source:
    """The position rules of a comms_noise handle."""

    def __init__(self, seed, stream=0, pos=0):
        self.seed, self.stream, self.pos = int(seed), int(stream), int(pos)

    def skip(self, n_words):
        self.pos = (self.pos + int(n_words)) & MASK64
        return self

    def bits(self, n, packed=False):
        n = int(n)
        nw = (n + 31) // 32
        w = words(self.seed, self.stream, self.pos, nw)
        self.skip(nw)
        b = np.unpackbits(w.astype("<u4").view(np.uint8), bitorder="little")[:n]
        return np.packbits(b, bitorder="little") if packed else b

    def uniform(self, n, lo=0.0, hi=1.0):
        """f64 values lo + (hi - lo) u, and the f32 the contract returns: rounded once, hi replaced by the float below it."""
        lo32, hi32 = np.float32(lo), np.float32(hi)
        u = _u24(words(self.seed, self.stream, self.pos, n))
        self.skip(n)
        exact = np.float64(lo32) + (np.float64(hi32) - np.float64(lo32)) * u
        f = exact.astype(np.float32)
        f[f >= hi32] = np.nextafter(hi32, np.float32(-np.inf))
        return exact, f

    def normal(self, n, mu=0.0, sd=1.0):
        z = std_normal_at(self.seed, self.stream, self.pos, n)
        self.skip(n)
        return mu + sd * z

    def complex_normal(self, n):
        """n complex standard pairs (z + i z'), after the advance to an even word."""
        self.pos = (self.pos + 1) & ~1 & MASK64
        z = std_normal_at(self.seed, self.stream, self.pos, 2 * n)
        self.skip(2 * n)
        return z[0::2] + 1j * z[1::2]

    def awgn(self, x, sigma):
        x = np.asarray(x, np.complex128)
        return x + float(sigma) * self.complex_normal(x.size)


# ---- bit-error-rate links ------------------------------------------------------------------------------------------
def symbol_link_bpsk(n_bits, ebn0_db, seed, stream=0):
    """Symbol-level BPSK over AWGN: bits from the source's bit draw, s = 1 - 2b, y = s + sigma z, b^ = y < 0.
    Returns (errors, n_bits, sigma).  Es = Eb = 1, N0 = 2 sigma^2."""
    src = Source(seed, stream)
    b = src.bits(n_bits)
    sigma = np.sqrt(1.0 / (2.0 * 10.0 ** (ebn0_db / 10.0)))
    y = (1.0 - 2.0 * b) + sigma * src.normal(n_bits)
    return int(np.count_nonzero((y < 0) != (b == 1))), n_bits, sigma


def map_symbols(bits, k, table):
    """Stream bits (0 / 1 array) -> symbols: value v = the next k bits, the first as the LSB -> table[v]."""
    bits = np.asarray(bits, np.int64)
    n_sym = bits.size // k
    v = bits[:n_sym * k].reshape(n_sym, k) @ (1 << np.arange(k))
    return np.asarray(table, np.complex128)[v], v


BPSK = np.array([1, -1], np.complex128)                        # digital.rs bpsk_bit_mod: bit -> re < 0
QPSK = np.array([1 + 1j, -1 + 1j, 1 - 1j, -1 - 1j], np.complex128)  # qpsk_bit_mod: bit 0 -> re < 0, bit 1 -> im < 0


def tx_wire(bits, k, taps, sps, tx_scale):
    """bits -> BPSK / QPSK symbols -> zero-stuffed pulse filter at `sps` samples per symbol -> (tx_scale * y) truncated toward
    zero: the i16 pairs IQOutput writes, as an (n, 2) int16 array."""
    sym, _ = map_symbols(bits, k, BPSK if k == 1 else QPSK)
    up = np.zeros(sym.size * sps, np.complex128)
    up[::sps] = sym
    y = np.convolve(up, np.asarray(taps, np.float64))[:up.size] * tx_scale
    return np.stack([np.trunc(y.real), np.trunc(y.imag)], 1).astype(np.int16)


def sample_link(bits, k, taps, sps, tx_scale, sigma, noise, wire=None, rx_scale=None):
    """The sample-level link: bits -> RRC pulse, sps samples per symbol -> scale (i16 wire, tx_wire; `wire` replaces it
    by recorded wire samples) -> times rx_scale (default 1 / tx_scale, as the f32 product comms_iq_i16_to_c32 forms),
    + sigma * noise -> matched FIR (the same taps) -> keep every sps-th
    -> per-axis sign (bit = component < 0).  The decision variable of symbol j is decimated sample j + delay with
    delay = (n_taps - 1) / sps, the group delay of the two filters in symbols.
    Returns (errors, n_compared_bits, d): d the (n_compared_symbols, k) decision variables, and the error count over the
    symbols that have one."""
    taps = np.asarray(taps, np.float64)
    assert (taps.size - 1) % sps == 0
    delay = (taps.size - 1) // sps
    bits = np.asarray(bits, np.int64)
    if wire is None:
        wire = tx_wire(bits, k, taps, sps, tx_scale)
    rx_scale = np.float32(1.0 / tx_scale if rx_scale is None else rx_scale)
    wire = (np.asarray(wire).reshape(-1, 2).astype(np.float32) * rx_scale).astype(np.float64)
    rx = (wire[:, 0] + 1j * wire[:, 1]) + sigma * np.asarray(noise, np.complex128)[:wire.shape[0]]
    y = np.convolve(rx, taps)[:rx.size][::sps]
    d = y[delay:]
    d = np.stack([d.real, d.imag], 1)[:, :k]
    sent = bits[:d.shape[0] * k].reshape(-1, k)
    errors = int(np.count_nonzero((d < 0) != (sent == 1)))
    return errors, d.size, d


# ---- the link of tests/test_gpu_noise.py (its parameters live here so that the CPU test can check the noise levels)
LINK_SPS, LINK_TAPS, LINK_BETA = 8, 65, 0.35
LINK_SIGMAS = (1.5, 1.0)  # per-component noise at unit symbol amplitude: bit-error rates near 3e-2 and 2e-3


def link_scale(h, k):
    """The i16 wire scale: the largest that cannot saturate, with 1 % to spare."""
    amp = np.sqrt(2.0) if k == 2 else 1.0
    return float(np.floor(32767.0 / (np.sum(np.abs(h)) * amp * 1.01)))


def link_delta(h, sigma, noise, rx_max, acc, tol):
    """How far a device decision variable may lie from the reference's: every received sample within the AWGN bound
    (sigma * acc * max(1, |z|) + 2^-23 |sample|, taken at the largest |z| and the largest sample), through a filter of these
    taps, plus the chain's own parity tolerance tol * sum|taps| * max|x|."""
    zmax = max(1.0, float(np.max(np.abs(noise.real))), float(np.max(np.abs(noise.imag))))
    sum_h = float(np.sum(np.abs(h)))
    return sum_h * (sigma * acc * zmax + 2.0 ** -23 * rx_max) + tol * sum_h * rx_max
