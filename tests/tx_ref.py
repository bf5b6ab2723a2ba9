"""Pure-Python / numpy reference of the transmit front end (test infrastructure, no GPU):

  PrnGen<T> of src/prns.rs:64-71 for an unsigned register of W = 8, 16, 32 or 64 bits
      out = state >> (W-1);  fb = popcount(state & mask) & 1;  state = ((state << 1) | fb) mod 2^W
  its GF(2) jump (one step is S' = A S, A a W x W matrix: row 0 = mask, row i = bit i-1), and
  the digital.rs modulators (bpsk/qpsk _bit_mod / _byte_mod) on Complex<i16> as int16 (n, 2).

Matrices are lists of W row words (Python ints); y = A s has bit i = parity(row_i & s).
"""
import numpy as np

WIDTHS = (8, 16, 32, 64)


def wmask(w):
    return (1 << w) - 1


def step(mask, state, w):
    """One PrnGen::next_byte: (bit, new_state)."""
    out = state >> (w - 1)
    fb = bin(state & mask).count("1") & 1
    return out, ((state << 1) | fb) & wmask(w)


def prns_serial(mask, state, n, w):
    """n bits by plain stepping: (uint8 bits, final state)."""
    bits = np.empty(n, np.uint8)
    for i in range(n):
        bits[i], state = step(mask, state, w)
    return bits, state


# ---- GF(2) algebra
def step_matrix(mask, w):
    return [mask] + [1 << (i - 1) for i in range(1, w)]


def identity(w):
    return [1 << i for i in range(w)]


def matvec(rows, s):
    y = 0
    for i, r in enumerate(rows):
        y |= (bin(r & s).count("1") & 1) << i
    return y


def matmul(x, y):
    """X Y: row i = XOR of rows j of Y with X_ij = 1."""
    out = []
    for r in x:
        acc, j = 0, 0
        while r:
            if r & 1:
                acc ^= y[j]
            r >>= 1
            j += 1
        out.append(acc)
    return out


class Jump:
    """A^(2^i) for i < 64: the state n steps ahead in popcount(n) mat-vecs."""

    def __init__(self, mask, w):
        self.w = w
        self.pw = [step_matrix(mask, w)]
        for _ in range(63):
            self.pw.append(matmul(self.pw[-1], self.pw[-1]))

    def skip(self, state, n):
        i = 0
        while n:
            if n & 1:
                state = matvec(self.pw[i], state)
            n >>= 1
            i += 1
        return state

    def power(self, n):
        """A^n as a matrix."""
        m = identity(self.w)
        i = 0
        while n:
            if n & 1:
                m = matmul(self.pw[i], m)
            n >>= 1
            i += 1
        return m


def is_maximal(mask, w, prime_factors):
    """Order test: A^(2^w - 1) = I and A^((2^w - 1) / p) != I for every prime p of 2^w - 1."""
    j = Jump(mask, w)
    per = (1 << w) - 1
    if j.power(per) != identity(w):
        return False
    return all(j.power(per // p) != identity(w) for p in prime_factors)


# ---- vectorised generation (many streams in parallel, jump-started): for long sequences
def _parity64(x):
    return (np.bitwise_count(x) & np.uint64(1)).astype(np.uint64)


def _matvec_np(rows, s):
    y = np.zeros_like(s)
    for i, r in enumerate(rows):
        y |= _parity64(s & np.uint64(r)) << np.uint64(i)
    return y


def _rev_w(s, w):
    """bit-reverse of the low w bits of each element (uint64 array)."""
    out = np.zeros_like(s)
    for i in range(w):
        out |= ((s >> np.uint64(i)) & np.uint64(1)) << np.uint64(w - 1 - i)
    return out


def prns_packed(mask, state, n, w, streams=4096):
    """n bits packed LSB first (ceil(n/8) bytes, trailing bits 0), computed from `streams` jump-started streams of
    W bits per step: the next W outputs of a state are its bits, most significant first."""
    n_steps_total = (n + w - 1) // w
    per = max(1, (n_steps_total + streams - 1) // streams)   # steps (of W bits) per stream
    m = (n_steps_total + per - 1) // per
    j = Jump(mask, w)
    starts = np.empty(m, np.uint64)
    s, jump = state, j.power(per * w)
    for k in range(m):
        starts[k] = s
        s = matvec(jump, s)
    aw = j.pw[{8: 3, 16: 4, 32: 5, 64: 6}[w]]
    chunks = np.empty((m, per), np.uint64)
    cur = starts.copy()
    for t in range(per):
        chunks[:, t] = _rev_w(cur, w)
        cur = _matvec_np(aw, cur)
    # chunk (k, t) holds W stream bits, stream bit b of the chunk at bit b
    flat = chunks.reshape(-1)
    nbytes_w = w // 8
    by = np.empty((flat.size, nbytes_w), np.uint8)
    for b in range(nbytes_w):
        by[:, b] = ((flat >> np.uint64(8 * b)) & np.uint64(0xFF)).astype(np.uint8)
    out = by.reshape(-1)[:(n + 7) // 8].copy()
    if n % 8:
        out[-1] &= (1 << (n % 8)) - 1
    return out


def unpack(packed, n):
    return np.unpackbits(packed, bitorder="little")[:n]


def pack(bits):
    return np.packbits(np.asarray(bits, np.uint8), bitorder="little")


# ---- digital.rs
BPSK = np.array([[1, 0], [-1, 0]], np.int16)
QPSK = np.array([[1, 1], [-1, 1], [1, -1], [-1, -1]], np.int16)


def bpsk_bit_mod(v):
    return None if v > 1 else BPSK[v]


def qpsk_bit_mod(v):
    return None if v > 3 else QPSK[v]


def bpsk_byte_mod(x):
    x = np.asarray(x, np.uint8).ravel()
    bits = (x[:, None] >> np.arange(8, dtype=np.uint8)) & 1
    return BPSK[bits.reshape(-1)]


def qpsk_byte_mod(x):
    x = np.asarray(x, np.uint8).ravel()
    v = (x[:, None] >> (2 * np.arange(4, dtype=np.uint8))) & 3
    return QPSK[v.reshape(-1)]


def map_bits(packed, n_sym, k, constellation):
    """Symbol i = constellation[v], v = stream bits k i .. k i + k - 1 (first = LSB): the COMMS_SYM_BITS rule."""
    bits = unpack(np.asarray(packed, np.uint8), n_sym * k).reshape(n_sym, k).astype(np.int64)
    v = (bits << np.arange(k)).sum(axis=1)
    return np.asarray(constellation, np.complex64)[v]
