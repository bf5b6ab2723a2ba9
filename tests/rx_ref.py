"""numpy reference of the receive end's hard decisions (test infrastructure, no GPU): the rule of include/comms_hip.h

  d_i = dx*dx + dy*dy, dx = y.re - c_i.re, dy = y.im - c_i.im, in f32 with every operation rounded on its own (numpy
  float32 arithmetic never fuses a multiply-add); i ascending, replaced only on a strictly smaller d -- ties to the
  lowest index, NaN to index 0;

and the COMMS_SYM_BITS packing: value v of symbol j at stream bits j*k ... j*k + k - 1 (LSB first; stream bit i = bit
i%8 of byte i/8), bits past n*k in the last byte zero.
"""
import numpy as np

BPSK_DEF = np.array([1, -1], np.complex64)                             # digital.rs bpsk_bit_mod (the NULL table)
QPSK_DEF = np.array([1 + 1j, -1 + 1j, 1 - 1j, -1 - 1j], np.complex64)  # digital.rs qpsk_bit_mod
BPSK_EX = np.array([-1, 1], np.complex64)                              # 2b - 1 (examples/single_thread_bpsk.rs)
QPSK_EX = np.array([-1 - 1j, 1 - 1j, -1 + 1j, 1 + 1j], np.complex64)   # (2x - 1, 2y - 1) (examples/single_thread_qpsk.rs)
TABLES = {"bpsk_def": (1, BPSK_DEF), "qpsk_def": (2, QPSK_DEF), "bpsk_ex": (1, BPSK_EX), "qpsk_ex": (2, QPSK_EX)}


def default_table(k):
    return BPSK_DEF if k == 1 else QPSK_DEF


def dist(y, c):
    """f32 squared distances of the symbols y to one point c, each operation rounded."""
    y = np.asarray(y, np.complex64)
    with np.errstate(over="ignore", invalid="ignore"):
        dx = y.real.astype(np.float32) - np.float32(np.real(c))
        dy = y.imag.astype(np.float32) - np.float32(np.imag(c))
        return (dx * dx) + (dy * dy)


def decide(y, constellation):
    """Index of the nearest point per symbol (int64), by the header's rule."""
    c = np.asarray(constellation, np.complex64).ravel()
    y = np.asarray(y, np.complex64).ravel()
    v = np.zeros(y.size, np.int64)
    best = dist(y, c[0])
    for i in range(1, c.size):
        d = dist(y, c[i])
        m = d < best  # NaN compares false: a NaN symbol keeps index 0
        v[m] = i
        best = np.where(m, d, best)
    return v


def pack(v, k):
    """Values (k bits each) -> packed bytes, LSB first, zero tail bits."""
    v = np.asarray(v, np.int64).ravel()
    bits = ((v[:, None] >> np.arange(k)) & 1).astype(np.uint8).ravel()
    return np.packbits(bits, bitorder="little")


def unpack_values(packed, n_sym, k):
    bits = np.unpackbits(np.asarray(packed, np.uint8), bitorder="little")[: n_sym * k].reshape(n_sym, k).astype(np.int64)
    return (bits << np.arange(k)).sum(axis=1)


def sym_to_bits(y, k, constellation=None):
    """What comms_sym_to_bits writes for the symbols y."""
    return pack(decide(y, default_table(k) if constellation is None else constellation), k)


def bit_errors(a, b, n_bits):
    ua = np.unpackbits(np.asarray(a, np.uint8), bitorder="little")[:n_bits]
    ub = np.unpackbits(np.asarray(b, np.uint8), bitorder="little")[:n_bits]
    return int(np.count_nonzero(ua != ub))
