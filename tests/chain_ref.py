"""A float64 reference of the chain node (comms_chain_*): the reference nodes in series in double precision --
MixerNode -> BatchFirNode -> DecimateNode [-> FMDemodNode], or BatchFirNode -> MixerNode -> DecimateNode --
from any initial FIR state, oscillator phase and FM.prev, one call at a time with the state carried as the reference
nodes carry it (src/filter/fir_node.rs:193-220, src/mixer.rs:79-82, src/modulation/analog.rs:9,31).

Every call's length is a multiple of the rate, so DecimateNode's restart per batch (src/util/resample_node.rs:53-65)
keeps the stream samples 0, R, 2R, ...: the helper computes only those outputs, as R-wide rows of the stream times a
tap matrix per row offset (complex128 matrix-vector products), in chunks that keep host memory to a few hundred MB.
Shared by tests/test_chain_ref.py (checked against the oracle on the CPU) and tests/test_gpu_chain_handover.py."""
from fractions import Fraction
import math

import numpy as np

MIX_T = 2.0 * math.pi   # one turn of the oscillator, as the library's fixed-point phase counts it
CHUNK = 1 << 22         # input samples per step of the reference


def wrap_dphase(dphase):
    """The mixer's step reduced to [0, 2 pi) (mix_wrap_dphase): the same rotation."""
    return float(Fraction(dphase) % Fraction(MIX_T))


def closed_form_phase(phase0, dphase, n):
    """Oscillator phase after n samples, (phase0 + n dphase) mod 2 pi, computed exactly in rationals."""
    return float((Fraction(phase0) + n * Fraction(wrap_dphase(dphase))) % Fraction(MIX_T))


def circ(d):
    """Distance on the circle."""
    return np.abs((np.asarray(d, np.float64) + np.pi) % (2 * np.pi) - np.pi)


class ChainRef:
    """The chain in f64.  `state`: the FIR history as comms_chain_set_fir_state takes it (raw input samples, newest
    first; with the mixer in front the FIR node's own history is then these samples mixed with the phases of samples
    -1, -2, ...); `phase0`: the oscillator phase of the first sample of the first call; `fm_prev`: FM.prev."""

    def __init__(self, taps, rate, dphase, phase0, fm, after, state=None, fm_prev=0j):
        self.h = np.asarray(taps, np.complex128)
        self.n_taps, self.rate = self.h.size, int(rate)
        self.dphase, self.phase0 = float(dphase), float(phase0)
        self.fm, self.after = bool(fm), bool(after)
        # raw history, OLDEST first: the last n_taps input samples (only the newest n_taps - 1 enter an output)
        hist = np.zeros(self.n_taps, np.complex128)
        if state is not None:
            st = np.asarray(state, np.complex128)
            assert st.size == self.n_taps
            hist = st[::-1].copy()
        self.hist = hist
        self.count = 0                       # input samples so far (the stream index of the next one)
        self.fm_prev = complex(fm_prev)
        self.last_y = None                   # the last decimated filter output (what FM.prev becomes)
        R, N = self.rate, self.n_taps
        self.D = (N - 1 + R - 1) // R        # row offsets of the tap matrix beyond 0
        self.P = R * self.D - (N - 1)        # zeros in front of the history: output j sits at row D + j
        G = np.zeros((self.D + 1, R), np.complex128)
        for d in range(self.D + 1):
            for c in range(R):
                k = R * d - c
                if 0 <= k < N:
                    G[d, c] = self.h[k]
        self.G = G

    def _rot(self, first, n, step=1):
        idx = first + step * np.arange(n, dtype=np.float64)
        return np.exp(1j * (self.phase0 + self.dphase * idx))

    def _chunk(self, x):
        R, N, n = self.rate, self.n_taps, x.size
        ext = np.concatenate([np.zeros(self.P, np.complex128), self.hist[1:], x])
        if not self.after:   # the mixer in front: every sample the FIR reads is mixed with its own phase
            ext[self.P:] *= self._rot(self.count - (N - 1), N - 1 + n)
        rows = ext.reshape(-1, R)
        n_out = n // R
        y = np.zeros(n_out, np.complex128)
        for d in range(self.D + 1):
            y += rows[self.D - d:self.D - d + n_out] @ self.G[d]
        if self.after:       # the mixer behind the FIR: the kept outputs only, each with its sample's phase
            y *= self._rot(self.count, n_out, R)
        self.hist = np.concatenate([self.hist, x])[-N:]
        self.count += n
        self.last_y = y[-1]
        if not self.fm:
            return y, y
        prev = np.concatenate([[self.fm_prev], y[:-1]])
        self.fm_prev = complex(y[-1])
        return np.angle(y * np.conj(prev)), y

    def run(self, x):
        """One call of the chain on x (len a multiple of the rate).  Returns (out, y): the chain's outputs (angles with
        FM demod) and the decimated filter outputs they come from, both float64 / complex128."""
        x = np.asarray(x)
        assert x.size % self.rate == 0 and x.size > 0
        step = max(self.rate, CHUNK - CHUNK % self.rate)
        outs, ys = [], []
        for a in range(0, x.size, step):
            o, y = self._chunk(x[a:a + step].astype(np.complex128))
            outs.append(o)
            ys.append(y)
        return np.concatenate(outs), np.concatenate(ys)

    def state(self, k=None):
        """The raw FIR history, newest first (comms_chain_get_fir_state)."""
        return self.hist[::-1][: self.n_taps if k is None else k]

    def phase(self):
        return closed_form_phase(self.phase0, self.dphase, self.count)


def out_bound(taps, x_max):
    """Decimated outputs: max|d| <= 2e-5 * sum|h| * max|x| (the FIR's error plus the mixer's rounding of it)."""
    return 2e-5 * float(np.sum(np.abs(taps))) * x_max


def check_outputs(got, want, y, prev, taps, x_max, fm, what=""):
    """got (the chain's outputs) against the f64 reference: every output, from the first.  FM: the angle's error on the
    circle weighted by the smaller magnitude of the two samples it is the argument of (y[j], y[j-1], y[-1] = prev)."""
    got = np.asarray(got)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if fm:
        mag = np.minimum(np.abs(y), np.abs(np.concatenate([[prev], y[:-1]])))
        d = circ(got.astype(np.float64) - want) * mag
        bound = 2 * out_bound(taps, x_max)
    else:
        d = np.abs(got.astype(np.complex128) - want)
        bound = out_bound(taps, x_max)
    k = int(np.argmax(d))
    assert d[k] <= bound, (what, "output", k, "of", d.size, float(d[k]), bound)
