"""A float64 reference of the symbol synchroniser (comms_symsync_*): the formula of include/comms_hip.h, call by call, with
its history of Q = (N - 1) // L raw input samples, the timing offset mu and the rotor phase carried across calls --

    y[k]   = sum_{j >= 0, p + L j < N} h[p + L j] x[k S + q - j],     p = mu mod L,  q = mu div L,   0 <= mu < S L
    out[k] = y[k] exp(+i (phase + k dphase))                          (Mixer::mix, src/mixer.rs:73-84)

which is what UpsampleNode(L) -> BatchFirNode(taps) -> skip mu -> DecimateNode(L S) -> MixerNode give in series, without the
products with stuffed zeros and the outputs that are dropped -- and the decision step, by way of rx_ref.
Also the relation between TimingEstimator::push and the node's tau (tau_from_estimate), which tests/test_symsync_ref.py pins.
Shared by tests/test_symsync_ref.py (pinned to the oracle's composition on the CPU) and tests/test_gpu_symsync.py."""
import numpy as np

import rx_ref

TWO_PI = 2.0 * np.pi


def out_len(n, sps):
    return n // max(int(sps), 1)


def state_len(n_taps, phases):
    return (n_taps - 1) // max(int(phases), 1)


def mu_of(tau, phases, sps):
    """comms_symsync_set_timing: floor-mod(llround(tau L), S L); llround rounds halves away from zero."""
    L, S = max(int(phases), 1), max(int(sps), 1)
    t = tau * L
    r = int(np.floor(abs(t) + 0.5)) * (1 if t >= 0 else -1)
    return r % (S * L)


def tau_from_estimate(e, n_taps, phases, sps):
    """The tau that puts the node's sample on the symbol centre, from TimingEstimator::push's return value e (estimator at
    n = sps) and the node's prototype of n_taps taps (odd, centred) over `phases` phases: e is the position of the symbol
    peaks in the call, mod sps, and the filter delays by (n_taps - 1) / (2 phases) input samples (include/comms_hip.h,
    comms_symsync_set_timing)."""
    return (e + (n_taps - 1) / (2.0 * phases)) % sps


# |e - c| of that relation over the CPU sweeps of tests/test_symsync_ref.py, in input samples
ESTIMATE_ACCURACY = 0.003


class SymSyncRef:
    def __init__(self, taps, phases, sps):
        h = np.asarray(taps, np.float64)
        assert h.ndim == 1 and h.size >= 1
        self.L, self.S, self.N = max(int(phases), 1), max(int(sps), 1), h.size
        self.Q = (self.N - 1) // self.L
        QP = self.Q + 1
        tab = np.zeros(self.L * QP, np.float64)          # tab[p][j] = h[p + L j]
        tab[: self.N] = h
        self.tab = tab.reshape(QP, self.L).T.copy()
        self.hist = np.zeros(self.Q, np.complex64)       # the last Q input samples, OLDEST first
        self.mu = 0
        self.phase, self.dphase = 0.0, 0.0
        self.x_max = 0.0
        self.bits, self.table = 0, None

    def set_timing(self, tau):
        self.mu = mu_of(tau, self.L, self.S)

    def set_rotation(self, dphase, phase=0.0):
        self.dphase, self.phase = float(dphase) % TWO_PI, float(phase) % TWO_PI

    def set_output(self, bits_per_sym=None, constellation=None):
        self.bits = int(bits_per_sym or 0)
        self.table = None if not self.bits else rx_ref.default_table(self.bits) if constellation is None else constellation

    def run_c(self, x):
        """One call: n / S outputs in complex128 (whatever the output format)."""
        x = np.ascontiguousarray(x, dtype=np.complex64)
        L, S, Q = self.L, self.S, self.Q
        assert x.size % S == 0
        n_out = x.size // S
        ext = np.concatenate([self.hist, x]).astype(np.complex128)   # sample i of the call at ext[Q + i]
        self.x_max = float(np.max(np.abs(ext), initial=0.0))
        p, q = self.mu % L, self.mu // L
        k = np.arange(n_out, dtype=np.int64)
        y = np.zeros(n_out, np.complex128)
        for j in range(Q + 1):                                      # j ascending, as the kernel sums
            if self.tab[p, j] != 0.0:
                y += self.tab[p, j] * ext[k * S + q - j + Q]
        if self.dphase != 0.0 or self.phase != 0.0:
            y = y * np.exp(1j * (self.phase + k * self.dphase))
        self.phase = (self.phase + n_out * self.dphase) % TWO_PI
        self.hist = np.concatenate([self.hist, x])[x.size:] if Q else self.hist
        return y

    def run(self, x):
        y = self.run_c(x)
        return rx_ref.pack(rx_ref.decide(y.astype(np.complex64), self.table), self.bits) if self.bits else y

    def state(self, k=None):
        """The history, newest first (comms_symsync_get_state)."""
        return self.hist[::-1][: self.Q if k is None else k].copy()

    def set_state(self, state):
        state = np.asarray(state, np.complex64)
        assert state.size == self.Q
        self.hist = state[::-1].copy()


def fractional_delay(sym, n_pulse, sps, phases, beta, d, rrc_taps, pulse):
    """`sym` shaped at sps samples per symbol with its timing moved by d / phases input samples: shaped at phases * sps
    samples per symbol by the odd pulse of (n_pulse - 1) phases + 1 taps (every phases-th tap of it is the pulse at sps), and
    every phases-th fine sample kept from offset d -- the peaks of the symbols sit at input samples
    (n_pulse - 1) / 2 - d / phases + k sps.  rrc_taps / pulse: the oracle's.  Complex128, (len(sym) - 1) * sps samples."""
    L = phases
    fine = rrc_taps((n_pulse - 1) * L + 1, float(L * sps), beta, np.complex128)
    y = pulse(np.asarray(sym, np.complex128), fine, L * sps, np.zeros(fine.size, np.complex128))
    return y[d::L][: (len(sym) - 1) * sps].copy()


def peak_position(n_pulse, phases, d):
    return (n_pulse - 1) / 2.0 - d / float(phases)
