"""A float64 reference of the rational resampler (comms_resample_*): the polyphase formula of include/comms_hip.h, call by
call, with its history of Q = (N - 1) // L input samples --

    out[j] = sum_{q >= 0, p + L q < N} h[p + L q] x[i - q],   p = (j M) mod L,  i = (j M) div L,   j < ceil(n L / M)

which is what UpsampleNode(L) -> BatchFirNode(taps) -> DecimateNode(M) give in series (src/util/resample_node.rs:53-65,
120-131; src/filter/fir.rs:87-102) without the products with stuffed zeros.  Rates 0 count as 1.  The decimator restarts at
sample 0 of every call; the history advances by all samples.
Shared by tests/test_resample_ref.py (pinned to the oracle's composition on the CPU) and tests/test_gpu_resample.py."""
import math

import numpy as np

BLOCK = 1 << 22   # products formed per step (keeps host memory to a few hundred MB)


def out_len(n, up, down):
    L, M = max(int(up), 1), max(int(down), 1)
    return -(-n * L // M)


def state_len(n_taps, up):
    return (n_taps - 1) // max(int(up), 1)


def unit(up, down):
    """Input samples after which the decimator's restart is phase-neutral: M / gcd(L, M)."""
    L, M = max(int(up), 1), max(int(down), 1)
    return M // math.gcd(L, M)


class ResampleRef:
    def __init__(self, taps, up, down, dtype=np.float32):
        h = np.asarray(taps, np.float64)
        assert h.ndim == 1 and h.size >= 1
        self.L, self.M, self.N = max(int(up), 1), max(int(down), 1), h.size
        self.Q = (self.N - 1) // self.L
        self.dtype = np.dtype(dtype)
        self.wide = np.complex128 if self.dtype.kind == "c" else np.float64
        QP = self.Q + 1
        tab = np.zeros(self.L * QP, np.float64)          # tab[p][q] = h[p + L q]: the taps written row-major as [QP][L] ...
        tab[: self.N] = h
        self.tab = tab.reshape(QP, self.L).T.copy()      # ... and transposed
        self.hist = np.zeros(self.Q, self.dtype)         # the last Q input samples, OLDEST first
        self.x_max = 0.0

    def run(self, x):
        """One call: ceil(n L / M) outputs in float64 / complex128."""
        x = np.ascontiguousarray(x, dtype=self.dtype)
        L, M, Q = self.L, self.M, self.Q
        n_out = out_len(x.size, L, M)
        ext = np.concatenate([self.hist, x]).astype(self.wide)   # sample i of the call at ext[Q + i]
        self.x_max = float(np.max(np.abs(ext), initial=0.0))     # over every sample this call's outputs are made of
        out = np.zeros(n_out, self.wide)
        q = np.arange(Q + 1, dtype=np.int64)
        step = max(1, BLOCK // (Q + 1))
        for a in range(0, n_out, step):
            j = np.arange(a, min(a + step, n_out), dtype=np.int64)
            p, i = (j * M) % L, (j * M) // L
            out[a:a + j.size] = np.sum(self.tab[p] * ext[(i + Q)[:, None] - q[None, :]], axis=1)
        self.hist = np.concatenate([self.hist, x])[x.size:] if Q else self.hist
        return out

    def state(self, k=None):
        """The history, newest first (comms_resample_get_state)."""
        return self.hist[::-1][: self.Q if k is None else k].copy()

    def set_state(self, state):
        state = np.asarray(state, self.dtype)
        assert state.size == self.Q
        self.hist = state[::-1].copy()


def bound(taps, x_max):
    """The project's f32 FIR bound: max|got - want| <= 1e-5 sum|taps| max|x|, x the samples the outputs are made of: the
    call's and, through the history, x[-1], x[-2], ... of earlier calls (ResampleRef.x_max after a call)."""
    return 1e-5 * float(np.sum(np.abs(np.asarray(taps, np.float64)))) * max(float(x_max), 1e-30)


def close(got, want, taps, x_max, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    b = bound(taps, x_max)
    d = np.abs(got.astype(np.complex128) - want.astype(np.complex128))
    worst = int(np.argmax(d)) if d.size else 0
    assert d.max(initial=0.0) <= b, (what, float(d.max()), b, worst)
