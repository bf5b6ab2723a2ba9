"""A float64 reference of the polyphase channelizer (comms_channelizer_*): the formula of include/comms_hip.h in complex128,
call by call, with its state of N - 1 input samples and the stream index t --

    v_p(t)   = sum_{q >= 0, p + M q < N} h[p + M q] x[t - p - M q]          p = 0 .. M-1
    out_k[j] = sum_{p < M} e^{+2 pi i k p / M} v_{(p + r) mod M}(t)          t = c + j D,  r = t mod M,  j < ceil(n / D)

which is what M chains MixerNode(0, -2 pi k / M) -> BatchFirNode(taps) -> DecimateNode(D) give (src/mixer.rs:43-84,
src/filter/fir.rs:87-102, src/util/resample_node.rs:53-65).  Rate 0 counts as 1.  The decimator restarts at sample 0 of
every call; the history and t advance by all samples.  The oscillator is the integer (k t) mod M: exact.
Shared by tests/test_channelizer_ref.py (pinned to tests/chain_ref.ChainRef and to the oracle's composition on the CPU),
tests/test_gpu_channelizer.py and the values the C++ graph test checks."""
import numpy as np

from chain_ref import out_bound

BLOCK = 1 << 21   # products formed per step (keeps host memory to a few hundred MB)


def out_len(n, down):
    return -(-n // max(int(down), 1))


def state_len(n_taps):
    return n_taps - 1


class ChannelizerRef:
    def __init__(self, taps, channels, down, layout="channel"):
        h = np.asarray(taps, np.float64)
        assert h.ndim == 1 and h.size >= 1 and layout in ("channel", "frame")
        self.M, self.D, self.N = int(channels), max(int(down), 1), h.size
        self.Q = -(-self.N // self.M)
        self.h = np.zeros(self.Q * self.M, np.float64)   # the taps padded to whole branches
        self.h[: self.N] = h
        self.layout = layout
        self.hist = np.zeros(self.N - 1, np.complex64)   # the last N - 1 input samples, OLDEST first
        self.t = 0                                       # stream index of the next input sample
        self.x_max = 0.0

    def run(self, x):
        """One call: ceil(n / D) frames of M outputs, complex128, [M][frames] or [frames][M] by the layout."""
        x = np.ascontiguousarray(x, dtype=np.complex64)
        M, D, Q, H = self.M, self.D, self.Q, self.N - 1
        frames = out_len(x.size, D)
        QM = Q * M
        ext = np.concatenate([np.zeros(QM - 1 - H, np.complex128), self.hist.astype(np.complex128), x.astype(np.complex128)])
        self.x_max = max(self.x_max, float(np.max(np.abs(ext), initial=0.0)))   # over every sample the outputs so far are made of
        out = np.zeros((frames, M), np.complex128)
        n_idx = np.arange(QM, dtype=np.int64)
        step = max(1, BLOCK // QM)
        for a in range(0, frames, step):
            j = np.arange(a, min(a + step, frames), dtype=np.int64)
            # sample t - n of frame j sits at ext[(QM - 1) + j D - n]
            u = self.h[None, :] * ext[(QM - 1 + j * D)[:, None] - n_idx[None, :]]   # h[n] x[t - n]
            v = u.reshape(j.size, Q, M).sum(axis=1)                                 # v_p(t)
            r = (self.t + j * D) % M
            z = v[np.arange(j.size)[:, None], (np.arange(M)[None, :] + r[:, None]) % M]
            out[a:a + j.size] = np.fft.ifft(z, axis=1) * M
        self.hist = np.concatenate([self.hist, x])[x.size:] if H else self.hist
        self.t += x.size
        return out if self.layout == "frame" else np.ascontiguousarray(out.T)

    def state(self, k=None):
        """The history, newest first (comms_channelizer_get_state)."""
        return self.hist[::-1][: self.N - 1 if k is None else k].copy()

    def set_state(self, state):
        state = np.asarray(state, np.complex64)
        assert state.size == self.N - 1
        self.hist = state[::-1].copy()

    def phase(self):
        return self.t % self.M

    def set_phase(self, t):
        self.t = int(t) % self.M

    def bound(self):
        """The chain's bound per output, 2e-5 sum|h| max|x| (chain_ref.out_bound): the transform adds about
        log2(M) 2^-24 sum|h| max|x|, under 1e-6 at M = 1024, so it stands unchanged."""
        return out_bound(self.h, max(self.x_max, 1e-30))


def check(got, want, ref, what=""):
    """Every output of a call, from the first, within the chain's bound."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    d = np.abs(got.astype(np.complex128) - want)
    b = ref.bound() if isinstance(ref, ChannelizerRef) else float(ref)
    worst = int(np.argmax(d)) if d.size else 0
    assert d.max(initial=0.0) <= b, (what, "output", worst, "of", d.size, float(d.max()), b)
