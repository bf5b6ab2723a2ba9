"""GPU tests of the chain node's state where it passes from one kernel to another: within one stream, where a chain of kind
Decim / DecimAny hands a call to fir_poly8_kernel or fir_decim_wave_kernel by the batch's length, format and output alignment
(chain.hip, comms_chain_run_dev); across chains of different kinds, where a checkpoint (FIR state, phase, FM.prev:
include/comms_hip.h, comms_chain_{get,set}_*) taken from one is restored into another; and the plan (plan_chain) either side
of each of its thresholds.  Every output of every call is compared with a float64 reference of the reference nodes in series
(tests/chain_ref.py), from the first output of the call on.  Run with -m gpu.

Tolerances as for every other chain test: decimated outputs max|d| <= 2e-5 * sum|h| * max|x|; demodulated angles on the
circle, weighted by the smaller magnitude of the two samples they are the argument of."""
import numpy as np
import pytest

import oracle
from chain_ref import ChainRef, check_outputs, circ, closed_form_phase, out_bound

pytestmark = pytest.mark.gpu

I16_SCALE = 1.0 / 8192


@pytest.fixture(scope="module")
def c():
    import comms_rs_amd as c

    assert c.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested (no CPU fallback)"
    return c


@pytest.fixture(scope="module")
def stream(c):
    """One device buffer of synthetic IQ (|re|, |im| <= 1), shared by the long legs."""
    import torch

    n = (1 << 26) + (1 << 24)
    xd = torch.empty(n, dtype=torch.complex64, device="cuda:0")
    c.synth_iq_dev(xd.data_ptr(), n, 0, 0x5EED)
    torch.cuda.synchronize()
    return xd


def lpf(n_taps, cutoff, cplx=False):
    k = np.arange(n_taps) - (n_taps - 1) / 2.0
    h = 2 * cutoff * np.sinc(2 * cutoff * k) * np.hamming(n_taps)
    if cplx:
        h = h * np.exp(1j * 0.01 * np.arange(n_taps))
    return h.astype(np.complex64)


class Stream:
    """One chain node and its f64 reference, driven call by call through run_dev on one stream."""

    def __init__(self, c, node, taps, rate, dphase, phase0, fm, after, state=None, seed=0):
        self.c, self.node, self.taps, self.rate, self.fm = c, node, taps, rate, fm
        self.ref = ChainRef(taps, rate, dphase, phase0, fm, after, state=state)
        self.x_max = float(np.max(np.abs(state))) if state is not None else 0.0
        self.rng = np.random.default_rng(seed)
        self.pos = 0            # next sample of the shared device buffer
        self.n_calls = 0

    def call(self, xd, n, want_kernel, variant="c32"):
        """One call of n samples: from the shared buffer ("c32"), into an output 8 bytes off a 16-byte boundary ("off8"),
        or as fresh i16 wire samples ("i16", compared with the reference of the converted samples)."""
        import torch

        node, rate, fm = self.node, self.rate, self.fm
        s = torch.cuda.current_stream().cuda_stream
        if variant == "i16":
            raw = self.rng.integers(-12000, 12000, (n, 2)).astype(np.int16)
            x = oracle.iq_i16_to_c32(raw, I16_SCALE)
            rd = torch.from_numpy(raw).cuda()
            node.set_input_format("i16", I16_SCALE)
            in_ptr = rd.data_ptr()
        else:
            x = xd[self.pos:self.pos + n].cpu().numpy()
            in_ptr = xd.data_ptr() + 8 * self.pos
            self.pos += n
        n_out = n // rate
        dt, npt = (torch.float32, np.float32) if fm else (torch.complex64, np.complex64)
        o = torch.empty(n_out + 2, dtype=dt, device="cuda:0")
        off = 8 if variant == "off8" else 0
        assert o.data_ptr() % 16 == 0
        node.run_dev(in_ptr, n, o.data_ptr() + off, s)
        torch.cuda.synchronize()
        if variant == "i16":
            node.set_input_format("c32")
        got = o.cpu().numpy().view(np.uint8)[off:off + n_out * np.dtype(npt).itemsize].view(npt)
        what = (self.n_calls, n, variant)
        self.n_calls += 1
        prev = self.ref.fm_prev
        want, y = self.ref.run(x)
        self.x_max = max(self.x_max, float(np.max(np.abs(x))))
        assert node.kernel == want_kernel, (what, node.kernel)
        check_outputs(got, want, y, prev, self.taps, self.x_max, fm, what)
        self.check_state(what)

    def check_state(self, what):
        node, ref = self.node, self.ref
        n_taps = self.taps.size
        np.testing.assert_array_equal(node.fir_state(n_taps), ref.state().astype(np.complex64), err_msg=str(what))
        assert circ(node.phase - ref.phase()) < 1e-9, (what, node.phase, ref.phase())
        if self.fm and ref.last_y is not None:
            assert abs(complex(node.fm_prev) - ref.last_y) <= out_bound(self.taps, self.x_max), (what, node.fm_prev, ref.last_y)


# ------------------------------------------------------------------ 1. per-call kernel switches inside one stream
# rate 8 (Decim, < 64 taps): the workgroup kernel on an unbalanced batch (4097 tiles of 128 outputs on 4096 single-wave
# workgroups), the wave-private kernel on 2^22 samples (4096 tiles), fir_poly8_kernel from 2^25 samples; the balanced batch
# again into an output 8 bytes off a 16-byte boundary and as i16 wire samples (both: the workgroup kernel)
R8_LEGS = [(8 * 1001, "time"), (1 << 25, "poly"), (8 * ((1 << 19) + 128), "time"), (1 << 22, "time"), ((1 << 25) + 8 * 5, "poly"),
           (1 << 22, "time", "off8"), (1 << 22, "time", "i16"), (8, "time")]
# rate 4 (Decim, 64 ... 127 taps): the time kernel below 2^22 samples, fir_poly8_kernel from 2^22
R4_LEGS = [(4 * 1001, "time"), ((1 << 22) - 4, "time"), (1 << 22, "poly"), (4 * ((1 << 19) + 37), "time"), ((1 << 22) + 4 * 1000, "poly"),
           (4, "time")]
# rate 64 (DecimAny, < 128 taps): the any-rate kernel below 2^23 samples, fir_poly8_kernel from 2^23
R64_LEGS = [(64 * 1001, "time_any"), (1 << 23, "poly"), (64 * 5003, "time_any"), ((1 << 23) + 64 * 7, "poly"), (64, "time_any")]


def _run_switch_stream(c, stream, rate, n_taps, fm, after, legs, user_state, kernel="auto", cplx=False):
    taps = lpf(n_taps, 0.4 / rate, cplx)
    dphase, phase0 = 2 * np.pi * 0.0123, 0.7
    node = c.ChainNode(dphase, phase0, taps, rate, fm, mixer_after_fir=after, kernel=kernel)
    state = None
    if user_state:
        state = (np.random.default_rng(n_taps).uniform(-1, 1, (n_taps, 2)) @ [1, 1j]).astype(np.complex64)
        node.set_fir_state(state)
    st = Stream(c, node, taps, rate, dphase, phase0, fm, after, state=state, seed=rate + n_taps)
    for leg in legs:
        st.call(stream, *leg)
    assert st.pos <= stream.numel()


@pytest.mark.parametrize("n_taps", [31, 63])
@pytest.mark.parametrize("fm,after,user_state", [(False, False, True), (False, True, False), (True, False, False)])
def test_switch_rate8_workgroup_wave_poly8(c, stream, n_taps, fm, after, user_state):
    _run_switch_stream(c, stream, 8, n_taps, fm, after, R8_LEGS, user_state)


@pytest.mark.parametrize("n_taps", [100, 127])
@pytest.mark.parametrize("fm,after,user_state", [(True, False, True), (False, False, False), (False, True, False)])
def test_switch_rate4_time_poly8(c, stream, n_taps, fm, after, user_state):
    _run_switch_stream(c, stream, 4, n_taps, fm, after, R4_LEGS, user_state)


@pytest.mark.parametrize("after,user_state", [(False, True), (True, False)])
def test_switch_rate64_any_rate_poly8(c, stream, after, user_state):
    """With the mixer in front the chain runs modulated taps, on the polyphase kernel in POST mode."""
    _run_switch_stream(c, stream, 64, 100, False, after, R64_LEGS, user_state)


@pytest.mark.parametrize("fm", [False, True])
@pytest.mark.parametrize("rate,n_taps,cplx", [(2, 31, False), (2, 64, True), (4, 63, False), (4, 128, True)])
def test_switch_rates_2_and_4_workgroup_wave(c, stream, rate, n_taps, cplx, fm):
    """The wave-private kernel on balanced batches (4096 tiles of 128 outputs), the workgroup kernel on an unbalanced batch, on
    the balanced batch into a misaligned output and on i16 input."""
    B = (1 << 20) if rate == 2 else (1 << 21)
    legs = [(rate * 1001, "time"), (B, "time"), (rate * 128 * 4097, "time"), (B, "time", "off8"), (B, "time"), (B, "time", "i16"),
            (B, "time"), (rate, "time")]
    _run_switch_stream(c, stream, rate, n_taps, fm, not fm, legs, user_state=fm and rate == 2, kernel="time", cplx=cplx)


# ------------------------------------------------------------------ 2. checkpoint and restore across kinds
# (taps, rate, FM settings, the kinds the flags reach: ChainNode keyword arguments)
RESTORE_GROUPS = {
    # Series / SeriesPost, Os1024 (FM: the separate demodulator), Decim on the time kernel, Poly8, Decim handing every call to poly8
    "127x8": (127, 8, (False, True), [dict(unfused=True), dict(kernel="freq"), dict(kernel="time"), dict(kernel="poly"), dict()]),
    # Series, Os1024, DecimAny (modulated taps with the mixer in front; FM in the kernel), Poly8 (FM: DecimAny with the
    # separate demodulator, handing every call to poly8), DecimAny handing every call to poly8
    "255x20": (255, 20, (False, True), [dict(unfused=True), dict(kernel="freq"), dict(kernel="time"), dict(kernel="poly"), dict()]),
    # Poly8 with the separate demodulator, Series, Os4096Dec, DecimAny
    "300x16": (300, 16, (True,), [dict(), dict(unfused=True), dict(kernel="freq"), dict(kernel="time")]),
    "700x5": (700, 5, (False, True), [dict(), dict(unfused=True)]),       # Os4096Dec, Series
    "2500x6": (2500, 6, (False, True), [dict(), dict(unfused=True)]),     # Os16kDec, Series
    "4100x3": (4100, 3, (False, True), [dict(), dict(unfused=True)]),     # SeriesPost (modulated taps with the mixer in front), Series
}


@pytest.mark.parametrize("after", [False, True])
@pytest.mark.parametrize("group", list(RESTORE_GROUPS))
def test_restore_across_kinds(c, group, after):
    n_taps, rate, fms, kinds = RESTORE_GROUPS[group]
    taps = lpf(n_taps, 0.4 / rate)
    dphase, phase0 = 2 * np.pi * 0.0371, 2.2
    n0 = rate * (1237 + n_taps // rate)                 # the checkpoint: a multiple of no segment size
    n = n0 + rate * (1900 + n_taps // rate)
    x = (np.random.default_rng(n_taps).uniform(-1, 1, (n, 2)) @ [1, 1j]).astype(np.complex64)
    x_max = float(np.max(np.abs(x)))
    a_cuts = [0, rate * 7, rate * 519, n0]
    b_cuts = [n0, n0 + rate, n0 + rate * 901, n]
    for fm in fms:
        want, y = ChainRef(taps, rate, dphase, phase0, fm, after).run(x)
        for ia, ka in enumerate(kinds):
            for ib, kb in enumerate(kinds):
                what = (group, fm, after, ka, kb)
                A = c.ChainNode(dphase, phase0, taps, rate, fm, mixer_after_fir=after, **ka)
                outs = [A.run(x[p:q]) for p, q in zip(a_cuts[:-1], a_cuts[1:])]
                state, phase = A.fir_state(n_taps), A.phase
                np.testing.assert_array_equal(state, x[:n0][::-1][:n_taps], err_msg=str(what))
                assert circ(phase - closed_form_phase(phase0, dphase, n0)) < 1e-9, what
                B = c.ChainNode(dphase, 0.0, taps, rate, fm, mixer_after_fir=after, **kb)
                if (ia + ib) % 2:
                    B.phase = phase
                    B.set_fir_state(state)
                else:
                    B.set_fir_state(state)
                    B.phase = phase
                if fm:
                    B.fm_prev = A.fm_prev
                else:
                    with pytest.raises(c.CommsError):
                        A.fm_prev
                outs += [B.run(x[p:q]) for p, q in zip(b_cuts[:-1], b_cuts[1:])]
                check_outputs(np.concatenate(outs), want, y, 0j, taps, x_max, fm, what)
                if ib == 0:
                    # the state's size is the filter's: one sample less or more is refused; fewer read the newest ones
                    for bad in (n_taps - 1, n_taps + 1):
                        with pytest.raises(c.CommsError):
                            A.set_fir_state(x[:bad])
                    with pytest.raises(c.CommsError):
                        A.fir_state(n_taps + 1)
                    for k in (1, n_taps // 3):
                        np.testing.assert_array_equal(A.fir_state(k), x[:n0][::-1][:k], err_msg=str((what, k)))


# ------------------------------------------------------------------ 3. the plan at its boundaries
F, T = False, True
FREQ, TIME, POLY, UNF = dict(kernel="freq"), dict(kernel="time"), dict(kernel="poly"), dict(unfused=True)
# (taps, rate, fm, mixer after, flags, the kind comms_chain_is_fused reports before any call)
PLAN_ROWS = [
    # the fused forms end at 257 taps; from 258 the polyphase kernel takes rate 8 from the start
    (257, 8, F, F, {}, "time"), (258, 8, F, F, {}, "poly"), (257, 8, F, T, {}, "time"), (258, 8, F, T, {}, "poly"),
    (257, 8, T, F, {}, "time"), (258, 8, T, F, {}, "poly"),
    (257, 8, F, F, FREQ, "freq"), (258, 8, F, F, FREQ, "freq"), (257, 8, F, F, TIME, "time"), (258, 8, F, F, TIME, "time_any"),
    (257, 8, F, F, UNF, "unfused"), (258, 8, F, T, UNF, "unfused"), (257, 8, F, F, POLY, "poly"), (258, 8, F, F, POLY, "poly"),
    # the demodulator inside the polyphase kernel up to 505 taps, its own launch behind it from 506
    (505, 8, T, F, {}, "poly"), (506, 8, T, F, {}, "poly"), (505, 8, T, T, {}, "poly"), (506, 8, T, T, {}, "poly"),
    (505, 8, T, F, POLY, "poly"), (506, 8, T, F, POLY, "poly"),
    # the polyphase kernel ends at 513 taps, the any-rate kernel at 512
    (513, 8, F, F, {}, "poly"), (514, 8, F, F, {}, "freq"), (513, 8, F, T, {}, "poly"), (514, 8, F, T, {}, "freq"),
    (512, 8, F, F, TIME, "time_any"), (513, 8, F, F, TIME, "unfused"),
    (512, 20, F, F, TIME, "time_any"), (513, 20, F, F, TIME, "unfused"), (512, 20, F, F, {}, "poly"), (513, 20, F, F, {}, "poly"),
    (514, 20, F, F, {}, "freq"), (512, 44, F, F, {}, "time_any"), (513, 44, F, T, {}, "freq"),
    # 258 ... 513 taps: the polyphase kernel at rates 4 m up to 36 and 8 m up to 64; the any-rate kernel at 44, 52, 60
    (300, 36, F, F, {}, "poly"), (300, 44, F, F, {}, "time_any"), (300, 48, F, F, {}, "poly"), (300, 60, F, T, {}, "time_any"),
    # the 4096-point decimating kernel to 1537 taps, the 16384-point one to 4097, the series beyond
    (1537, 5, F, F, {}, "freq"), (1538, 5, F, F, {}, "freq"), (1537, 5, T, T, {}, "freq"), (1538, 5, T, T, {}, "freq"),
    (1538, 5, F, F, UNF, "unfused"), (4097, 5, F, F, {}, "freq"), (4098, 5, F, F, {}, "unfused"), (4097, 5, F, T, {}, "freq"),
    (4098, 5, F, T, {}, "unfused"), (4098, 5, T, F, {}, "unfused"),
    # the per-rate kernel to rate 16, the any-rate kernel from 17
    (63, 16, F, F, {}, "time"), (63, 17, F, F, {}, "time_any"), (63, 16, T, F, {}, "time"), (63, 17, T, F, {}, "time_any"),
    (63, 16, F, F, FREQ, "freq"), (63, 17, F, F, FREQ, "freq"),
    # the 1024-point fusion and the any-rate kernel to rate 2^20 (can_fuse_nofm), the series beyond
    (63, 1 << 20, F, F, {}, "time_any"), (63, (1 << 20) + 1, F, F, {}, "unfused"), (63, 1 << 20, F, T, FREQ, "freq"),
    (63, (1 << 20) + 1, F, T, FREQ, "unfused"),
]


@pytest.mark.parametrize("n_taps,rate,fm,after,flags,want", PLAN_ROWS,
                         ids=["%dx%d%s%s%s" % (r[0], r[1], "-fm" if r[2] else "", "-after" if r[3] else "",
                                               "".join("-%s" % v if v is not True else "-%s" % k for k, v in r[4].items())) for r in PLAN_ROWS])
def test_plan_boundaries(c, n_taps, rate, fm, after, flags, want):
    taps = lpf(n_taps, 0.4 / min(rate, 64))
    dphase, phase0 = 2 * np.pi * 0.0213, 0.4
    node = c.ChainNode(dphase, phase0, taps, rate, fm, mixer_after_fir=after, **flags)
    assert node.kernel == want
    n_out = max(3, 600, (3 * n_taps) // rate) if rate < 4096 else 3
    n = rate * n_out
    x = (np.random.default_rng(n_taps + rate).uniform(-1, 1, (n, 2)) @ [1, 1j]).astype(np.complex64)
    ref = ChainRef(taps, rate, dphase, phase0, fm, after)
    cuts = sorted({0, rate, rate * (n_out // 3 + 1), n})
    for p, q in zip(cuts[:-1], cuts[1:]):
        prev = ref.fm_prev
        w, y = ref.run(x[p:q])
        check_outputs(node.run(x[p:q]), w, y, prev, taps, float(np.max(np.abs(x))), fm, (p, q))
    np.testing.assert_array_equal(node.fir_state(n_taps), ref.state().astype(np.complex64))
    assert circ(node.phase - ref.phase()) < 1e-9
