"""The one property every stateful node keeps whatever kernel runs it: after any sequence of calls its state is the tail of
[zeros at creation (or the user's state) | every input so far], newest first -- input samples, so bit for bit, no tolerance.
All of these nodes keep that history in the same device type (History, csrc/common.hpp); this file runs each of them through
the shapes at which the history mixes old samples and new ones:

  taps    1 (the shortest state the node has: none for the resampler and the channelizer), 2 and 5 (9 for the resampler,
          whose state is (taps - 1) // up samples)
  calls   n = 1 and n = H - 1 (shorter than the history: the new history is part old history, part input), H + 1, 64, 3;
          a chain takes multiples of its rate
  reads   n_state = 0, 1, one strictly between 1 and H, and H
  series  the same on the nodes' fallbacks: 258 real taps, up = 257, three channels
  restore where the node has a setter: the state read from one node written into a fresh one, whose next call must equal the
          uncut node's bit for bit
  stream  the nodes behind the resampler, whose accessors are the same shared helper (csrc/stream_call.hpp), at the smallest
          shapes that mix old and new history: the symbol synchroniser (phases = sps = 2 with 1, 2 and 5 taps: Q = 0, 0, 2;
          9 taps on one phase: Q = 8; timing and rotation travel with the state), the frame synchroniser (the shortest word,
          2 symbols, and one of 5, guard 0 and 2: H = P + 2 G - 1), the OFDM synchroniser (window 2, lag 1, guard 0; window 5,
          lag 3, guard 2: H = W + L + 2 G - 1) and the deframer (n_payload 1 and 4 without lookback: H = 0 and 3; n_payload 2
          with lookback 6: H = 6); the position travels with the state of the last three.  The synchronisers run under a
          threshold of 1e-6, so that a call returns many detections, and the deframer is handed one frame per call that
          starts `lookback` symbols back: the restored node's output is made from the restored history.
  refusal every kind's getter refuses n_state = H + 1 and its setter H - 1 and H + 1 samples with COMMS_ERR_ARG (code 1), and a
          refused setter leaves the state as it was

Chains mix by a quarter turn per sample (dphase = pi / 2) and are cut at a multiple of four samples: the oscillator's phase
at the cut is then exactly 0 in every representation (the fused kinds keep 64-bit turns, the series a double), and the
rotors are (1, 0), (0, 1), (-1, 0), (0, -1) up to 1e-16, far below an f32 rounding -- so that the restored node's outputs
can be asked to match bit for bit even where its history of MIXED samples is rebuilt on the host (the unfused chain).
What the parity and hand-over tests already assert (kernel switches of a chain, cut points of resampler and channelizer) is
not repeated here."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def c():
    import comms_rs_amd as c

    assert c.device_count() >= 1, "no MI355X visible: the HIP path cannot be tested (no CPU fallback)"
    return c


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    np.testing.assert_array_equal(got.view(np.uint8), want.view(np.uint8), err_msg=str(what))


def samples(rng, n, dtype):
    """n samples of a node's stream type: int16 (n, 2), float32, complex64 or complex128."""
    if dtype == np.int16:
        return rng.integers(-30000, 30000, (n, 2)).astype(np.int16)
    if np.dtype(dtype).kind == "c":
        return (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(dtype)
    return rng.uniform(-1, 1, n).astype(dtype)


class Kind:
    """How one node type is made, run and read.  hist(n_taps): samples of state; multiple: calls are multiples of it."""

    def __init__(self, make, dtype, hist, get, set_=None, taps_dtype=None, multiple=1, init_state=False, carry=(), run=None, cut=4,
                 restore=None):
        self.make, self.dtype, self.hist, self.get, self.set, self.multiple = make, dtype, hist, get, set_, multiple
        self.taps_dtype = taps_dtype or dtype
        self.init_state = init_state    # make(c, taps, state) takes the reference's initial state
        self.carry = carry              # attributes a restore copies beside the history (oscillator phase, stream index)
        self.run = run or (lambda node, x: node.run(x))   # one call; what it returns is compared bit for bit after a restore
        self.cut = cut                  # multiple > 1: the calls before a restore add up to a multiple of `cut` samples
        self.restore = restore          # restore(fresh, node): what travels with the state and is no plain attribute


CHAIN_DPHASE = np.pi / 2


def _chain(**kw):
    def make(c, taps, state=None):
        node = c.ChainNode(CHAIN_DPHASE, 0.0, taps, 2, False, **kw)
        assert node.fused == (not kw.get("unfused", False)), (kw, node.kernel)
        return node
    return Kind(make, np.complex64, lambda t: t, lambda n, k: n.fir_state(k), lambda n, s: n.set_fir_state(s),
                taps_dtype=np.float32, multiple=2, carry=("phase",))


def _resample(dtype, up=2, down=3):
    return Kind(lambda c, taps, state=None: c.ResampleNode(taps, up, down, dtype), dtype, lambda t: (t - 1) // max(up, 1),
                lambda n, k: n.get_state(k), lambda n, s: n.set_state(s), taps_dtype=np.float32)


def _channelizer(channels):
    return Kind(lambda c, taps, state=None: c.ChannelizerNode(taps, channels, 3), np.complex64, lambda t: t - 1,
                lambda n, k: n.get_state(k), lambda n, s: n.set_state(s), taps_dtype=np.float32, carry=("phase",))


SS_SPS = 2
THRESHOLD = 1e-6


def _symsync(phases):
    """dphase = pi / 2 per symbol, cut at a multiple of four symbols (eight samples): the phase at the cut is exactly 0, as the
    chains'.  `timing` reads mu in steps of 1 / phases and is set in samples."""
    def make(c, taps, state=None):
        node = c.SymbolSyncNode(taps, phases, SS_SPS)
        node.set_timing(1.0 / phases)
        node.set_rotation(CHAIN_DPHASE, 0.0)
        return node

    def restore(fresh, node):
        fresh.set_timing(node.timing / phases)
        fresh.set_rotation(*node.rotation)
    return Kind(make, np.complex64, lambda t: (t - 1) // phases, lambda n, k: n.get_state(k), lambda n, s: n.set_state(s),
                taps_dtype=np.float32, multiple=SS_SPS, cut=4 * SS_SPS, restore=restore)


def _with_position(fresh, node):
    fresh.set_position(node.position())


def _framesync(guard):
    """The taps are the word."""
    return Kind(lambda c, taps, state=None: c.FrameSyncNode(taps, THRESHOLD, guard), np.complex64, lambda t: t + 2 * guard - 1,
                lambda n, k: n.state(k), lambda n, s: n.set_state(s), run=lambda n, x: n.run(x, raw=True), restore=_with_position)


def _ofdmsync(lag, guard):
    """The tap count is the window."""
    def run(node, x):
        det, cfo = node.run(x, raw=True)
        return np.concatenate([det.view(np.uint8), cfo.view(np.uint8)])
    return Kind(lambda c, taps, state=None: c.OfdmSyncNode(lag, len(taps), THRESHOLD, guard), np.complex64,
                lambda t: t + lag + 2 * guard - 1, lambda n, k: n.state(k), lambda n, s: n.set_state(s), taps_dtype=np.float32, run=run,
                restore=_with_position)


def _deframe(lookback):
    """The tap count is n_payload.  A call long enough to complete it gets one frame that starts `lookback` symbols back (none
    stays pending: a restore carries state and position only)."""
    def run(node, x):
        import comms_rs_amd as c
        pos, det = node.position(), np.zeros(0, c.FRAME_DETECTION_DTYPE)
        start = pos - min(lookback, pos)
        if start + node.n_payload <= pos + len(x):
            det = np.zeros(1, c.FRAME_DETECTION_DTYPE)
            det[0] = (start, 0.6, 0.8, 1.0, 1.0)
        return node.run(x, det)
    return Kind(lambda c, taps, state=None: c.DeframeNode(len(taps), 0, lookback), np.complex64, lambda t: max(lookback, t - 1),
                lambda n, k: n.state(k), lambda n, s: n.set_state(s), taps_dtype=np.float32, run=run, restore=_with_position)


KINDS = {
    "fir": Kind(lambda c, taps, state=None: c.BatchFirNode(taps, state), np.complex64, lambda t: t, lambda n, k: n.state(k),
                lambda n, s: n.set_state(s), init_state=True),
    "fir_i16": Kind(lambda c, taps, state=None: c.BatchFirNodeI16(taps, state), np.int16, lambda t: t, lambda n, k: n.state(k),
                    init_state=True),
    "fir_f64": Kind(lambda c, taps, state=None: c.BatchFirNodeF64(taps, state), np.complex128, lambda t: t, lambda n, k: n.state(k),
                    lambda n, s: n.set_state(s), init_state=True),
    "rfir": Kind(lambda c, taps, state=None: c.RealFirDecimNode(taps, 2, state), np.float32, lambda t: t, lambda n, k: n.get_state(k),
                 lambda n, s: n.set_state(s), init_state=True),
    "resample_f32": _resample(np.float32),
    "resample_c32": _resample(np.complex64),
    "channelizer": _channelizer(4),
    "chain_fused": _chain(),
    "chain_unfused": _chain(unfused=True),
    # the series fallbacks
    "rfir_series": Kind(lambda c, taps, state=None: c.RealFirDecimNode(taps, 2, state), np.float32, lambda t: t,
                        lambda n, k: n.get_state(k), lambda n, s: n.set_state(s)),
    "resample_series": _resample(np.float32, up=257, down=3),
    "channelizer_series": _channelizer(3),
    # the stream nodes behind the resampler
    "symsync": _symsync(2),
    "symsync_one_phase": _symsync(1),
    "framesync_g0": _framesync(0),
    "framesync_g2": _framesync(2),
    "ofdmsync_l1_g0": _ofdmsync(1, 0),
    "ofdmsync_l3_g2": _ofdmsync(3, 2),
    "deframe": _deframe(0),
    "deframe_lookback6": _deframe(6),
}

CASES = [(name, t) for name in ("fir", "fir_i16", "fir_f64", "rfir", "channelizer", "chain_fused", "chain_unfused") for t in (1, 2, 5)]
CASES += [(name, t) for name in ("resample_f32", "resample_c32") for t in (1, 2, 5, 9)]
# (up = 257 with 3 taps keeps no sample at all; 600 taps keep two)
STREAM_CASES = [("symsync", 1), ("symsync", 2), ("symsync", 5), ("symsync_one_phase", 9), ("framesync_g0", 2), ("framesync_g0", 5),
                ("framesync_g2", 2), ("framesync_g2", 5), ("ofdmsync_l1_g0", 2), ("ofdmsync_l3_g2", 5), ("deframe", 1), ("deframe", 4),
                ("deframe_lookback6", 2)]
SERIES_CASES = [("rfir_series", 258), ("resample_series", 3), ("resample_series", 600), ("channelizer_series", 2), ("channelizer_series", 5)]


def call_lengths(H, multiple, longest, cut=4):
    """n = 1, H - 1, H + 1, `longest`, 3 as multiples of `multiple` (each rounded up; a chain's total a multiple of `cut`)."""
    lens = [n for n in (1, H - 1, H + 1, longest, 3) if n > 0]
    lens = [(n + multiple - 1) // multiple * multiple for n in lens]
    if multiple > 1 and sum(lens) % cut:
        lens.append(cut - sum(lens) % cut)
    return lens


def reads(H):
    return sorted({0, 1, (H + 1) // 2 if H >= 3 else 1, H} & set(range(H + 1)))


def check_state(kind, node, stream, H, what):
    """stream: [initial history, time order | inputs so far]."""
    for k in reads(H):
        want = stream[len(stream) - k:][::-1]
        same_bits(kind.get(node, k), want, what + ("n_state", k))


def run_property(c, name, n_taps, longest, state=None):
    kind = KINDS[name]
    rng = np.random.default_rng(100 * n_taps + len(name))
    taps = samples(rng, n_taps, kind.taps_dtype)
    H = kind.hist(n_taps) if state is None else len(state)
    node = kind.make(c, taps, state)
    stream = np.zeros_like(samples(rng, H, kind.dtype)) if state is None else np.ascontiguousarray(state[::-1])
    check_state(kind, node, stream, H, (name, n_taps, "created"))
    lens = call_lengths(H, kind.multiple, longest, kind.cut)
    for i, n in enumerate(lens):
        x = samples(rng, n, kind.dtype)
        kind.run(node, x)
        stream = np.concatenate([stream, x])
        check_state(kind, node, stream, H, (name, n_taps, "call", i, n))
    if kind.set is None:
        return
    # restore: the state (and what travels with it) into a fresh node; the next call of both, and their states after it
    assert kind.multiple == 1 or sum(lens) % kind.cut == 0
    fresh = kind.make(c, taps, None if state is None else np.zeros_like(state))
    kind.set(fresh, kind.get(node, H))
    for attr in kind.carry:
        setattr(fresh, attr, getattr(node, attr))
    if kind.restore:
        kind.restore(fresh, node)
    x = samples(rng, (H + 2) * kind.multiple, kind.dtype)
    got, want = kind.run(fresh, x), kind.run(node, x)
    assert len(want), (name, n_taps, "the call after the restore returns nothing to compare")
    same_bits(got, want, (name, n_taps, "restored output"))
    same_bits(kind.get(fresh, H), kind.get(node, H), (name, n_taps, "restored state"))


@pytest.mark.parametrize("name,n_taps", CASES)
def test_state_is_the_tail_of_the_stream(c, name, n_taps):
    run_property(c, name, n_taps, 64)


@pytest.mark.parametrize("name,n_taps", STREAM_CASES)
def test_state_is_the_tail_of_the_stream_stream_nodes(c, name, n_taps):
    run_property(c, name, n_taps, 64)


@pytest.mark.parametrize("name,n_taps", SERIES_CASES)
def test_state_is_the_tail_of_the_stream_series(c, name, n_taps):
    node = KINDS[name].make(c, samples(np.random.default_rng(0), n_taps, np.float32))
    assert "series" in node.kernel(300), (name, n_taps, node.kernel(300))
    run_property(c, name, n_taps, 300 - 300 % KINDS[name].multiple)


@pytest.mark.parametrize("name", [k for k, v in KINDS.items() if v.init_state])
def test_short_initial_state(c, name):
    """An initial state shorter than the taps: n_eff, and with it the state's length, follows the state."""
    kind = KINDS[name]
    state = samples(np.random.default_rng(7), 3, kind.dtype)
    run_property(c, name, 5, 64, state=state)
    node = kind.make(c, samples(np.random.default_rng(8), 5, kind.taps_dtype), state)
    with pytest.raises(c.CommsError):
        kind.get(node, 4)


# one case per node kind: (kind, taps) with a state of H >= 2 samples, so that H - 1 >= 1 samples are refused too
ARGUMENT_CASES = [("fir", 5), ("fir_i16", 5), ("fir_f64", 5), ("rfir", 5), ("resample_c32", 9), ("channelizer", 5), ("chain_fused", 5),
                  ("symsync", 5), ("framesync_g2", 2), ("deframe", 4), ("ofdmsync_l1_g0", 2)]


@pytest.mark.parametrize("name,n_taps", ARGUMENT_CASES)
def test_state_lengths_are_refused_with_the_argument_code(c, name, n_taps):
    """The getter takes n_state <= H, the setter exactly H: anything else is COMMS_ERR_ARG (1), and a refused set changes nothing."""
    kind = KINDS[name]
    rng = np.random.default_rng(5)
    node = kind.make(c, samples(rng, n_taps, kind.taps_dtype))
    H = kind.hist(n_taps)
    assert H >= 2
    kind.run(node, samples(rng, 8 * kind.multiple, kind.dtype))
    before = kind.get(node, H)
    assert np.any(before.view(np.uint8)), (name, "the state under test is all zeros")
    with pytest.raises(c.CommsError) as err:
        kind.get(node, H + 1)
    assert err.value.code == 1, (name, "get", H + 1, err.value)
    if kind.set is None:
        return
    for n in (H - 1, H + 1):
        with pytest.raises(c.CommsError) as err:
            kind.set(node, samples(rng, n, kind.dtype))
        assert err.value.code == 1, (name, "set", n, err.value)
        same_bits(kind.get(node, H), before, (name, "state after a refused set of", n))
