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

    def __init__(self, make, dtype, hist, get, set_=None, taps_dtype=None, multiple=1, init_state=False, carry=()):
        self.make, self.dtype, self.hist, self.get, self.set, self.multiple = make, dtype, hist, get, set_, multiple
        self.taps_dtype = taps_dtype or dtype
        self.init_state = init_state    # make(c, taps, state) takes the reference's initial state
        self.carry = carry              # attributes a restore copies beside the history (oscillator phase, stream index)


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
}

CASES = [(name, t) for name in ("fir", "fir_i16", "fir_f64", "rfir", "channelizer", "chain_fused", "chain_unfused") for t in (1, 2, 5)]
CASES += [(name, t) for name in ("resample_f32", "resample_c32") for t in (1, 2, 5, 9)]
# (up = 257 with 3 taps keeps no sample at all; 600 taps keep two)
SERIES_CASES = [("rfir_series", 258), ("resample_series", 3), ("resample_series", 600), ("channelizer_series", 2), ("channelizer_series", 5)]


def call_lengths(H, multiple, longest):
    """n = 1, H - 1, H + 1, `longest`, 3 as multiples of `multiple` (each rounded up; a chain's total a multiple of 4)."""
    lens = [n for n in (1, H - 1, H + 1, longest, 3) if n > 0]
    lens = [(n + multiple - 1) // multiple * multiple for n in lens]
    if multiple > 1 and sum(lens) % 4:
        lens.append(4 - sum(lens) % 4)
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
    lens = call_lengths(H, kind.multiple, longest)
    for i, n in enumerate(lens):
        x = samples(rng, n, kind.dtype)
        node.run(x)
        stream = np.concatenate([stream, x])
        check_state(kind, node, stream, H, (name, n_taps, "call", i, n))
    if kind.set is None:
        return
    # restore: the state (and what travels with it) into a fresh node; the next call of both, and their states after it
    assert kind.multiple == 1 or sum(lens) % 4 == 0
    fresh = kind.make(c, taps, None if state is None else np.zeros_like(state))
    kind.set(fresh, kind.get(node, H))
    for attr in kind.carry:
        setattr(fresh, attr, getattr(node, attr))
    x = samples(rng, (H + 2) * kind.multiple, kind.dtype)
    same_bits(fresh.run(x), node.run(x), (name, n_taps, "restored output"))
    same_bits(kind.get(fresh, H), kind.get(node, H), (name, n_taps, "restored state"))


@pytest.mark.parametrize("name,n_taps", CASES)
def test_state_is_the_tail_of_the_stream(c, name, n_taps):
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
