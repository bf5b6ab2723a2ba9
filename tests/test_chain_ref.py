"""CPU check of tests/chain_ref.py, the float64 chain reference the GPU hand-over tests compare with: against the oracle's
nodes in series on complex128 (to f64 rounding) and on complex64 (within the chain tolerance), ragged calls, a user FIR
state and FM.prev, both mixer orders, and a call long enough to be cut into chunks."""
import numpy as np
import pytest

import oracle
from chain_ref import ChainRef, check_outputs, closed_form_phase, circ


def rand_c(rng, n, dtype=np.complex64):
    return (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(dtype)


def lpf(n_taps, cutoff):
    k = np.arange(n_taps) - (n_taps - 1) / 2.0
    return (2 * cutoff * np.sinc(2 * cutoff * k) * np.hamming(n_taps)).astype(np.complex64)


def oracle_calls(x, cuts, taps, rate, dphase, phase0, fm, after, state, fm_prev, dtype):
    """The oracle's nodes in series, one batch per call; the FIR node's state is the MIXED halo with the mixer in front."""
    h = taps.astype(dtype)
    st = np.asarray(state, dtype).copy()
    if not after:
        k = np.arange(1, st.size + 1, dtype=np.float64)
        st = (st.astype(np.complex128) * np.exp(1j * (phase0 - k * dphase))).astype(dtype)
    mx, dem = oracle.Mixer(phase0, dphase), oracle.FM(dtype)
    dem.prev[0] = fm_prev
    outs, ys = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        xb = x[a:b].astype(dtype)
        y = mx.mix(oracle.batch_fir(xb, h, st)) if after else oracle.batch_fir(mx.mix(xb), h, st)
        y = oracle.decimate(y, rate)
        ys.append(y)
        outs.append(dem.demod(y) if fm else y)
    return np.concatenate(outs), np.concatenate(ys)


@pytest.mark.parametrize("fm", [False, True])
@pytest.mark.parametrize("after", [False, True])
@pytest.mark.parametrize("rate,n_taps", [(8, 63), (4, 127), (20, 255), (3, 40), (64, 100)])
def test_chain_ref_matches_the_oracle(rate, n_taps, after, fm):
    rng = np.random.default_rng(rate * 1000 + n_taps + 7 * after + 3 * fm)
    taps = lpf(n_taps, 0.4 / rate)
    taps = (taps * np.exp(1j * 0.02 * np.arange(n_taps))).astype(np.complex64)   # complex taps
    n = rate * 700
    x = rand_c(rng, n)
    state = rand_c(rng, n_taps)
    dphase, phase0, prev = 2 * np.pi * 0.137, 2.5, complex(0.3, -0.4)
    cuts = [0, rate, rate * 5, rate * 333, rate * 334, n]
    ref = ChainRef(taps, rate, dphase, phase0, fm, after, state=state, fm_prev=prev)
    got, gy = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        o, y = ref.run(x[a:b])
        got.append(o)
        gy.append(y)
        np.testing.assert_array_equal(ref.state(), np.concatenate([state[::-1], x[:b]])[::-1][:n_taps])
        assert circ(ref.phase() - ((phase0 + b * dphase) % (2 * np.pi))) < 1e-10   # (the f64 product is the inexact side)
        assert ref.fm_prev == (y[-1] if fm else prev)
    got, gy = np.concatenate(got), np.concatenate(gy)
    # complex128 oracle: the same arithmetic in another order
    w64, y64 = oracle_calls(x, cuts, taps, rate, dphase, phase0, fm, after, state, prev, np.complex128)
    assert np.max(np.abs(gy - y64)) <= 1e-12
    if fm:
        assert np.max(circ(got - w64) * np.minimum(np.abs(y64), np.abs(np.concatenate([[prev], y64[:-1]])))) <= 1e-12
    # complex64 oracle: inside the tolerance the GPU tests hold the chain to, on every output
    w32, y32 = oracle_calls(x, cuts, taps, rate, dphase, phase0, fm, after, state, prev, np.complex64)
    x_max = max(np.max(np.abs(x)), np.max(np.abs(state)))
    check_outputs(w32, got, gy, prev, taps, x_max, fm, "oracle f32")


def test_chain_ref_chunks_a_long_call(monkeypatch):
    """A call longer than the reference's chunk gives what the same stream gives in one chunk."""
    import chain_ref

    rng = np.random.default_rng(5)
    taps = lpf(63, 0.05)
    x = rand_c(rng, 8 * 3000)
    whole = ChainRef(taps, 8, 0.3, 0.1, True, False).run(x)[0]
    monkeypatch.setattr(chain_ref, "CHUNK", 8 * 97 + 3)
    cut = ChainRef(taps, 8, 0.3, 0.1, True, False).run(x)[0]
    assert np.max(np.abs(whole - cut)) <= 1e-12


def test_closed_form_phase():
    assert closed_form_phase(0.0, 2 * np.pi * 0.25, 4) == 0.0
    assert abs(closed_form_phase(1.0, -0.5, 3) - (2 * np.pi - 0.5)) < 1e-15
    # 2^27 steps: exact in rationals, where the running f64 sum drifts
    n = 1 << 27
    assert abs(closed_form_phase(0.3, 0.1, n) - (0.3 + n * 0.1) % (2 * np.pi)) < 1e-6
