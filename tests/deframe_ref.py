"""Reference material of the deframer (comms_deframe_*), shared by tests/test_deframe_ref.py (CPU) and
tests/test_gpu_deframe.py:

  ref_frames    the definition of include/comms_hip.h: the per-frame values u, g (f64, rounded to f32 once), then z, the
                decisions and the LLRs in f64, with the pending-list bookkeeping over arbitrary calls.
  model_frames  the ARITHMETIC of deframe_kernel: f32, zr = fma(-yi, ui, yr ur), zi = fma(yi, ur, yr ui), the products by g,
                the distances of the decision rule and the LLR's subtraction and product each rounded on their own (an FMA is
                emulated as the f64 sum of the exact product, rounded to f32: framesync_ref._fma).
  cases         every stream, configuration and call plan the GPU test runs, so that the CPU test measures the model on
                exactly those.  The detections are framesync_ref.ref_detect's (their correlation rounded to f32), so that
                neither test needs the frame synchroniser.
"""
import collections
import functools
import math

import numpy as np

import framesync_ref as fr
import rx_ref

# Largest distance of model_frames from ref_frames over cases(), measured by tests/test_deframe_ref.py (which asserts that
# they still hold): z relative to |z|, the LLRs relative to s * max_i d_i of their symbol.
MODEL_Z_DISTANCE = 1.2e-7      # measured 1.110e-7 ("amp1e3-norm": the inner product, the FMA and the product by g, half an ulp each at worst)
MODEL_LLR_DISTANCE = 3.0e-7    # measured 2.343e-7 ("F2053-K1": the two distances' roundings meet in the difference)
# The GPU tolerances: four times those (the project's rule: the kernel may fuse where the model does not).
Z_TOL = 4 * MODEL_Z_DISTANCE
LLR_TOL = 4 * MODEL_LLR_DISTANCE
# Every payload symbol of every case (the NaN one excepted) keeps this distance, relative to |z|, from the nearest decision
# boundary of its table: far more than eight times MODEL_Z_DISTANCE, so that no rounding within Z_TOL can flip a bit and
# bits are compared exactly.  At SIGMA = 0.05 A a symbol nearer than that is a 15-sigma event; a case that violates it is
# replaced, not tolerated.
DECISION_MARGIN = 0.1
SIGMA = fr.SIGMA
WG = 256                       # lanes per workgroup of deframe_kernel (checked against comms_deframe_get_kernel)

WORD, THR, GUARD = "qpsk32", 0.5, 31
P = 32

DET_DTYPE = np.dtype([("index", np.uint64), ("corr_re", np.float32), ("corr_im", np.float32), ("metric", np.float32),
                      ("energy", np.float32)])       # comms_frame_detection_t

Case = collections.namedtuple("Case", "name y F offset lookback K table normalise scale cuts nan_at")


def word():
    return fr.words()[WORD]


def word_energy():
    p = word().astype(np.complex128)
    return float(np.sum(p.real ** 2 + p.imag ** 2))


def table_of(case):
    return rx_ref.default_table(case.K) if case.table is None else np.asarray(case.table, np.complex64)


# ------------------------------------------------------------------ bookkeeping: what a call emits
def bookkeeping(calls, F, offset, lookback):
    """calls: [(n, detections)].  Per call the detections whose frames it emits (start + F <= T_after, ascending), and the
    ones still pending at the end.  The refusal rules of the contract are asserted: no case breaks them."""
    T, pending, out = 0, [], []
    for n, dets in calls:
        for d in dets:
            start = int(d["index"]) + offset
            assert start >= T - lookback, "stale detection"
            assert not pending or int(d["index"]) > int(pending[-1]["index"]), "unordered detection"
            pending.append(d)
        T += n
        ready = [d for d in pending if int(d["index"]) + offset + F <= T]
        pending = pending[len(ready):]
        out.append(ready)
    return out, pending


def frame_values(d, normalise, Ep):
    """u (complex of two f32 values) and g (an f32 value) of a detection: f64, rounded once."""
    cr, ci = float(d["corr_re"]), float(d["corr_im"])
    mag = math.hypot(cr, ci)
    u = complex(float(np.float32(cr / mag)), float(np.float32(-ci / mag)))
    g = float(np.float32(Ep / mag)) if normalise else 1.0
    return u, g


def _empty(F, K):
    return dict(index=np.zeros(0, np.int64), start=np.zeros(0, np.int64), u=np.zeros(0, np.complex128), g=np.zeros(0), metric=np.zeros(0),
                z=np.zeros((0, F), np.complex128), values=np.zeros((0, F), np.int64), llr=np.zeros((0, F * K)))


def _frames(case, y, calls, per_frame):
    Ep = word_energy()
    emitted, pending = bookkeeping(calls, case.F, case.offset, case.lookback)
    out = []
    for ready in emitted:
        rec = _empty(case.F, case.K)
        if ready:
            rows = []
            for d in ready:
                start = int(d["index"]) + case.offset
                u, g = frame_values(d, case.normalise, Ep)
                rows.append((int(d["index"]), start, u, g, float(d["metric"])) + per_frame(y[start: start + case.F], u, g))
            rec = dict(index=np.array([r[0] for r in rows], np.int64), start=np.array([r[1] for r in rows], np.int64),
                       u=np.array([r[2] for r in rows]), g=np.array([r[3] for r in rows]), metric=np.array([r[4] for r in rows]),
                       z=np.stack([r[5] for r in rows]), values=np.stack([r[6] for r in rows]), llr=np.stack([r[7] for r in rows]))
        out.append(rec)
    return out, len(pending)


def ref_frames(case, y, calls):
    """The definition, f64: per call a dict of index, start, u, g, metric, z (frames x F), values (the decided indices) and
    llr (frames x F K, [j K + b]); and the number of frames left pending."""
    c = table_of(case).astype(np.complex128)
    K, s = case.K, float(np.float32(case.scale))

    def per_frame(sym, u, g):
        with np.errstate(invalid="ignore", over="ignore"):
            z = sym.astype(np.complex128) * u * g
            d = (z.real[:, None] - c.real[None, :]) ** 2 + (z.imag[:, None] - c.imag[None, :]) ** 2
            values = np.argmin(d, axis=1)                                   # the first minimum; a NaN row gives 0
            llr = np.empty((z.size, K))
            for b in range(K):
                one = ((np.arange(c.size) >> b) & 1).astype(bool)
                llr[:, b] = s * (np.min(d[:, one], axis=1) - np.min(d[:, ~one], axis=1))
        return z, values.astype(np.int64), llr.reshape(-1)

    return _frames(case, y, calls, per_frame)


def model_frames(case, y, calls):
    """deframe_kernel's arithmetic in numpy f32; the same structure as ref_frames (z and llr widened to f64)."""
    f32 = np.float32
    c = table_of(case)
    K, s = case.K, f32(case.scale)

    def per_frame(sym, u, g):
        sym = np.asarray(sym, np.complex64)
        yr, yi = sym.real.astype(f32), sym.imag.astype(f32)
        ur, ui = np.full(yr.size, u.real, f32), np.full(yr.size, u.imag, f32)
        with np.errstate(invalid="ignore", over="ignore"):
            zr = fr._fma(-yi, ui, yr * ur)
            zi = fr._fma(yi, ur, yr * ui)
            if case.normalise:
                zr, zi = zr * f32(g), zi * f32(g)
            z = np.empty(yr.size, np.complex64)
            z.real, z.imag = zr, zi
            d = [rx_ref.dist(z, ci) for ci in c]
            values = rx_ref.decide(z, c)
            llr = np.empty((z.size, K), f32)
            for b in range(K):
                best = [None, None]
                for i in range(c.size):                                     # ascending, replaced on a strictly smaller distance
                    w = (i >> b) & 1
                    best[w] = d[i] if best[w] is None else np.where(d[i] < best[w], d[i], best[w])
                llr[:, b] = s * (best[1] - best[0])
        return z.astype(np.complex128), values, llr.reshape(-1).astype(np.float64)

    return _frames(case, y, calls, per_frame)


def records(case, values):
    """The BITS records of frames x F decided values: packed LSB first, each frame padded with zeros to a multiple of 4 bytes."""
    nb = -(-case.F * case.K // 8)
    out = np.zeros((values.shape[0], -(-nb // 4) * 4), np.uint8)
    for f in range(values.shape[0]):
        out[f, :nb] = rx_ref.pack(values[f], case.K)
    return out


def boundary_margin(z, table):
    """Distance of every z from the nearest decision boundary of the table, relative to |z| (f64)."""
    c = np.asarray(table).astype(np.complex128)
    d = np.abs(z[:, None] - c[None, :]) ** 2
    best = np.argmin(d, axis=1)
    rows = np.arange(z.size)
    gap = (d - d[rows, best][:, None]) / (2 * np.maximum(np.abs(c[None, :] - c[best][:, None]), 1e-300))
    gap[rows, best] = np.inf
    return np.min(gap, axis=1) / np.abs(z)


# ------------------------------------------------------------------ detections and call plans
def detect(y):
    """framesync_ref.ref_detect of the flushed stream as comms_frame_detection_t records (the correlation rounded to f32)."""
    k, c, m, e, _ = fr.ref_detect(y, word(), THR, GUARD)
    out = np.zeros(k.size, DET_DTYPE)
    out["index"], out["corr_re"], out["corr_im"], out["metric"], out["energy"] = k, c.real, c.imag, m, e
    return out


def plan(y, dets, cuts):
    """[(n, detections)]: the stream cut at `cuts`; a detection goes to the call the frame synchroniser reports it in -- the
    first with T_after >= index + P + G -- and those it reports only when flushed go to a last call with n = 0."""
    edges = [0] + [c for c in cuts] + [y.size]
    calls, used = [], 0
    for a, b in zip(edges[:-1], edges[1:]):
        take = used
        while take < dets.size and int(dets["index"][take]) + P + GUARD <= b:
            take += 1
        calls.append((b - a, dets[used:take]))
        used = take
    if used < dets.size:
        calls.append((0, dets[used:]))
    return calls


# ------------------------------------------------------------------ cases
def _case(name, positions, length, F, K=2, A=1.0, theta=0.7, seed=1, normalise=False, table=None, cuts=(), lookback=GUARD - 1, scale=1.0,
          nan_at=None):
    y = fr.stream(word(), positions, length, A, theta, seed)
    if nan_at is not None:
        y = y.copy()
        y[nan_at] = np.complex64(complex(np.nan, 1.0))
        y.setflags(write=False)
    return Case(name, y, F, P, lookback, K, table, normalise, scale, tuple(cuts), nan_at)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    seed = 200
    # word, lane-group and workgroup edges: two frames, the second back to back with the first one's payload
    for F in (1, 15, 16, 17, 31, 32, 33, 2048 + 5):
        for K in (1, 2):
            seed += 1
            k2 = 5 + P + max(F, GUARD)      # detections are more than GUARD apart
            out.append(_case("F%d-K%d" % (F, K), [5, k2], k2 + P + F + 3, F, K, seed=seed, scale=0.5 * K))
    k, F = 40, 50
    # the frame synchroniser reports word k in the call with T_before < k + P + G: cut at the last such T_before, where the
    # payload starts exactly `lookback` = G - 1 symbols before the call
    out.append(_case("lookback-edge", [k], 400, F, cuts=[k + P + GUARD - 1], seed=231))
    out.append(_case("straddle", [k], 400, 100, cuts=[k + P + GUARD + 10], seed=232))           # 41 symbols in the history, 59 in the block
    out.append(_case("ends-at-T", [k], 400, 100, cuts=[k + P + 100], seed=233))
    out.append(_case("ends-at-T+1", [k], 400, 100, cuts=[k + P + 99, k + P + 100], seed=234))      # pending, then a call with n = 1
    out.append(_case("three-calls", [k], 400, 100, cuts=[k + P + GUARD, k + P + GUARD + 25, k + P + GUARD + 50], seed=235))   # H = 99
    out.append(_case("overlap", [k, k + P + 20], 400, 100, seed=236))                               # the second word inside the first payload
    out.append(_case("adjacent", [k, k + P + 24], 300, 24, K=2, seed=237))                          # records of 6 + 2 bytes, no shared symbol
    for A, tag in ((1e-3, "amp1e-3"), (1.0, "amp1"), (1e3, "amp1e3")):
        for nrm in (False, True):
            seed += 1
            out.append(_case(tag + ("-norm" if nrm else "-raw"), [k, 200], 330, 33, A=A, theta=-2.2, seed=seed, normalise=nrm, scale=2.0))
    out.append(_case("custom-table", [k, 200], 330, 33, A=1e3, theta=1.9, seed=251,
                     table=tuple((1e3 * rx_ref.QPSK_EX).astype(np.complex64).tolist()), scale=1e-6))
    out.append(_case("one-nan", [k], 300, 64, seed=252, nan_at=k + P + 37))
    n = 300
    out.append(_case("300-frames", [10 + 44 * i for i in range(n)], 10 + 44 * n + 20, 8, seed=253))
    Fb = 2048 + 5
    per = P + Fb + 3
    out.append(_case("past-the-grid", [7 + per * i for i in range(n)], 7 + per * n + 40, Fb, seed=254))
    assert len({c.name for c in out}) == len(out)
    return out


def case(name):
    return [i for i, cs in enumerate(cases()) if cs.name == name][0]


@functools.lru_cache(maxsize=None)
def detections(idx):
    d = detect(cases()[idx].y)
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def calls(idx):
    cs = cases()[idx]
    return plan(cs.y, detections(idx), list(cs.cuts))


@functools.lru_cache(maxsize=None)
def reference(idx):
    """ref_frames of case idx over its own call plan, computed once: (per-call records, frames left pending)."""
    cs = cases()[idx]
    return ref_frames(cs, cs.y, calls(idx))


def joined(per_call, key):
    return np.concatenate([r[key] for r in per_call])
