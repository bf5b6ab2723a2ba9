"""The definition of the OFDM synchroniser (include/comms_hip.h, "OFDM synchroniser") in numpy complex128 / float64, an f32
model of the kernels' order of summation and of the correct stage's rotor, and the streams, cases and bounds that
tests/test_ofdmsync_ref.py (no GPU), tests/test_gpu_ofdmsync.py and tests/test_gpu_dense_metrics.py (the model at every
position, bit for bit) share.  Nothing here touches the library."""
import functools

import numpy as np

import ofdm_ref as r

TILE = 2048               # decided positions per tile ("tile=" of kernel())
BLK = 32                  # absolute indices per block of prefix / suffix sums
RUN = 8                   # samples per f64 anchor of the correct stage
MAX_LAG, MAX_WINDOW, MAX_GUARD, MAX_ADVANCE, MAX_FRAME = 2048, 2048, 512, 2048, 1 << 20
DET_DTYPE = np.dtype([("index", np.int64), ("d", np.int64), ("P", np.complex128), ("R", np.float64), ("m", np.float64)])

# ---------------------------------------------------------------- the definition


def _extended(x, lo, hi, dtype):
    """x[i] for lo <= i < hi, zero outside the stream."""
    x = np.asarray(x)
    out = np.zeros(hi - lo, dtype)
    a, b = max(lo, 0), min(hi, x.size)
    if b > a:
        out[a - lo: b - lo] = x[a:b]
    return out


def ref_metric(x, L, W, d_lo, d_hi):
    """(P, R, m) of the positions d_lo <= d < d_hi (either may lie outside the stream, which is zero there)."""
    e = _extended(x, d_lo, d_hi + W + L, np.complex128)
    n = d_hi - d_lo + W - 1
    q = np.conj(e[:n]) * e[L: L + n]
    b = np.abs(e[:n]) ** 2 + np.abs(e[L: L + n]) ** 2
    cq = np.concatenate([[0], np.cumsum(q)])
    cb = np.concatenate([[0], np.cumsum(b)])
    if np.all(np.isfinite(e)):
        P, B = cq[W:] - cq[:-W], cb[W:] - cb[:-W]
    else:   # a NaN must reach the windows that hold it and no other
        P = np.array([q[i: i + W].sum() for i in range(d_hi - d_lo)])
        B = np.array([b[i: i + W].sum() for i in range(d_hi - d_lo)])
    R = 0.5 * B
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.where(R == 0, 0.0, np.abs(P) ** 2 / np.where(R == 0, 1.0, R) ** 2)
    return P, R, m


def peaks(m, G, thr, lo):
    """Indices k into m (m[k] is position lo + k) that win under the frame synchroniser's rule; m must reach G past either end."""
    out = []
    with np.errstate(invalid="ignore"):
        cand = np.flatnonzero(m >= thr)
    if G == 0:                      # no neighbours to beat: every candidate wins (the dense streams have thousands)
        return cand.astype(np.int64)
    for k in cand:
        if k - G < 0 or k + G >= m.size:
            continue
        with np.errstate(invalid="ignore"):
            if np.all(m[k] > m[k - G: k]) and np.all(m[k] >= m[k + 1: k + G + 1]):
                out.append(k)
    return np.array(out, np.int64)


def ref_detect(x, L, W, G, A, thr, origin=0, metric=None):
    """The detections of the whole stream followed by a flush: DET_DTYPE records, ascending."""
    x = np.asarray(x)
    lo, hi = -G, x.size + G + 1
    P, R, m = (metric or ref_metric)(x, L, W, lo, hi)
    out = []
    for k in peaks(m, G, np.float32(thr), lo):
        d = lo + int(k)
        if origin + A <= d <= x.size:
            out.append((d - A, d, P[k], R[k], m[k]))
    return np.array(out, DET_DTYPE)


def ref_cfo(P, L):
    return np.arctan2(np.imag(P), np.real(P)) / L


def ref_correct(records, cfo):
    x = np.asarray(records, np.complex128)
    n = np.arange(x.shape[-1])
    return x * np.exp(-1j * np.asarray(cfo, np.float64)[:, None] * n[None, :])

# ---------------------------------------------------------------- the f32 model of the chosen order


def fma32(a, b, c):
    """fma(a, b, c) of f32 arrays, rounded once.  The product of two f32 values is exact in f64; its f64 sum with c is rounded to
    53 bits, and rounding that to f32 is a second rounding that differs from the single one exactly where the f64 sum lands on
    the midpoint of two f32 values without being it: there the sum is moved one f64 step towards what it lost."""
    p, c = a.astype(np.float64) * b.astype(np.float64), c.astype(np.float64)
    t = p + c
    tie = (t.view(np.int64) & 0x1FFFFFFF) == 0x10000000
    if np.any(tie):
        p, c, s = np.broadcast_to(p, t.shape)[tie], np.broadcast_to(c, t.shape)[tie], t[tie]
        v = s - p
        lost = (p - (s - v)) + (c - v)                       # the exact sum minus its rounded value (Knuth's two-sum)
        t[tie] = np.where(lost == 0, s, np.nextafter(s, np.where(lost > 0, np.inf, -np.inf)))
    return t.astype(np.float32)


_fma = fma32


def model_metric(x, L, W, d_lo, d_hi):
    """ref_metric in the kernel's order: f32 products with its FMAs, prefix and suffix sums inside blocks of 32 absolute
    indices, P = (suf[d] + mid) + pre[e] with mid the full blocks ascending from +0, a direct sum where the window lies in one
    block.  (P, R, m) as complex64 / float32."""
    f32 = np.float32
    lo = d_lo - d_lo % BLK                                   # a multiple of 32, also below 0
    nblk = (d_hi + W - 1 - lo + BLK - 1) // BLK
    e = _extended(x, lo, lo + BLK * nblk + L, np.complex64)
    n = BLK * nblk
    ar, ai, cr, ci = e.real[:n], e.imag[:n], e.real[L: L + n], e.imag[L: L + n]
    q = [_fma(ai, ci, (ar * cr).astype(f32)), _fma(-ai, cr, (ar * ci).astype(f32)),
         _fma(ci, ci, _fma(cr, cr, _fma(ai, ai, (ar * ar).astype(f32))))]
    d = np.arange(d_lo, d_hi) - lo
    en = d + W - 1
    kd, ke = d // BLK, en // BLK
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for v in q:
            blocks = v.reshape(nblk, BLK)
            pre = np.cumsum(blocks, axis=1, dtype=f32)
            suf = np.cumsum(blocks[:, ::-1], axis=1, dtype=f32)[:, ::-1]
            F = pre[:, -1]
            mid = np.zeros(d.size, f32)
            for t in range(int(np.max(ke - kd)) if d.size else 0):
                use = kd + 1 + t < ke
                mid = np.where(use, (mid + F[np.minimum(kd + 1 + t, nblk - 1)]).astype(f32), mid)
            joined = ((suf.ravel()[d] + mid).astype(f32) + pre.ravel()[en]).astype(f32)
            direct = np.zeros(d.size, f32)
            if W <= BLK:
                for t in range(W):
                    direct = (direct + v[d + t]).astype(f32)
            out.append(np.where(ke == kd, direct, joined))
        pr, pi, B = out
        R = (f32(0.5) * B).astype(f32)
        num = ((pr * pr).astype(f32) + (pi * pi).astype(f32)).astype(f32)
        den = (R * R).astype(f32)
        m = np.where(R == 0, f32(0), num / np.where(R == 0, f32(1), den)).astype(f32)
    return (pr + 1j * pi).astype(np.complex64), R, m


def model_correct(records, cfo):
    """ref_correct with the kernel's phases: an f64 anchor at every eighth sample rounded to f32, stepped by the f32 rotor."""
    f32 = np.float32
    x = np.asarray(records, np.complex64)
    w = np.asarray(cfo, np.float64)
    n_frames, F = x.shape
    runs = -(-F // RUN)
    n0 = (np.arange(runs) * RUN).astype(np.float64)
    ang = -(w[:, None] * n0[None, :])
    c, s = np.cos(ang).astype(f32), np.sin(ang).astype(f32)
    c1, s1 = np.cos(w).astype(f32)[:, None], (-np.sin(w)).astype(f32)[:, None]
    xp = np.zeros((n_frames, runs * RUN), np.complex64)
    xp[:, :F] = x
    xr, xi = xp.real.reshape(n_frames, runs, RUN), xp.imag.reshape(n_frames, runs, RUN)
    out = np.zeros((n_frames, runs, RUN), np.complex64)
    for u in range(RUN):
        out[:, :, u] = _fma(-xi[:, :, u], s, (xr[:, :, u] * c).astype(f32)) + 1j * _fma(xi[:, :, u], c, (xr[:, :, u] * s).astype(f32))
        c, s = _fma(-s, np.broadcast_to(s1, s.shape), (c * c1).astype(f32)), _fma(s, np.broadcast_to(c1, s.shape), (c * s1).astype(f32))
    return out.reshape(n_frames, -1)[:, :F]

# ---------------------------------------------------------------- streams


def small_format(n_fft=64, n_cp=16, n_syms=4, seed=11):
    kind = r.map_80211a() if n_fft == 64 else r.map_generic(n_fft)
    return r.Format(n_fft, n_cp, kind, n_syms, 2, r.POLARITY, seed=seed)


SIGMA = 0.04      # per component: the frames' samples have power near 0.8 (52 of 64 carriers), |H|^2 near 1.2 -- about 25 dB


def build_stream(f, gaps, eps, seed, frames=None, sigma=SIGMA, tail=None):
    """Frames of format f (random data, or `frames` (n, frame_samples)) behind gaps[i] silent samples each, `tail` more at the
    end, through the three-tap channel of ofdm_ref over the whole stream, turned by e^{+i eps n}, plus seeded noise.
    Returns (stream complex64, the frames' first samples)."""
    rng = np.random.default_rng(seed)
    if frames is None:
        z = (rng.standard_normal((len(gaps), f.data_syms)) + 1j * rng.standard_normal((len(gaps), f.data_syms))) / np.sqrt(2)
        frames = r.ref_mod(f, z.astype(np.complex64))
    parts, starts, at = [], [], 0
    for g, fr in zip(gaps, np.asarray(frames, np.complex128)):
        parts += [np.zeros(g, np.complex128), fr]
        starts.append(at + g)
        at += g + fr.size
    parts.append(np.zeros(f.sym_len + 40 if tail is None else tail, np.complex128))
    s = np.concatenate(parts)
    y = np.convolve(s, r.H_TAPS)[: s.size] * np.exp(1j * eps * np.arange(s.size))
    y = y + sigma * (rng.standard_normal(s.size) + 1j * rng.standard_normal(s.size))
    return y.astype(np.complex64), np.array(starts, np.int64)


class Case:
    def __init__(self, name, L, W, G, A, thr, stream):
        self.name, self.L, self.W, self.G, self.A, self.thr, self.x = name, L, W, G, A, thr, stream

    args = property(lambda self: (self.L, self.W, self.thr, self.G, self.A))


@functools.lru_cache(maxsize=None)
def cases():
    """The streams of the GPU tests: the issue's (L, W, G, A) on 3 to 6 frames with gaps, the channel, a CFO of 0.3 pi / L and
    noise.  Seeds and gaps were chosen on the CPU so that no decision of the reference lies within 2 METRIC_BOUND of flipping
    (tests/test_ofdmsync_ref.py asserts it)."""
    f = small_format()
    big = small_format(1024, 256, 2, seed=12)
    even = f.train.copy()
    even[1::2] = 0                                           # training symbols of two identical halves: lag N / 2
    halves = f.but(train=even)
    out = []
    for name, (L, W, G, A), thr, fmt, gaps, seed in (
            ("sym80", (80, 80, 40, 8), 0.5, f, (200, 333, 90, 1500, 47), 1),
            ("half32", (32, 32, 16, 0), 0.5, halves, (100, 411, 77, 1203), 3),
            ("prefix64", (64, 16, 8, 4), 0.6, f, (150, 95, 612), 3),
            ("odd7", (7, 13, 3, 0), 0.3, f, (64, 201, 1111, 5, 330, 91), 4),
            ("sym1280", (1280, 1280, 512, 128), 0.5, big, (3000, 4100, 2222), 5)):
        x, _ = build_stream(fmt, gaps, 0.3 * np.pi / L, 100 + seed)
        out.append(Case(name, L, W, G, A, thr, x))
    return tuple(out)


def case(name):
    return next(cs for cs in cases() if cs.name == name)


@functools.lru_cache(maxsize=None)
def reference(name):
    cs = case(name)
    return ref_detect(cs.x, cs.L, cs.W, cs.G, cs.A, cs.thr)


def late_cut():
    """Where the sym80 stream is cut so that its last frame's guard window ends one sample after the cut."""
    cs = case("sym80")
    return int(reference("sym80")["d"][-1]) + cs.W + cs.L + cs.G - 1


def seam_stream():
    """sym80 frames whose peaks lie on the last decided position of tile 0, the first of tile 1 and one past it, in a stream fed
    whole (tile t of the single call decides the positions t TILE - (W + L + G) + 1 + [0, TILE)), and one in the ragged last
    tile of 2^20 + 3 samples."""
    f = small_format()
    first = TILE - (80 + 80 + 40) + 1                  # first decided position of tile 1
    n = (1 << 20) + 3
    starts = [first - 1, first + 2 * TILE, first + 4 * TILE + 1, n - 900]
    rng = np.random.default_rng(77)
    x = (SIGMA * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    z = (rng.standard_normal((len(starts), f.data_syms)) + 1j * rng.standard_normal((len(starts), f.data_syms))) / np.sqrt(2)
    fr = r.ref_mod(f, z.astype(np.complex64))
    for s0, v in zip(starts, fr):
        x[s0: s0 + v.size] += (v * np.exp(1j * 0.01 * np.arange(v.size))).astype(np.complex64)
    return x, np.array(starts, np.int64)


# ---------------------------------------------------------------- the correct stage's inputs
CORRECT_SHAPES = ((1, 257), (5, 3), (1280, 1), (1280, 257), (1 << 20, 1), (1 << 20, 3))   # (record length, frames)


def correct_input(F, n_frames):
    rng = np.random.default_rng(5000 + F + n_frames)
    x = ((rng.standard_normal((n_frames, F)) + 1j * rng.standard_normal((n_frames, F))) / np.sqrt(2)).astype(np.complex64)
    cfo = rng.uniform(-np.pi / 7, np.pi / 7, n_frames)
    cfo[0] = np.pi / 7
    if n_frames > 1:
        cfo[-1] = -np.pi / 7
    if n_frames > 2:
        cfo[1] = 0.0
    return x, cfo


def correct_distance(got, want, x):
    """max |got - want| / |x| over the samples."""
    return float(np.max(np.abs(np.asarray(got, np.complex128) - want) / np.abs(x)))


# Four times the worst distance of model_metric from ref_metric over cases() and seam_stream() -- of P and R relative to R, of
# m absolutely (the OFDM tests' rule for CHANNEL_BOUND).  tests/test_ofdmsync_ref.py measures it and holds the constant to it.
METRIC_MODEL_WORST = 6.68e-7           # sym1280; half32 5.41e-7, sym80 4.45e-7, link 4.94e-7, prefix64 4.46e-7, seams 3.06e-7, odd7 2.12e-7
#                                        (the dense streams below stay inside it at every position: at most 5.69e-7, (2048, 2048))
METRIC_BOUND = 4 * METRIC_MODEL_WORST
# Four times the worst correct_distance of model_correct from ref_correct over CORRECT_SHAPES.
CORRECT_MODEL_WORST = 4.09e-7          # 257 records of 1280; a record of 2^20 samples 3.52e-7
CORRECT_BOUND = 4 * CORRECT_MODEL_WORST

# ---------------------------------------------------------------- dense streams (tests/test_gpu_dense_metrics.py)
# With G = 0 the peak rule is "m >= thr": under a tiny threshold every position with a metric above 0 is a detection, and the
# kernel's sums show at every position.  The streams hold noise everywhere, so no window has R == 0 before the stream's end.
DENSE_N = 2 * TILE + 77                # positions whose whole reach W + L lies in the stream: two tiles and a ragged third
DENSE_THR = 1e-30
DENSE_SIGMA = 0.15                     # per component, against planted repetitions of power 1: their metric is near 0.9
DENSE_SHAPES = ((1, 2), (7, 13), (33, 31), (32, 32), (31, 33), (64, 65), (80, 80), (2048, 2048))     # (L, W)
DENSE_GUARD = 512                      # the large-guard layout of the residue runs
DENSE_RESIDUE_SHAPES = ((31, 33), (80, 80))
DENSE_LEAD = 4096                      # the residue runs start at position DENSE_LEAD + r, r = 0 .. 31
DENSE_FAR_SHAPES = ((7, 13), (31, 33), (2048, 2048))                 # run again at positions past 2^32
FAR_BASE, FAR_RESIDUES = 8192, (0, 1, 31)
FAR_SHIFTS = ((1 << 32) - 12288, 1 << 40, (1 << 62) - (1 << 20))     # multiples of 32; base + the first lies below 2^32
BRANCHES = ("direct", "ke0", "ke0+1")


@functools.lru_cache(maxsize=None)
def dense_stream(L, W):
    """DENSE_N + W + L - 1 samples of noise with a repetition of period L (W + L samples of power 1, turned by 0.3 pi / L per
    sample) added at 300 and 200 before the last full reach: positions 0 .. DENSE_N - 1 have their whole reach in the stream."""
    n = DENSE_N + W + L - 1
    rng = np.random.default_rng(7000 + 31 * L + W)
    x = DENSE_SIGMA * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    u = (rng.standard_normal(L) + 1j * rng.standard_normal(L)) / np.sqrt(2)
    i = np.arange(W + L)
    seg = u[i % L] * np.exp(1j * (0.3 * np.pi / L) * i)
    for at in (300, n - (W + L) - 200):
        x[at: at + W + L] += seg
    x = x.astype(np.complex64)
    x.setflags(write=False)
    return x


def behind_zeros(x, lead):
    """The stream a node sees that starts at position `lead` with zero state."""
    return np.concatenate([np.zeros(lead, np.complex64), x])


def dense_expected(x, L, W, G=0, lead=0, metric=model_metric):
    """The records of x behind `lead` zeros under DENSE_THR, in the kernel's order of operations (or the definition's)."""
    return ref_detect(behind_zeros(x, lead), L, W, G, 0, DENSE_THR, metric=metric)


@functools.lru_cache(maxsize=None)
def dense_model(L, W):
    """(P, R, m) of model_metric at the positions 0 .. len of dense_stream(L, W): position d at element d."""
    out = model_metric(dense_stream(L, W), L, W, 0, dense_stream(L, W).size + 1)
    for a in out:
        a.setflags(write=False)
    return out


def branch_of(d, W):
    """(lane column, branch) of the absolute positions d in ofdmsync_detect_kernel: a lane holds the eight positions from
    idx0 = d - d % 8, all in block kd; ke0 is the block of the first one's end.  0 direct (the window lies in one block),
    1 joined with the mid of [kd + 1, ke0), 2 joined with that mid extended by block ke0."""
    d = np.asarray(d, np.int64)
    kd, ke, ke0 = d // BLK, (d + W - 1) // BLK, (d - d % RUN + W - 1) // BLK
    return d % RUN, np.where(ke == kd, 0, np.where(ke == ke0, 1, 2))


def branch_classes(W):
    """Every (column, branch) that window W can produce: the pattern repeats with the block."""
    c, b = branch_of(np.arange(BLK), W)
    return sorted(set(zip(c.tolist(), b.tolist())))


def class_picks(L, W):
    """{(column, branch): d}: per class a position of dense_stream(L, W) whose whole reach lies in the stream and whose model
    metric lies between the 20th and the 80th percentile, so that a threshold of exactly m[d] splits thousands of positions on
    either side.  Class i of n takes the first such position at or behind i DENSE_N / (n + 1): they spread over the tiles."""
    m = dense_model(L, W)[2][:DENSE_N]
    lo, hi = np.percentile(m, [20, 80])
    d = np.flatnonzero((m >= lo) & (m <= hi))
    c, b = branch_of(d, W)
    classes = branch_classes(W)
    out = {}
    for i, (ci, bi) in enumerate(classes):
        hit = d[(c == ci) & (b == bi) & (d >= i * DENSE_N // (len(classes) + 1))]
        if hit.size:
            out[(ci, bi)] = int(hit[0])
    return out


def nan_reach(at, L, W):
    """The positions whose P or R holds sample `at`."""
    return np.unique(np.concatenate([np.arange(at - W + 1, at + 1), np.arange(at - L - W + 1, at - L + 1)]))


# ---------------------------------------------------------------- the link of check 8
LINK_FRAMES = 12
LINK_SYMS = 2                                   # data symbols per frame: 96 16-QAM values
LINK_M = 4
LINK_EPS = 0.3 * np.pi / 80
LINK_ADVANCE = 8
LINK_THRESHOLD, LINK_GUARD = 0.5, 40
LINK_SEED = 2028
LINK_SIGMA = 0.02                               # per component of the received samples
LINK_LLR_SCALE = 4.0                            # 1 / (2 s^2) for s = 0.35 at the table's scale: the equalised noise on a weak carrier
LINK_QSCALE = 0.5
LINK_CUTS = (0.23, 0.71)                        # the stream is fed in three uneven calls


def link_ofdm():
    return r.Format(64, 16, r.map_80211a(), LINK_SYMS, 2, r.POLARITY, cpe=True, seed=13)


@functools.lru_cache(maxsize=None)
def link_format():
    import crc_ref as cr
    import ratematch_ref as rr
    import viterbi_ref as vr

    p = cr.CATALOGUE["CRC24A"][0]
    pattern = rr.PATTERNS["3/4"]
    E = LINK_M * link_ofdm().data_syms           # 384 transmitted bits
    for T in range(1, 1000):
        info = T + p.W
        N = 2 * vr.n_steps(info, 7, True)
        src, _ = rr.build_map(N, pattern)
        if src.size == E:
            return dict(p=p, T=T, info=info, N=N, pattern=pattern, src=src, E=E, F=E // LINK_M)
    raise AssertionError("no payload length fills the OFDM frame")


@functools.lru_cache(maxsize=None)
def link_transmit():
    """payload bits, framed, coded, matched bits, data-carrier values (frames, data_syms)."""
    import crc_ref as cr
    import ratematch_ref as rr
    import symmap_ref as sm
    import viterbi_ref as vr

    f = link_format()
    payload = np.random.default_rng(LINK_SEED).integers(0, 2, (LINK_FRAMES, f["T"]), dtype=np.uint8)
    framed = cr.ref_attach(payload, f["p"])
    coded = vr.ref_encode(framed, 7, vr.GENS[(7, 2)])
    sent = rr.ref_tx(coded, f["src"])
    sym = sm.ref_map(sent, LINK_M, sm.qam_table(LINK_M))
    return payload, framed, coded, sent, sym


def link_gaps():
    return np.random.default_rng(LINK_SEED + 1).integers(30, 700, LINK_FRAMES)


def link_stream(frames):
    """The received stream of the transmitted `frames` (LINK_FRAMES, frame_samples)."""
    return build_stream(link_ofdm(), link_gaps(), LINK_EPS, LINK_SEED + 2, frames=frames, sigma=LINK_SIGMA)


def link_receive(z):
    """Equalised data-carrier values (frames, data_syms) -> (payload, passed, crc) on the references."""
    import crc_ref as cr
    import ratematch_ref as rr
    import symmap_ref as sm
    import viterbi_ref as vr

    f = link_format()
    llr = sm.ref_llr_records(np.asarray(z, np.complex64).ravel(), sm.qam_table(LINK_M), f["F"], LINK_LLR_SCALE)
    words = rr.ref_rx(llr.view(np.uint32), f["src"], f["N"])
    decoded, _ = vr.ref_decode(vr.ref_quantise(words.view(np.float32), LINK_QSCALE), 7, vr.GENS[(7, 2)], f["info"])
    return cr.ref_check(decoded, f["p"], f["T"])


def link_reference(x, correct=True):
    """The reference receive chain on stream x: detections, extracted records (derotated or not), equalised values, CRC results."""
    f = link_ofdm()
    sym = f.sym_len
    det = ref_detect(x, sym, sym, LINK_GUARD, LINK_ADVANCE, LINK_THRESHOLD)
    recs = np.stack([x[i: i + f.frame_samples] for i in det["index"] if i + f.frame_samples <= x.size]).astype(np.complex64)
    cfo = ref_cfo(det["P"], sym)[: recs.shape[0]]
    used = ref_correct(recs, cfo).astype(np.complex64) if correct else recs
    z = r.ref_demod(f, used).astype(np.complex64)
    return det, recs, cfo, z, link_receive(z)
