"""The tile planners of the three polyphase stream nodes restated in Python, and the case table of tests/test_gpu_tile_plans.py:
one case for every plan a planner can choose (no GPU here; tests/test_plan_cases.py holds the table to the rules below).

symsync_kernel, resample_kernel and channelizer_kernel plan their tile per handle: tile size, workgroup width, unroll factor, LDS
tier, padded or unpadded stride and whether taps or samples sit in LDS all follow from the format, and indexing, staging and the
store path differ between plans.  Every planner line restated here is listed in ANCHORS with its source text, so a change to a
planner fails tests/test_plan_cases.py until the port follows.

A plan is a tuple --
    symsync      (tier, TO, WG, U, padded)          tier: the LDS limit it was found under; padded: plan_stride's stride fitted
    resample     (dtype, tier, TO, WG, tab_lds)     tab_lds False: the planner's second try, the table left in global memory
    channelizer  (M, F, halvings, staged, tab_lds)  F = (2048 / M) >> halvings frames per tile
-- and a case is the smallest format of its plan within the enumerated domain, by (LDS bytes, taps, then the format's numbers).
The symsync domain is every (S, taps per phase) comms_symsync_create takes and the channelizer domain every (M, D, taps per
branch) of the kernel's range: nothing else enters their planners.  The resample domain is a SAMPLE of (L, M, taps per phase):
a plan that only other formats reach is not in its table."""
import collections
import functools

import numpy as np

CSRC = "comms_rs_amd/csrc/"
ANCHORS = [
    # ---- shared
    (CSRC + "stream_call.hpp", "static inline int tile_workgroup(int TO) { return TO >= 256 ? 256 : TO < 64 ? 64 : TO; }"),
    (CSRC + "common.hpp", "inline int plan_stride(int R, int len, int lanes = 32) {"),
    (CSRC + "common.hpp", "    for (int c = 0; c < lanes; ++c) {"),
    (CSRC + "common.hpp", "        const int stride = len + c;"),
    (CSRC + "common.hpp", "        for (int s0 = 0; s0 < R * lanes; s0 += lanes) {  // every phase alignment of a group (period R groups)"),
    (CSRC + "common.hpp", "                ++banks[((s % R) * stride + s / R) & (lanes - 1)];"),
    (CSRC + "common.hpp", "            cost += worst > 2 ? worst - 2 : 0;"),
    (CSRC + "common.hpp", "        if (best_cost < 0 || cost < best_cost) {"),
    # ---- symsync
    (CSRC + "symsync.hip", "constexpr size_t SS_MAX_PHASES = 256, SS_MAX_SPS = 256, SS_MAX_ROW = 1024;"),
    (CSRC + "symsync.hip", "constexpr size_t SS_LDS_FOUR = 40 * 1024;"),
    (CSRC + "symsync.hip", "constexpr size_t SS_LDS_MAX = 64 * 1024;"),
    (CSRC + "symsync.hip", "constexpr size_t SS_LDS_WIDE = 96 * 1024;"),
    (CSRC + "symsync.hip", "constexpr int SS_MIN_TILE = 32;"),
    (CSRC + "symsync.hip", "    for (size_t limit : {SS_LDS_FOUR, SS_LDS_MAX, SS_LDS_WIDE})"),
    (CSRC + "symsync.hip", "        for (int TO = 1024; TO >= (limit == SS_LDS_FOUR ? 256 : SS_MIN_TILE); TO /= 2) {"),
    (CSRC + "symsync.hip", "            if ((static_cast<size_t>(TO) + h->HB) * S * 8 > limit) continue;"),
    (CSRC + "symsync.hip", "            int stride = plan_stride(S, TO + h->HB, 16);"),
    (CSRC + "symsync.hip", "            if (static_cast<size_t>(S) * stride * 8 > limit) stride = TO + h->HB;  // the padding does not fit: unpadded does"),
    (CSRC + "symsync.hip", "            const size_t lds = static_cast<size_t>(S) * stride * 8;"),
    (CSRC + "symsync.hip", "    h->Q = (n_taps - 1) / L;"),
    (CSRC + "symsync.hip", "    h->NB = static_cast<int>((h->Q + 1 + 3) / 4);"),
    (CSRC + "symsync.hip", "    h->HB = static_cast<int>((4 * h->NB - 1 + S - 1) / S);"),
    (CSRC + "symsync.hip", "    h->WG = tile_workgroup(h->TO);"),
    (CSRC + "symsync.hip", "    h->U = h->TO >= 4 * h->WG ? 4 : h->TO >= 2 * h->WG ? 2 : 1;"),
    # ---- resample
    (CSRC + "resample.hip", "constexpr size_t RS_MAX_UP = 256, RS_MAX_DOWN = 256, RS_MAX_RATIO = 64, RS_MAX_TABLE = 24 * 1024;"),
    (CSRC + "resample.hip", "constexpr size_t RS_LDS_MAX = 64 * 1024;"),
    (CSRC + "resample.hip", "constexpr size_t RS_LDS_FOUR = 40 * 1024;"),
    (CSRC + "resample.hip", "size_t rs_samples(size_t TO, size_t L, size_t M, size_t NB) { return (L - 1 + (TO - 1) * M) / L + 4 * NB; }"),
    (CSRC + "resample.hip", "    for (size_t limit : {RS_LDS_FOUR, RS_LDS_MAX})"),
    (CSRC + "resample.hip", "        for (size_t TO = 1024; TO >= (limit == RS_LDS_FOUR ? 256u : 16u); TO /= 2) {"),
    (CSRC + "resample.hip", "            const size_t S = rs_samples(TO, L, M, NB), lds = tab_bytes + S * E;"),
    (CSRC + "resample.hip", "            if (lds > limit) continue;"),
    (CSRC + "resample.hip", "    h->series = L > RS_MAX_UP || M > RS_MAX_DOWN || M > RS_MAX_RATIO * L || L * QP * 4 > RS_MAX_TABLE;"),
    (CSRC + "resample.hip", "    h->NB = static_cast<int>((QP + 3) / 4);"),
    (CSRC + "resample.hip", "    h->RS = 4 * (h->NB | 1);  // RS / 4 odd"),
    (CSRC + "resample.hip", "    h->tab_lds = plan_tile(h.get(), tab_floats * 4);"),
    (CSRC + "resample.hip", "    if (!h->tab_lds && !plan_tile(h.get(), 0))"),
    (CSRC + "resample.hip", "    h->WG = tile_workgroup(h->TO);"),
    # ---- channelizer
    (CSRC + "channelizer.hip", "constexpr size_t CHZ_MAX_M = 1024;"),
    (CSRC + "channelizer.hip", "constexpr size_t CHZ_TAPS_PER_M = 16;"),
    (CSRC + "channelizer.hip", "constexpr size_t CHZ_RATE_PER_M = 4;"),
    (CSRC + "channelizer.hip", "constexpr size_t CHZ_TILE = 2048;"),
    (CSRC + "channelizer.hip", "constexpr size_t CHZ_LDS_MAX = 64 * 1024;"),
    (CSRC + "channelizer.hip", "constexpr size_t CHZ_TAB_LDS = 16 * 1024;"),
    (CSRC + "channelizer.hip", "    const size_t M = h->M, D = h->D, QM = static_cast<size_t>(h->Q) * M, MS = M + 1;"),
    (CSRC + "channelizer.hip", "    const size_t tab = QM * 4 <= CHZ_TAB_LDS ? QM * 4 : 0;"),
    (CSRC + "channelizer.hip", "    const size_t F0 = CHZ_TILE / M;"),
    (CSRC + "channelizer.hip", "    for (size_t F = F0; F >= 1; F /= 2) {"),
    (CSRC + "channelizer.hip", "        const size_t S = (F - 1) * D + QM;"),
    (CSRC + "channelizer.hip", "        const size_t lds = tab + (F * MS + std::max(F * MS, S)) * 8;"),
    (CSRC + "channelizer.hip", "        if (lds > CHZ_LDS_MAX) continue;"),
    (CSRC + "channelizer.hip", "    h->lds = tab + 2 * F0 * MS * 8;"),
    (CSRC + "channelizer.hip", "        h->Q = static_cast<int>((n_taps + M - 1) / M);"),
]

KIB = 1024


def tile_workgroup(TO):
    return 256 if TO >= 256 else 64 if TO < 64 else TO


@functools.lru_cache(maxsize=None)
def _stride_pad(R, len_mod, lanes):
    """plan_stride's choice as stride - len: the banks depend on the stride modulo `lanes` only."""
    s = np.arange(R * lanes, dtype=np.int64)
    group = s // lanes
    best, best_cost = 0, -1
    for c in range(lanes):
        stride = len_mod + c
        banks = ((s % R) * stride + s // R) & (lanes - 1)
        worst = np.bincount(group * lanes + banks, minlength=R * lanes).reshape(R, lanes).max(axis=1)
        cost = int(np.sum(np.maximum(worst - 2, 0)))
        if best_cost < 0 or cost < best_cost:
            best_cost, best = cost, c
    return best


def plan_stride(R, length, lanes=32):
    return length + _stride_pad(R, length % lanes, lanes)


# ---------------------------------------------------------------- symsync
SS_MAX_PHASES = SS_MAX_SPS = 256
SS_MAX_ROW = 1024
SS_LDS_FOUR, SS_LDS_MAX, SS_LDS_WIDE = 40 * KIB, 64 * KIB, 96 * KIB
SS_MIN_TILE = 32
SS_TIERS = {SS_LDS_FOUR: "40K", SS_LDS_MAX: "64K", SS_LDS_WIDE: "96K"}

SsPlan = collections.namedtuple("SsPlan", "tier TO WG U padded")
SsTile = collections.namedtuple("SsTile", "plan lds stride HB NB Q")


@functools.lru_cache(maxsize=None)
def symsync_tile(L, S, N):
    """comms_symsync_create's plan for N taps over L phases at S samples per symbol."""
    assert 1 <= L <= SS_MAX_PHASES and 1 <= S <= SS_MAX_SPS and 1 <= N <= SS_MAX_ROW * L
    Q = (N - 1) // L
    NB = (Q + 1 + 3) // 4
    HB = (4 * NB - 1 + S - 1) // S
    for limit in (SS_LDS_FOUR, SS_LDS_MAX, SS_LDS_WIDE):
        TO = 1024
        while TO >= (256 if limit == SS_LDS_FOUR else SS_MIN_TILE):
            if (TO + HB) * S * 8 <= limit:
                stride = plan_stride(S, TO + HB, 16)
                padded = S * stride * 8 <= limit
                if not padded:
                    stride = TO + HB
                WG = tile_workgroup(TO)
                U = 4 if TO >= 4 * WG else 2 if TO >= 2 * WG else 1
                return SsTile(SsPlan(SS_TIERS[limit], TO, WG, U, padded), S * stride * 8, stride, HB, NB, Q)
            TO //= 2
    raise AssertionError("symsync: no tile fits (%d, %d, %d)" % (L, S, N))


SS_L = 4                                         # the plan depends on the taps per phase, not on L: every case has four phases
SS_ROWS = tuple(range(1, SS_MAX_ROW + 1))        # taps per phase: every count comms_symsync_create takes


def symsync_domain():
    """(L, S, N): every S crossed with every number of taps per phase -- the plan follows from (S, taps per phase) alone."""
    return [(SS_L, S, SS_L * row) for S in range(1, SS_MAX_SPS + 1) for row in SS_ROWS]


def _smallest(domain, tile_of, taps_of):
    """plan -> its smallest format: fewest LDS bytes, then fewest taps, then the format's own numbers."""
    best = {}
    for f in domain:
        t = tile_of(*f)
        key = (t.lds, taps_of(f), f)
        if t.plan not in best or key < best[t.plan][0]:
            best[t.plan] = (key, f)
    return {p: f for p, (_, f) in best.items()}


@functools.lru_cache(maxsize=None)
def symsync_plans():
    return _smallest(symsync_domain(), symsync_tile, lambda f: f[2])


# (L, S, N): the smallest format of every plan ...
SYMSYNC_CASES = ((4, 1, 4), (4, 4, 4068), (4, 5, 4), (4, 9, 1988), (4, 10, 4), (4, 18, 1940), (4, 19, 996), (4, 28, 3924), (4, 32, 4), (4, 60, 1684),
                 (4, 64, 4), (4, 119, 1428), (4, 127, 4), (4, 222, 2660), (4, 241, 964))
# ... which has one tap per phase on most padded-stride plans.  The same plans at 33 taps per phase (nine blocks of four, a halo of
# several outputs) and at S that do not divide the workgroup: dp = WG mod S != 0, and de = 0 from S = 65
SYMSYNC_MORE = ((4, 5, 132), (4, 10, 132), (4, 20, 132), (4, 63, 132), (4, 126, 132), (4, 248, 132))


# ---------------------------------------------------------------- resample
RS_MAX_UP = RS_MAX_DOWN = 256
RS_MAX_RATIO = 64
RS_MAX_TABLE = 24 * KIB
RS_LDS_FOUR, RS_LDS_MAX = 40 * KIB, 64 * KIB

RsPlan = collections.namedtuple("RsPlan", "dtype tier TO WG tab_lds")
RsTile = collections.namedtuple("RsTile", "plan lds S NB RS Q")
ELEM = {"f32": 4, "c32": 8}


def resample_in_range(L, M, N):
    QP = (N - 1) // L + 1
    return not (L > RS_MAX_UP or M > RS_MAX_DOWN or M > RS_MAX_RATIO * L or L * QP * 4 > RS_MAX_TABLE)


def rs_samples(TO, L, M, NB):
    return (L - 1 + (TO - 1) * M) // L + 4 * NB


@functools.lru_cache(maxsize=None)
def resample_tile(L, M, N, dtype):
    """comms_resample_create's plan: the tile beside the table in LDS, or -- the second try -- with the table in global memory."""
    assert resample_in_range(L, M, N)
    E = ELEM[dtype]
    Q = (N - 1) // L
    NB = (Q + 1 + 3) // 4
    RS = 4 * (NB | 1)
    for tab_lds, tab_bytes in ((True, L * RS * 4), (False, 0)):
        for limit in (RS_LDS_FOUR, RS_LDS_MAX):
            TO = 1024
            while TO >= (256 if limit == RS_LDS_FOUR else 16):
                S = rs_samples(TO, L, M, NB)
                lds = tab_bytes + S * E
                if lds <= limit:
                    tier = "40K" if limit == RS_LDS_FOUR else "64K"
                    return RsTile(RsPlan(dtype, tier, TO, tile_workgroup(TO), tab_lds), lds, S, NB, RS, Q)
                TO //= 2
    raise AssertionError("resample: no tile fits (%d, %d, %d)" % (L, M, N))


RS_SWEEP_L = (1, 2, 3, 4, 5, 6, 7, 16, 21, 64, 147, 256)
# taps per phase: a few short rows, every 37th count, and 5440 -- one phase of 5440 Complex<f32> taps leaves room for 16 samples
# beside its table and no more
RS_SWEEP_ROWS = tuple(sorted({1, 2, 4, 5, 16, 33, 129, 512, 1024, 1536, 3072, 5440, 6144, *range(1, 6145, 37)}))


def resample_domain():
    """A SAMPLE of the kernel's range: the L above, every M, the rows above (N = L row), both dtypes."""
    return [(L, M, L * row, dt) for dt in ("f32", "c32") for L in RS_SWEEP_L for M in range(1, RS_MAX_DOWN + 1) for row in RS_SWEEP_ROWS
            if resample_in_range(L, M, L * row)]


@functools.lru_cache(maxsize=None)
def resample_plans():
    return _smallest(resample_domain(), resample_tile, lambda f: f[2])


# (L, M, N, dtype): the smallest format of every plan of the sample ...
RESAMPLE_CASES = ((1, 1, 4996, "f32"), (1, 1, 5477, "c32"), (1, 3, 5440, "c32"), (1, 5, 1, "c32"), (1, 6, 5403, "c32"), (1, 8, 4108, "f32"),
                  (1, 11, 5403, "c32"), (1, 23, 5292, "c32"), (1, 52, 4959, "c32"), (1, 64, 33, "f32"), (1, 64, 2776, "c32"), (1, 64, 4145, "c32"),
                  (1, 64, 4145, "f32"), (2, 20, 2, "f32"), (2, 64, 32, "c32"), (2, 128, 66, "c32"), (3, 1, 6108, "c32"), (3, 59, 114, "c32"),
                  (4, 40, 4, "c32"), (5, 100, 5, "f32"), (6, 24, 6144, "c32"), (6, 210, 1116, "f32"), (16, 1, 16, "f32"), (21, 1, 21, "c32"))
# ... and the tile of 256 outputs, one trip per lane, with several blocks of taps: both tiers, and phases that do not divide the rate
RESAMPLE_MORE = ((1, 10, 16, "c32"), (1, 20, 16, "c32"), (3, 31, 16, "c32"), (3, 31, 16, "f32"))
# The plans the planner's loops could name and no format of the sample reaches (none was found in a sweep of every L either): f32
# with a tile of 32 or 16 or with the table in global memory, Complex<f32> with the table in global memory and a tile of 16.


# ---------------------------------------------------------------- channelizer
CHZ_MAX_M = 1024
CHZ_TAPS_PER_M = 16
CHZ_RATE_PER_M = 4
CHZ_TILE = 2048
CHZ_LDS_MAX = 64 * KIB
CHZ_TAB_LDS = 16 * KIB

ChzPlan = collections.namedtuple("ChzPlan", "M F halvings staged tab_lds")
ChzTile = collections.namedtuple("ChzTile", "plan lds S Q")


@functools.lru_cache(maxsize=None)
def channelizer_tile(M, D, N):
    assert 2 <= M <= CHZ_MAX_M and M & (M - 1) == 0 and 1 <= N <= CHZ_TAPS_PER_M * M and 1 <= D <= CHZ_RATE_PER_M * M
    Q = (N + M - 1) // M
    QM, MS = Q * M, M + 1
    tab = QM * 4 if QM * 4 <= CHZ_TAB_LDS else 0
    F0 = CHZ_TILE // M
    F, halvings = F0, 0
    while F >= 1:
        S = (F - 1) * D + QM
        lds = tab + (F * MS + max(F * MS, S)) * 8
        if lds <= CHZ_LDS_MAX:
            return ChzTile(ChzPlan(M, F, halvings, True, tab != 0), lds, S, Q)
        F //= 2
        halvings += 1
    return ChzTile(ChzPlan(M, F0, 0, False, tab != 0), tab + 2 * F0 * MS * 8, 0, Q)


def channelizer_domain():
    """(M, D, N): every M of the kernel, every rate D = 1 .. 4 M, every number of taps per branch Q = 1 .. 16 (N = Q M: the plan
    takes N through Q = ceil(N / M) alone)."""
    return [(1 << lg, D, Q * (1 << lg)) for lg in range(1, 11) for D in range(1, CHZ_RATE_PER_M * (1 << lg) + 1) for Q in range(1, CHZ_TAPS_PER_M + 1)]


@functools.lru_cache(maxsize=None)
def channelizer_plans():
    return _smallest(channelizer_domain(), channelizer_tile, lambda f: f[2])


# (M, D, N): the smallest format of every plan ...
CHANNELIZER_CASES = ((2, 1, 2), (2, 5, 4), (4, 1, 4), (4, 11, 8), (8, 1, 8), (8, 23, 16), (16, 1, 16), (16, 47, 32), (32, 1, 32), (32, 96, 32),
                     (64, 1, 64), (64, 195, 64), (128, 1, 128), (128, 396, 128), (256, 1, 256), (256, 822, 256), (256, 981, 2816), (512, 1, 512),
                     (512, 1, 4608), (512, 1, 7680), (512, 511, 4608), (512, 1791, 512), (512, 1791, 3584), (512, 2047, 5120), (1024, 1, 1024),
                     (1024, 1, 5120), (1024, 1, 7168), (1024, 1023, 5120), (1024, 3071, 2048))
# ... which has one or two taps per branch in most halved tiles.  Halved tiles at the largest rate and with several taps per branch, ragged
CHANNELIZER_MORE = ((2, 8, 2), (64, 256, 64), (8, 31, 35), (16, 64, 67), (256, 1023, 1000))


# ---------------------------------------------------------------- the streams of tests/test_gpu_tile_plans.py
def call_outputs(TO):
    """Outputs (symbols, samples, frames) of the calls of one stream: one, a tile less one, a tile, a tile and one, three tiles and five."""
    return [k for k in (1, TO - 1, TO, TO + 1, 3 * TO + 5) if k > 0]


def symsync_mus(L, S):
    """0, L + 3 (q = 1), the last one, and one with 1 < q < S - 1 where there is one."""
    out = {0, (S - 1) * L + L - 1}
    if L + 3 < S * L:
        out.add(L + 3)
    if S >= 4:
        out.add((S // 2) * L + 1)
    return sorted(out)


def resample_len(k, L, M):
    """Input samples of a call that writes k outputs (the nearest count below where none gives exactly k)."""
    return max(1, k * M // L)


BITS_N_SYM = (1, 31, 32, 33)


def bits_n_sym(TO):
    return sorted({*BITS_N_SYM, TO - 1, TO, TO + 1, 3 * TO + 5})
