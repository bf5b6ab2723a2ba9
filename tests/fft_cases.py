"""Which kernels an FFT length runs on, restated from the dispatch code, and the case tables of tests/test_gpu_fft_lengths.py
drawn from that rule (no GPU here; tests/test_fft_cases.py holds the tables to the rule).

`family_f32(n)` restates fft_setup / pow2_plan_build / pow2_run / comms_fft_run_dev (csrc/fft.hip), `family_f64(n)` restates
fft_f64_prepare / pow2_run / comms_fft_f64_run_dev (csrc/fft_f64.hip).  Every threshold used here is listed in ANCHORS with the
source text it restates; the CPU test looks each text up in the source, so a threshold that moves in the code fails there
rather than leaving a table that no longer crosses its seam.

A case is (n, batches, in_place): transform length, the batch counts to run it at, and whether the in-place run is checked
too (bitwise against the out-of-place one)."""

# ---------------------------------------------------------------- thresholds (see ANCHORS for the source text of each)
NUM_CU = 256                 # common.hpp: kNumCU
F32_DIRECT_MAX = 64          # fft_setup: default of COMMS_FFT_DIRECT_MAX
F32_BLU_MAX_N = 1 << 23      # fft_setup: Bluestein refuses longer transforms
F32_BLU_CHUNK_POINTS = 1 << 24   # comms_fft_run_dev: chunk = 2^24 / M padded transforms per pass of the Bluestein loop
F32_TILE_POINTS = 16384      # launch_rx: points per tile of fft_rx1024_kernel
F32_RX_GRID = NUM_CU         # launch_rx: full tiles run on at most kNumCU workgroups
F32_DIRECT_GROUP_CAP = 8 * NUM_CU  # comms_fft_run_dev: dft_small_kernel's grid, in groups of G = 256 / N transforms
F64_LDS_POINTS = 4096        # fft_f64.hip: one pass through LDS up to here; the DFT sum up to here
F64_MAX_P = 1 << 24          # fft_f64_prepare: the largest power-of-two transform
F64_FOUR_STEP_PIECE = 64     # pow2_run: transforms per column + row pass pair
F64_ONE_PASS_PIECE = 1 << 20  # pow2_run: transforms per launch of the one-pass form
F64_DFT_PIECE = 32768        # comms_fft_f64_run_dev: transforms per launch of the DFT sum

FFT_HIP = "comms_rs_amd/csrc/fft.hip"
FFT_F64_HIP = "comms_rs_amd/csrc/fft_f64.hip"
COMMON_HPP = "comms_rs_amd/csrc/common.hpp"

# (file, function the text stands in, text) -- the source lines the rules below restate
ANCHORS = [
    (COMMON_HPP, "kNumCU", "constexpr int kNumCU = 256;"),
    (FFT_HIP, "fft_setup", 'diag_knob("COMMS_FFT_DIRECT_MAX", 64)'),
    (FFT_HIP, "fft_setup", "if (N <= direct_max && N <= 4096) {"),
    (FFT_HIP, "fft_setup", 'COMMS_ARG(N <= (static_cast<size_t>(1) << 23), "FFT length %zu too large", N);'),
    (FFT_HIP, "fft_setup", "while (M < 2 * N - 1) M <<= 1;"),
    (FFT_HIP, "pow2_plan_build", "COMMS_ARG(logN <= 24,"),
    (FFT_HIP, "pow2_plan_build", "const bool rx = (N >= 2 && N <= 32) || N == 64 || N == 128 || N == 256 || N == 512 || N == 1024 || "
                                 "N == 2048 || N == 4096 || N == 8192 || N == 16384;"),
    (FFT_HIP, "pow2_plan_build", "if (N == 32768 && pl.d_fw1) {"),
    (FFT_HIP, "pow2_plan_build", "} else if (logN > 20) {"),
    (FFT_HIP, "pow2_plan_build", "const int log1 = (logN >= 15 && logN <= 20) ? logN - 10 : logN / 2, log2v = logN - log1;"),
    (FFT_HIP, "pow2_plan_build", "(pl.pass[0].L == 64 || pl.pass[0].L == 128 || pl.pass[0].L == 256 || pl.pass[0].L == 512)) {"),
    (FFT_HIP, "pow2_run", 'diag_knob("COMMS_FFT_LARGE_GATHER", 23)'),
    (FFT_HIP, "launch_rx", "const size_t n_full = n_points / 16384, rem = n_points % 16384;"),
    (FFT_HIP, "launch_rx", "n_full < static_cast<size_t>(kNumCU) ? n_full : kNumCU"),
    (FFT_HIP, "comms_fft_run_dev", "size_t chunk = (static_cast<size_t>(1) << 24) / M;"),
    (FFT_HIP, "comms_fft_run_dev", "const bool fuse = h->plan.rx_rad != 0 && !no_fuse;"),
    (FFT_HIP, "comms_fft_run_dev", "if (h->N <= 128) {"),
    (FFT_HIP, "comms_fft_run_dev", "groups < 8u * kNumCU ? groups : 8u * kNumCU"),
    (FFT_HIP, "comms_fft_run_dev", "(batch + 256 / h->N - 1) / (256 / h->N)"),
    (FFT_F64_HIP, "F64_LDS_POINTS", "constexpr int F64_LDS_POINTS = 4096;"),
    (FFT_F64_HIP, "fft_f64_prepare", "h->kind = pow2 ? (N <= 4096 ? 0 : 1) : (N <= 4096 ? 2 : 3);"),
    (FFT_F64_HIP, "fft_f64_prepare", "while (P < 2 * N - 1) P <<= 1;"),
    (FFT_F64_HIP, "fft_f64_prepare", "COMMS_ARG(P <= (static_cast<size_t>(1) << 24),"),
    (FFT_F64_HIP, "fft_f64_prepare", "h->logN1 = (h->logP + 1) / 2, h->logN2 = h->logP - h->logN1;"),
    (FFT_F64_HIP, "fft_f64_prepare", "h->h = h->logP / 2;"),
    (FFT_F64_HIP, "pow2_run", "if (h->logP <= 12) {"),
    (FFT_F64_HIP, "pow2_run", "for (size_t b0 = 0; b0 < batch; b0 += 1u << 20) {"),
    (FFT_F64_HIP, "pow2_run", "for (size_t b0 = 0; b0 < batch; b0 += 64) {"),
    (FFT_F64_HIP, "pow2_run", "p.B = F64_LDS_POINTS / p.N < 16 ? F64_LDS_POINTS / p.N : 16;"),
    (FFT_F64_HIP, "comms_fft_f64_run_dev", "for (size_t b0 = 0; b0 < batch; b0 += 32768) {"),
]


def is_pow2(n):
    return n >= 1 and n & (n - 1) == 0


def ilog2(n):
    return (n - 1).bit_length()


def padded(n):
    """Bluestein's power-of-two length (fft_setup: `while (M < 2 * N - 1) M <<= 1`; fft_f64_prepare: the same for P)."""
    m = 1
    while m < 2 * n - 1:
        m <<= 1
    return m


def _pow2_form_f32(length):
    """The form a power-of-two transform of `length` points runs on, with or without Bluestein around it."""
    log = ilog2(length)
    if length <= 32:          # pow2_plan_build: `rx = (N >= 2 && N <= 32) || ...` -> rx_rad = -100 - N, the in-register forms
        return "tiny"
    if length <= 16384:       # pow2_plan_build: `rx = ... N == 64 || ... || N == 16384`; pow2_run: `if (pl.rx_rad && !no_rx)`
        return "rx%d" % length  # (one instantiation of fft_rx1024_kernel per length: RAD 0, 128, 256, 512, 1, 2, 4, 8, 16)
    if length == 32768:       # pow2_plan_build: `if (N == 32768 && pl.d_fw1)`; pow2_run: `if (pl.d_rx32 && !no_rx32k)`
        return "rx32k"
    if log <= 19:             # pow2_plan_build: log1 = logN - 10 -> N1 = 64 ... 512 -> col_kind set: fft_cols_kernel + 1024-point rows
        return "cols_2p%d" % log
    if log == 20:             # N1 = N2 = 1024: both passes on fft1024x16_kernel (pl.fast(i)), no column kernel
        return "fast_2p20"
    if log <= 23:             # pow2_plan_build: `else if (logN > 20)`; pow2_run: `ilog2(pl.N) <= gather_max` (23): gathered columns + rows
        return "gather_2p%d" % log
    if log == 24:             # pow2_run: columns, rows in place, transpose
        return "three_2p24"
    raise ValueError("power-of-two FFT supports up to 2^24 points")  # pow2_plan_build: COMMS_ARG(logN <= 24, ...)


def family_f32(n):
    """Label of the kernels FFTBatchNode(n) runs; ValueError where comms_fft_create refuses."""
    if n < 1:                 # comms_fft_create: COMMS_ARG(fft_size >= 1, ...)
        raise ValueError("fft_size must be >= 1")
    if is_pow2(n):            # fft_setup: `if ((N & (N - 1)) == 0)` -> kind 0
        if n == 1:            # comms_fft_run_dev: `if (h->N == 1)`: a copy
            return "pow2_copy"
        return "pow2_" + _pow2_form_f32(n)
    if n <= F32_DIRECT_MAX:   # fft_setup: `if (N <= direct_max && N <= 4096)` -> kind 1; run_dev: `if (h->N <= 128)`: dft_small_kernel
        return "direct"
    if n > F32_BLU_MAX_N:     # fft_setup: COMMS_ARG(N <= (1 << 23), "FFT length %zu too large")
        raise ValueError("FFT length too large")
    m = padded(n)
    form = _pow2_form_f32(m)  # fft_setup: pow2_plan_build(h->plan, M)
    if form.startswith("rx") and form != "rx32k":  # run_dev: `fuse = h->plan.rx_rad != 0`: two launches of fft_rx1024_kernel, modes 1 and 2
        return "blu_fused_M%d" % m
    if form == "rx32k":
        return "blu_rx32k"
    kind, log = form.split("_")  # unfused: blu_pre_kernel, pow2_run, blu_mul_kernel, pow2_run, blu_post_kernel
    return "blu_%s_M%s" % (kind, log)


def family_f64(n):
    """Label of the kernels FFTBatchNodeF64(n) runs; ValueError where comms_fft_f64_create refuses."""
    if n < 1:                 # comms_fft_f64_create: COMMS_ARG(fft_size >= 1, ...)
        raise ValueError("fft_size must be >= 1")
    if is_pow2(n):            # fft_f64_prepare: `h->kind = pow2 ? (N <= 4096 ? 0 : 1) : ...`
        if n <= F64_LDS_POINTS:   # pow2_run: `if (h->logP <= 12)`: one pass of fft_f64_lds_kernel
            return "lds"
        if n > F64_MAX_P:     # fft_f64_prepare: COMMS_ARG(P <= (1 << 24), ...)
            raise ValueError("the limit is 2^24")
        return "four_step_%d" % ilog2(n)  # logN1 = (logP + 1) / 2, twiddle split h = logP / 2: different for every size
    if n <= F64_LDS_POINTS:   # fft_f64_prepare: `... : (N <= 4096 ? 2 : 3)`: dft_f64_direct_kernel
        return "dft_sum"
    p = padded(n)             # fft_f64_prepare: `while (P < 2 * N - 1) P <<= 1`
    if p > F64_MAX_P:
        raise ValueError("the limit is 2^24")
    return "blu_P2p%d" % ilog2(p)  # per transform: blue_in, four-step forward, blue_mul, four-step inverse, blue_out


def _seam_lengths(limit):
    """Lengths at which a family can change: the rules above depend on n only through `n is a power of two`, the direct
    threshold and the padded length, which steps at 2^k + 1."""
    ns = set(range(1, F32_DIRECT_MAX + 3))
    k = 1
    while k <= limit:
        ns.update((k - 1, k, k + 1))
        k <<= 1
    ns.update((F64_LDS_POINTS - 1, F64_LDS_POINTS + 1))
    return sorted(v for v in ns if v >= 1)


def all_families(family, limit=1 << 25):
    out = set()
    for n in _seam_lengths(limit):
        try:
            out.add(family(n))
        except ValueError:
            pass
    return out


def direct_group(n):
    """Transforms per workgroup of dft_small_kernel (`const int G = 256 / N`)."""
    return 256 // n


def tile_xforms(n):
    """Padded transforms per 16384-point tile of the fused Bluestein form (1 where a transform is a tile)."""
    return max(F32_TILE_POINTS // padded(n), 1)


def _non_pow2(lo, hi):
    return [n for n in range(lo, hi + 1) if not is_pow2(n)]


def _fused_batches(n):
    xpt = tile_xforms(n)
    return tuple(sorted({1, xpt + 1, 2 * xpt + 3} | ({xpt - 1} if xpt - 1 >= 1 else set())))


FUSED_LENGTHS = (65, 127, 129, 255, 257, 511, 513, 1023, 1025, 2047, 2049, 4095, 4097, 8191)  # M / 4 + 1 and M / 2 - 1, M = 256 ... 16384


def past_rx_grid(n):
    """Smallest batch of the fused form whose full tiles outnumber launch_rx's grid (blocks = min(n_full, kNumCU))."""
    return (F32_RX_GRID + 1) * tile_xforms(n)


F32_GROUPS = {
    # dft_small_kernel at every length it serves: two full groups of G transforms and a ragged one
    "direct_every_length": [(n, (2 * direct_group(n) + 1,), False) for n in _non_pow2(3, F32_DIRECT_MAX - 1)],
    # ... and with more groups than its grid of 8 * kNumCU workgroups: the group loop's second trip
    "direct_grid_cap": [(n, (2 * F32_DIRECT_GROUP_CAP * direct_group(n) + 3,), False) for n in (3, 63)],
    # fused Bluestein at both edge lengths of every padded length, around a tile's worth of transforms
    "blu_fused": [(n, _fused_batches(n), False) for n in FUSED_LENGTHS],
    # ... and with more full tiles than workgroups: the persistent loop's second trip in both modes
    "blu_fused_grid": [(n, (past_rx_grid(n),), False) for n in (129, 8191)],
    # unfused Bluestein: M = 2^15 (one pass), 2^16 ... 2^20 (four-step under pre / mul / post with work2)
    "blu_unfused": [(n, (2,), False) for n in (8193, 16385, 40000, 100000, 200000, 300000)],
    # M = 2^21 ... 2^23 (gathered columns), 2^24 (three launches)
    "blu_unfused_large": [(n, (1,), False) for n in (600011, 1500000, 3000000, 5000000)],
    # the Bluestein loop's second chunk (chunk = 2^24 / M): fused, rx32k, four-step
    "blu_chunk_seams": [(4100, (1027,), True), (10007, (515,), True), (40000, (131,), True)],
    # one case per power-of-two family (test_gpu_parity.py goes deeper on these; here so that no label is left without a case)
    "pow2": ([(1, (5,), True)] + [(1 << k, (2 * (F32_TILE_POINTS >> k) + 3,), True) for k in range(1, 15)] +
             [(1 << 15, (3,), True)] + [(1 << k, (2,), True) for k in range(16, 21)] + [(1 << k, (1,), True) for k in range(21, 25)]),
}
F32_CASES = [case for group in F32_GROUPS.values() for case in group]
F32_REFUSED = F32_BLU_MAX_N + 1


def f64_lds_group(n):
    """Transforms per workgroup of the one-pass form (`p.B = F64_LDS_POINTS / p.N < 16 ? F64_LDS_POINTS / p.N : 16`)."""
    return min(F64_LDS_POINTS // n, 16)


F64_GROUPS = {
    # one pass through LDS at every size: two full workgroups and a ragged one
    "one_pass": [(1 << k, (2 * f64_lds_group(1 << k) + 1,), False) for k in range(1, 13)],
    # four-step at every size (2^24 is test_gpu_f64_fft.py's): the splits logN1 = (logP + 1) / 2 and h = logP / 2 of each
    "four_step": [(1 << k, (2 if k <= 20 else 1,), False) for k in range(13, 24)],
    # second pieces of the batch loops: four-step (64 per pass pair), one pass (2^20 per launch)
    "seams": [(1 << 13, (65, 129), True), (2, ((1 << 20) + 3,), True)],
    # ... and of the DFT sum (32768 per launch), which cannot run in place
    "seam_dft_sum": [(3, (F64_DFT_PIECE + 5,), False)],
    "dft_sum": [(n, (3,), False) for n in (3, 6, 10, 15, 63, 100, 255, 257, 1000, 4095)],
    "bluestein": [(n, (2,), False) for n in (4097, 8191, 8193, 16385, 300000, 600011)],
    "bluestein_large": [(n, (1,), False) for n in (1500000, 3000000, 5000000)],
    # P = 2^17, 2^18, 2^19: the padded lengths the lists above leave out
    "bluestein_other_p": [(n, (1,), False) for n in (40000, 100000, 200000)],
}
F64_CASES = [case for group in F64_GROUPS.values() for case in group]
F64_REFUSED = (1 << 23) + 1
# labels whose case lives in another module (256 MiB of input: not run twice)
F64_COVERED_ELSEWHERE = {"four_step_24": "test_gpu_f64_fft.py::test_fft_f64_2p24_and_round_trip"}

# Seam cases: (table, group) -> what "crosses" means for (n, batch)
SEAMS = {
    ("f32", "blu_chunk_seams"): lambda n, b: b * padded(n) > F32_BLU_CHUNK_POINTS,
    ("f32", "direct_grid_cap"): lambda n, b: b > F32_DIRECT_GROUP_CAP * direct_group(n),
    ("f32", "blu_fused_grid"): lambda n, b: b * padded(n) // F32_TILE_POINTS > F32_RX_GRID and b * padded(n) <= F32_BLU_CHUNK_POINTS,
    ("f64", "seams"): lambda n, b: b > (F64_FOUR_STEP_PIECE if n > F64_LDS_POINTS else F64_ONE_PASS_PIECE),
    ("f64", "seam_dft_sum"): lambda n, b: b > F64_DFT_PIECE,
}

# Fallback forms of the diagnostic build: selector -> (value, [(n, batch), ...])
FALLBACKS = {
    "COMMS_FFT_NO_RX": ("1", [(64, 3), (1024, 3), (4096, 3), (16384, 3), (1000, 3)]),  # the generic tile kernel; Bluestein unfused on it
    "COMMS_FFT_NO_RX32K": ("1", [(32768, 1), (32768, 3)]),                              # 32 x 1024 on the tile kernel + rows
    "COMMS_FFT_NO_COLS": ("1", [(1 << 16, 2), (1 << 19, 2)]),                           # column pass on the tile kernel
    "COMMS_FFT_BLU_UNFUSED": ("1", [(100, 3), (1000, 3), (5000, 3)]),                   # pre / mul / post around the single-pass kernel
    "COMMS_FFT_DIRECT_MAX": ("4096", [(100, 3), (1000, 3), (4095, 3)]),                 # dft_small_kernel at 65 ... 128, dft_direct_kernel above
}
