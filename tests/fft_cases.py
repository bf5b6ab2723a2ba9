"""Which kernels an FFT length runs on, restated from the dispatch code, and the case tables of tests/test_gpu_fft_lengths.py
drawn from that rule (no GPU here; tests/test_fft_cases.py holds the tables to the rule).

`family_f32(n)` restates fft_form / pow2_form (csrc/fft_plan.hpp, the rule csrc/fft.hip builds its plans from): the CPU test
runs that rule itself (tests/fft_plan_test.cpp) at every length up to 70000 and at every power of two +- 1 and compares the
labels, and the header's batching constants with the F32_* values below.  `family_f64(n)` restates fft_f64_prepare / pow2_run /
comms_fft_f64_run_dev (csrc/fft_f64.hip): every threshold of it is listed in ANCHORS with the source text it restates, and the
CPU test looks each text up in the source.  Either way a threshold that moves in the code fails there rather than leaving a
table that no longer crosses its seam.

A case is (n, batches, in_place): transform length, the batch counts to run it at, and whether the in-place run is checked
too (bitwise against the out-of-place one)."""

# ---------------------------------------------------------------- thresholds (f32: fft_plan.hpp's constants; f64: see ANCHORS)
NUM_CU = 256                 # common.hpp: kNumCU
F32_DIRECT_MAX = 64          # FftKnobs::direct_max: default of COMMS_FFT_DIRECT_MAX
F32_DIRECT_MAX_CAP = 4096    # kDirectMaxCap: the longest direct DFT whatever the selector says
F32_SMALL_DFT_MAX = 128      # kSmallDftMax: dft_small_kernel up to here, dft_direct_kernel above
F32_SMALL_DFT_LANES = 256    # kSmallDftLanes: dft_small_kernel runs G = 256 / N transforms per workgroup
F32_BLU_MAX_N = 1 << 23      # kBluMaxN: Bluestein refuses longer transforms
F32_BLU_CHUNK_POINTS = 1 << 24   # kBluChunkPoints: chunk = 2^24 / M padded transforms per pass of the Bluestein loop
F32_TILE_POINTS = 16384      # kRxTilePoints: points per tile of fft_rx1024_kernel
F32_RX_GRID = NUM_CU         # launch_rx: full tiles run on at most kNumCU workgroups (persistent_grid)
F32_DIRECT_GROUP_CAP = 8 * NUM_CU  # small_dft_grid_cap(kNumCU): dft_small_kernel's grid, in groups of G transforms
F64_LDS_POINTS = 4096        # fft_f64.hip: one pass through LDS up to here; the DFT sum up to here
F64_MAX_P = 1 << 24          # fft_f64_prepare: the largest power-of-two transform
F64_FOUR_STEP_PIECE = 64     # pow2_run: transforms per column + row pass pair
F64_ONE_PASS_PIECE = 1 << 20  # pow2_run: transforms per launch of the one-pass form
F64_DFT_PIECE = 32768        # comms_fft_f64_run_dev: transforms per launch of the DFT sum

FFT_F64_HIP = "comms_rs_amd/csrc/fft_f64.hip"
COMMON_HPP = "comms_rs_amd/csrc/common.hpp"

# (file, function the text stands in, text) -- the source lines the f64 rule and NUM_CU restate
ANCHORS = [
    (COMMON_HPP, "kNumCU", "constexpr int kNumCU = 256;"),
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
    """Bluestein's power-of-two length (fft_form: `while (c.M < 2 * N - 1) c.M <<= 1`; fft_f64_prepare: the same for P)."""
    m = 1
    while m < 2 * n - 1:
        m <<= 1
    return m


def _pow2_form_f32(length):
    """The form a power-of-two transform of `length` points runs on, with or without Bluestein around it."""
    log = ilog2(length)
    if length <= 32:          # Pow2Form::Tiny, Pow2Choice::rad = -N: the in-register forms of fft_rx1024_kernel
        return "tiny"
    if length <= 16384:       # Pow2Form::Rx
        return "rx%d" % length  # (one instantiation of fft_rx1024_kernel per length: Pow2Choice::rad 0, 128, 256, 512, 1, 2, 4, 8, 16)
    if length == 32768:       # Pow2Form::Rx32k
        return "rx32k"
    if log <= 19:             # Pow2Form::Cols, Pow2Choice::kind by the column length 64 ... 512: fft_cols_kernel + 1024-point rows
        return "cols_2p%d" % log
    if log == 20:             # Pow2Form::Fast20: N1 = N2 = 1024, both passes on fft1024x16_kernel, no column kernel
        return "fast_2p20"
    if log <= 23:             # Pow2Form::Gather up to FftKnobs::large_gather (23): gathered columns + rows
        return "gather_2p%d" % log
    if log == 24:             # Pow2Form::Three: columns, rows in place, transpose
        return "three_2p24"
    raise ValueError("power-of-two FFT supports up to 2^24 points")  # fft_form: kPow2MaxLog


def family_f32(n):
    """Label of the kernels FFTBatchNode(n) runs; ValueError where comms_fft_create refuses."""
    if n < 1:                 # comms_fft_create: COMMS_ARG(fft_size >= 1, ...)
        raise ValueError("fft_size must be >= 1")
    if is_pow2(n):            # fft_form: FftKind::Pow2
        if n == 1:            # FftKind::Copy
            return "pow2_copy"
        return "pow2_" + _pow2_form_f32(n)
    if n <= F32_DIRECT_MAX:   # fft_form: `N <= k.direct_max && N <= kDirectMaxCap` -> FftKind::DirectSmall (N <= 128): dft_small_kernel
        return "direct"
    if n > F32_BLU_MAX_N:     # fft_form: `N > kBluMaxN`: "FFT length %zu too large"
        raise ValueError("FFT length too large")
    m = padded(n)
    form = _pow2_form_f32(m)  # fft_setup: pow2_plan_build(h->plan, M, pow2_form(M, ...))
    if form.startswith("rx") and form != "rx32k":  # FftKind::BluFused (the plan's form is Rx): two launches of fft_rx1024_kernel, modes 1 and 2
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
    return F32_SMALL_DFT_LANES // n


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
