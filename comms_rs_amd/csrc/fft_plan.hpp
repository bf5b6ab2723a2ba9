// fft_plan.hpp -- which kernels an FFT length runs on (Complex<f32>, fft.hip): the whole rule, as two pure functions.
// Host code without HIP headers: fft.hip builds its plans from it, tests/fft_plan_test.cpp runs it at every length.
#pragma once

#include <cstddef>
#include <cstdio>

namespace comms {

// The forms of a power-of-two transform, one per launch sequence of pow2_run (fft.hip).
enum class Pow2Form {
    Tiny,    // N = 2 ... 32: fft_rx1024_kernel, sixteen consecutive points per lane
    Rx,      // 64 ... 16384: fft_rx1024_kernel, one pass
    Rx32k,   // 32768: fft_rx32k_kernel, one pass
    Cols,    // 2^16 ... 2^19: fft_cols_kernel on the N / 1024-point columns, fft1024x16_kernel on the rows
    Fast20,  // 2^20: both passes on fft1024x16_kernel
    Gather,  // 2^21 ... 2^23: N / 1024-point columns gathered by fft_rx1024_kernel, fft1024x16_kernel on the rows
    Three,   // 2^24: 1024-point columns, N / 1024-point rows in place, transpose
    Tile,    // fft_tile_kernel: what a selector falls back to.  One pass up to 4096 points (1024: fft1024x16_kernel in
             // its 8-wave form), two above; from 32768 points on the second pass has 1024-point rows and keeps
             // fft1024x16_kernel
};

// The diagnostic build's selectors (COMMS_FFT_*; the product build has these defaults at compile time)
struct FftKnobs {
    bool no_rx = false;           // NO_RX: 2 ... 16384 points off fft_rx1024_kernel
    bool no_rx32k = false;        // NO_RX32K
    bool no_cols = false;         // NO_COLS
    int large_gather = 23;        // LARGE_GATHER: the largest log2 N on the Gather form
    size_t direct_max = 64;       // DIRECT_MAX: the longest transform on the O(N^2) sum
    bool blu_unfused = false;     // BLU_UNFUSED: pre / mul / post kernels around the single-pass kernel
};

constexpr size_t kRxTilePoints = 16384;                          // points per tile of fft_rx1024_kernel
constexpr size_t kTileOnePassMax = 4096;                         // fft_tile_kernel: one pass up to here
constexpr int kPow2MaxLog = 24;                                  // the longest power-of-two transform
constexpr size_t kBluMaxN = static_cast<size_t>(1) << 23;        // Bluestein: the longest transform (M = 2^24)
constexpr size_t kBluChunkPoints = static_cast<size_t>(1) << 24; // ... runs 2^24 / M padded transforms per trip
constexpr size_t kDirectMaxDefault = 64, kDirectMaxCap = 4096;   // the O(N^2) sum: measured crossover; LDS limit
constexpr size_t kSmallDftMax = 128;                             // dft_small_kernel up to here, dft_direct_kernel above
constexpr size_t kSmallDftLanes = 256;                           // ... 256 / N transforms per workgroup
constexpr size_t small_dft_grid_cap(size_t num_cu) { return 8 * num_cu; }

inline int ilog2(size_t v) {
    int l = 0;
    while ((static_cast<size_t>(1) << l) < v) ++l;
    return l;
}

struct Pow2Choice {
    Pow2Form form;
    int rad;       // Tiny, Rx: RAD of fft_rx1024_kernel (-N; 0, 128, 256, 512 for N = 64 ... 512; N / 1024 from 1024 on).
                   // Gather: RAD of the column pass, (N / 1024) / 1024
    int kind;      // Cols: KIND of fft_cols_kernel (0 for 64-point columns, else their length: 128, 256, 512)
    bool scratch;  // two passes through a scratch buffer of the call's size
};

// N: a power of two, 2 ... 2^24
inline Pow2Choice pow2_form(size_t N, const FftKnobs& k) {
    const int log = ilog2(N);
    if (log <= 14) {
        if (k.no_rx) return {Pow2Form::Tile, 0, 0, N > kTileOnePassMax};
        if (N <= 32) return {Pow2Form::Tiny, -static_cast<int>(N), 0, false};
        return {Pow2Form::Rx, N == 64 ? 0 : N < 1024 ? static_cast<int>(N) : static_cast<int>(N / 1024), 0, false};
    }
    if (log == 15) return {k.no_rx32k ? Pow2Form::Tile : Pow2Form::Rx32k, 0, 0, k.no_rx32k};
    if (log <= 19) return {k.no_cols ? Pow2Form::Tile : Pow2Form::Cols, 0, log == 16 ? 0 : 1 << (log - 10), true};
    if (log == 20) return {Pow2Form::Fast20, 0, 0, true};
    if (log <= k.large_gather) return {Pow2Form::Gather, 1 << (log - 20), 0, true};
    return {Pow2Form::Three, 0, 0, true};
}

enum class FftKind { Copy, Pow2, DirectSmall, Direct, BluFused, BluUnfused, Refused };

struct FftChoice {
    FftKind kind;
    size_t M;       // Pow2: N; Bluestein: the padded length (the power-of-two plan's); else 0
    char why[80];   // Refused: the message
};

// N >= 1
inline FftChoice fft_form(size_t N, const FftKnobs& k) {
    FftChoice c{FftKind::Refused, 0, {0}};
    if ((N & (N - 1)) == 0) {
        if (ilog2(N) > kPow2MaxLog) {
            snprintf(c.why, sizeof(c.why), "power-of-two FFT supports up to 2^24 points (got 2^%d)", ilog2(N));
            return c;
        }
        c.kind = N == 1 ? FftKind::Copy : FftKind::Pow2;
        c.M = N == 1 ? 0 : N;
        return c;
    }
    // short odd lengths: the exact-index O(N^2) DFT (f64 accumulation); above that Bluestein on the
    // power-of-two kernels is faster by far (N = 1000: 2.3 -> 20 Gpoints/s) -- measured crossover ~64
    if (N <= k.direct_max && N <= kDirectMaxCap) {
        c.kind = N <= kSmallDftMax ? FftKind::DirectSmall : FftKind::Direct;
        return c;
    }
    if (N > kBluMaxN) {
        snprintf(c.why, sizeof(c.why), "FFT length %zu too large", N);
        return c;
    }
    c.M = 1;
    while (c.M < 2 * N - 1) c.M <<= 1;
    // a padded length on the single-pass kernel takes the chirp products into its loads and stores: two launches
    const Pow2Form f = pow2_form(c.M, k).form;
    c.kind = (f == Pow2Form::Tiny || f == Pow2Form::Rx) && !k.blu_unfused ? FftKind::BluFused : FftKind::BluUnfused;
    return c;
}

}  // namespace comms
