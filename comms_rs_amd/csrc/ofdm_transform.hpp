// ofdm_transform.hpp -- the wave-level N-point transform, N = 64 ... 1024, that ofdm.hip's kernels and spectrum.hip's share:
// the N = 16 L points of one symbol (segment) sit in L = N / 16 lanes, 16 per lane, so a wave holds 64 / L = 1024 / N of them.
// The steps are described at the head of ofdm.hip ("transform"); the butterflies are fft_radix.hpp's.
#pragma once

#include "fft_radix.hpp"

namespace comms {

constexpr int OF_WAVE_BUF = 1024 + 64;   // a wave's exchange buffer: 1024 / N symbols of N + N / 16 elements

__device__ __forceinline__ void of_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int of_pad(int i) { return i + (i >> 4); }

// R-point DFT of x[0 .. R), natural order in and out
template <int R, int DIR>
__device__ __forceinline__ void of_dft(cf* x) {
    if constexpr (R == 2) radix2<DIR>(x[0], x[1]);
    if constexpr (R == 4) radix4<DIR>(x[0], x[1], x[2], x[3]);
    if constexpr (R == 8) radix8<DIR>(*reinterpret_cast<cf(*)[8]>(x));
    if constexpr (R == 16) {
        radix16<DIR>(*reinterpret_cast<cf(*)[16]>(x));
        cf t[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) t[k] = x[R16_POS(k)];
#pragma unroll
        for (int k = 0; k < 16; ++k) x[k] = t[k];
    }
}

template <int N>
struct OfGeom {
    static constexpr int L = N / 16;                              // lanes per symbol
    static constexpr int SPW = 64 / L;                            // symbols per wave
    static constexpr int NP = N + N / 16;                         // a symbol's padded buffer
    static constexpr int R2 = N == 64 ? 4 : N == 128 ? 8 : 16;
    static constexpr int R3 = L / R2;                             // 1, 1, 1, 2, 4 (= M2)
    static constexpr int LAST = R3 > 1 ? R3 : R2;                 // radix of the step that ends in registers
    // the bin of result i of lane-in-symbol l: i = u LAST + j, butterfly l + L u, output j
    __device__ static __forceinline__ int bin(int l, int i) { return l + L * (i / LAST) + (R3 > 1 ? 256 : 16) * (i % LAST); }
};

// The N-point transform of the wave's 64 / L symbols: v[a] = x[l + L a] in, r[i] = X[bin(l, i)] out.  `buf` is the symbol's
// part of the wave's buffer.  Ends behind a wave barrier: the buffer is free again.
template <int N, int DIR>
__device__ __forceinline__ void of_transform(cf (&v)[16], cf* buf, const cf* tw, int l) {
    using G = OfGeom<N>;
    constexpr int L = G::L, R2 = G::R2, R3 = G::R3;
    radix16<DIR>(v);
#pragma unroll
    for (int k1 = 0; k1 < 16; ++k1) {
        cf y = v[R16_POS(k1)];
        if (k1) y = tw_mul<DIR>(y, tw[l * k1]);
        buf[of_pad(k1 * L + l)] = y;
    }
    of_wave_sync();
#pragma unroll
    for (int u = 0; u < 16 / R2; ++u) {
        const int t = l + L * u, lp = t % R3, k1 = t / R3;
#pragma unroll
        for (int b = 0; b < R2; ++b) v[u * R2 + b] = buf[of_pad(k1 * L + lp + R3 * b)];
        of_dft<R2, DIR>(&v[u * R2]);
    }
    of_wave_sync();
    if constexpr (R3 > 1) {   // (16 / R2 = 1: one butterfly per lane, t = l)
        const int lp = l % R3, k1 = l / R3;
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2) {
            cf y = v[k2];
            if (k2) y = tw_mul<DIR>(y, tw[16 * lp * k2]);
            buf[of_pad(lp * 256 + k1 + 16 * k2)] = y;
        }
        of_wave_sync();
#pragma unroll
        for (int u = 0; u < 16 / R3; ++u) {
#pragma unroll
            for (int j = 0; j < R3; ++j) v[u * R3 + j] = buf[of_pad(j * 256 + l + L * u)];
            of_dft<R3, DIR>(&v[u * R3]);
        }
        of_wave_sync();
    }
}

}  // namespace comms
