// ofdm.hip -- the OFDM stages between SymbolMapNode and DemapNode: records of data-carrier values -> frames of time samples
// (ofdm_mod_kernel: carrier map, pilots, training symbols, IFFT, cyclic prefix) and frames of received samples -> records of
// equalised data-carrier values (ofdm_demod_kernel: prefix removal, FFT, least-squares channel estimate from the training
// symbols, one-tap equaliser, pilot phase correction, carrier extraction), every frame of a call by ONE launch each.  One
// handle serves both directions; both are stateless.
//
// The reference has no such block; the contract is include/comms_hip.h's ("OFDM modulator and demodulator"), and
// tests/ofdm_ref.py restates it in complex128.
//   transform     N = 16 L points of one symbol sit in L = N / 16 lanes, 16 per lane, so a wave holds 64 / L = 1024 / N
//                 symbols (16 at N = 64, one at N = 1024) and no lane idles on a full group.  With n = l + L a, k = k1 + 16 k':
//                   step 1  lane l loads x[l + L a] (consecutive lanes, consecutive samples), radix-16 over a, times
//                           W_N^{l k1}, into the wave's LDS buffer at [k1 L + l];
//                   step 2  the L-point transforms over l, l = l' + M2 b: radix R2 = 4, 8, 16, 16, 16 over b for N = 64 ...
//                           1024, 16 / R2 butterflies per lane.  N <= 256: done, X[k1 + 16 k2] is in registers.
//                   step 3  N = 512, 1024: times W_L^{l' k2}, into LDS at [l' 256 + k1 + 16 k2], radix M2 = 2, 4 over l':
//                           X[k1 + 16 k2 + 256 k3].
//                 One LDS exchange per radix step, wave-private, no workgroup barrier; the buffer index i sits at i + i / 16
//                 (fft.hip's padding).  Twiddles are W_N^j, j < N, built on the host in f64 and rounded once, read from LDS.
//   load / store  prefix removal, the carrier scatter (bin -> record index, a host-built table), pilots and training values
//                 are the modulator's load stage; scaling and the prefix copy its store stage.  The demodulator loads past
//                 the prefix and its store stage multiplies by 1 / H_k, corrects the pilots' common phase and writes the
//                 data bins only.  All global accesses are 8 bytes wide: a symbol behind an odd prefix is 8, not 16, bytes
//                 off alignment.
//   work split    a workgroup of four waves takes an item (frame, block of symbols); its waves walk the block's groups of
//                 1024 / N symbols.  The demodulator first transforms the frame's T training symbols (all four waves), sums
//                 them in symbol order and leaves T train[k] / sum_t Y_{t,k} = 1 / H_k in LDS.  ofdm_block() chooses the
//                 block: one per frame when the call has at least as many frames as the grid has workgroups, otherwise
//                 just enough blocks per frame to give every workgroup an item.
//   channel state ofdm_demod_kernel<N, true> (comms_ofdm_demod_csi_run_dev) is the same launch with one store more behind the
//                 1 / H_k step: den = |sum_t Y_{t,k}|^2 is in a register there, and g = den / |T train[k]|^2 = |H_k|^2 goes to
//                 the frame's record of D floats, data carriers in bin order.  Every item of a frame forms 1 / H_k; the item
//                 whose block starts at symbol 0 writes the record.  The divisor is a host-built table (f64, rounded once).
// Both kernels walk their items grid-stride under the library's grid cap.
#include <cmath>

#include "common.hpp"
#include "fft_radix.hpp"
#include "ofdm_transform.hpp"

namespace comms {

constexpr int OF_WG = 256, OF_WAVES = OF_WG / 64;
constexpr size_t OF_MAX_FRAME = size_t(1) << 24;

constexpr size_t ofdm_lds(int n) { return static_cast<size_t>(n) * (2 * sizeof(float2) + sizeof(int)) + OF_WAVES * OF_WAVE_BUF * sizeof(float2); }

struct OfdmArgs {
    const float2* in;
    float2* out;
    const float2* tw;      // W_N^j = (cos, -sin)(2 pi j / N), j < N
    const int* map;        // bin -> d >= 0 (data value d of a symbol), -1 (null), -2 - q (pilot q)
    const float2* pilots;  // Q
    const float* pol;      // n_pol >= 1
    const float2* train;   // modulator: train[k]; demodulator: T train[k]
    const float* tt2;      // demodulator with channel state: |T train[k]|^2
    float* csi;            // ... and its records of D floats
    size_t items;          // n_frames * nblk
    unsigned n_pol, T, S, D, CP;
    unsigned blk, nblk;    // symbols per block, blocks per frame
    float scale;           // modulator: tx_scale; demodulator without training: 1 / (N tx_scale)
    int cpe;
};

// (frame, first symbol, end symbol) of an item; `per_frame` symbols are split into nblk blocks of blk
__device__ __forceinline__ void of_item(const OfdmArgs& a, size_t item, unsigned per_frame, size_t& frame, unsigned& s0, unsigned& s1) {
    frame = item / a.nblk;
    s0 = static_cast<unsigned>(item % a.nblk) * a.blk;
    s1 = s0 + a.blk < per_frame ? s0 + a.blk : per_frame;
}

__device__ __forceinline__ cf of_scale(cf y, float s) { return cf{__fmul_rn(y.x, s), __fmul_rn(y.y, s)}; }

template <int N>
__global__ __launch_bounds__(OF_WG) void ofdm_mod_kernel(const OfdmArgs a) {
    using G = OfGeom<N>;
    extern __shared__ __align__(16) unsigned char of_smem[];
    cf* tw = reinterpret_cast<cf*>(of_smem);
    int* map = reinterpret_cast<int*>(tw + 2 * N);
    cf* ex = reinterpret_cast<cf*>(map + N);
    for (int i = threadIdx.x; i < N; i += OF_WG) {
        tw[i] = to_cf(a.tw[i]);
        map[i] = a.map[i];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane / G::L, l = lane % G::L;
    cf* buf = ex + wave * OF_WAVE_BUF + q * G::NP;
    const unsigned per_frame = a.T + a.S, sym_len = N + a.CP;
    for (size_t item = blockIdx.x; item < a.items; item += gridDim.x) {
        size_t frame;
        unsigned s0, s1;
        of_item(a, item, per_frame, frame, s0, s1);
        // `g` is wave-uniform: every lane of a wave takes part in the exchanges
        for (unsigned g = s0 + wave * G::SPW; g < s1; g += OF_WAVES * G::SPW) {
            const unsigned s = g + q;
            const bool live = s < s1;
            cf v[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) v[i] = cf{0.f, 0.f};
            if (live) {
                if (s < a.T) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) v[i] = to_cf(a.train[l + G::L * i]);
                } else {
                    const unsigned sd = s - a.T;
                    const float2* rec = a.in + (frame * a.S + sd) * a.D;
                    const float p = a.pol[sd % a.n_pol];
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int code = map[l + G::L * i];
                        if (code >= 0)
                            v[i] = to_cf(rec[code]);
                        else if (code < -1)
                            v[i] = of_scale(to_cf(a.pilots[-2 - code]), p);
                    }
                }
            }
            of_transform<N, +1>(v, buf, tw, l);
            if (live) {
                float2* sym = a.out + (frame * per_frame + s) * sym_len;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const unsigned n = static_cast<unsigned>(G::bin(l, i));
                    const float2 y = to_f2(of_scale(v[i], a.scale));
                    sym[a.CP + n] = y;
                    if (n + a.CP >= N) sym[n + a.CP - N] = y;
                }
            }
        }
    }
}

template <int N, bool CSI = false>
__global__ __launch_bounds__(OF_WG) void ofdm_demod_kernel(const OfdmArgs a) {
    using G = OfGeom<N>;
    extern __shared__ __align__(16) unsigned char of_smem[];
    cf* tw = reinterpret_cast<cf*>(of_smem);
    cf* inv = tw + N;   // the training symbols' sum, then 1 / H_k (0 on a null bin)
    int* map = reinterpret_cast<int*>(inv + N);
    cf* ex = reinterpret_cast<cf*>(map + N);
    for (int i = threadIdx.x; i < N; i += OF_WG) {
        tw[i] = to_cf(a.tw[i]);
        map[i] = a.map[i];
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane / G::L, l = lane % G::L;
    cf* buf = ex + wave * OF_WAVE_BUF + q * G::NP;
    const unsigned per_frame = a.T + a.S, sym_len = N + a.CP;
    constexpr unsigned ROUND = OF_WAVES * G::SPW;   // symbols the workgroup transforms at once
    for (size_t item = blockIdx.x; item < a.items; item += gridDim.x) {
        size_t frame;
        unsigned s0, s1;
        of_item(a, item, a.S, frame, s0, s1);
        const float2* in = a.in + frame * per_frame * sym_len;
        __syncthreads();   // the tables are in place; the previous item is done with inv
        for (int k = threadIdx.x; k < N; k += OF_WG) inv[k] = a.T ? cf{0.f, 0.f} : cf{map[k] == -1 ? 0.f : a.scale, 0.f};
        for (unsigned t0 = 0; t0 < a.T; t0 += ROUND) {   // (workgroup-uniform)
            const unsigned t = t0 + wave * G::SPW + q;
            cf v[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) v[i] = t < a.T ? to_cf(in[t * sym_len + a.CP + l + G::L * i]) : cf{0.f, 0.f};
            of_transform<N, -1>(v, buf, tw, l);
#pragma unroll
            for (int i = 0; i < 16; ++i) buf[of_pad(G::bin(l, i))] = v[i];
            __syncthreads();
            const unsigned left = a.T - t0, slots = left < ROUND ? left : ROUND;
            for (int k = threadIdx.x; k < N; k += OF_WG) {
                cf acc = inv[k];
                for (unsigned sl = 0; sl < slots; ++sl)   // in symbol order
                    acc = cadd(acc, ex[(sl / G::SPW) * OF_WAVE_BUF + (sl % G::SPW) * G::NP + of_pad(k)]);
                inv[k] = acc;
            }
            __syncthreads();
        }
        if (a.T) {
            for (int k = threadIdx.x; k < N; k += OF_WG) {
                const cf h = inv[k];
                const float den = __fmaf_rn(h.x, h.x, __fmul_rn(h.y, h.y));
                const cf num = cmulcf(to_cf(a.train[k]), h);   // T train[k] conj(sum)
                inv[k] = map[k] == -1 ? cf{0.f, 0.f} : cf{__fdiv_rn(num.x, den), __fdiv_rn(num.y, den)};
                if constexpr (CSI) {
                    if (s0 == 0 && map[k] >= 0) a.csi[frame * a.D + map[k]] = __fdiv_rn(den, a.tt2[k]);   // (D > map[k])
                }
            }
        }
        __syncthreads();
        for (unsigned g = s0 + wave * G::SPW; g < s1; g += ROUND) {   // (wave-uniform)
            const unsigned s = g + q;
            const bool live = s < s1;
            cf v[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) v[i] = live ? to_cf(in[(a.T + s) * sym_len + a.CP + l + G::L * i]) : cf{0.f, 0.f};
            of_transform<N, -1>(v, buf, tw, l);
#pragma unroll
            for (int i = 0; i < 16; ++i) v[i] = cmulf(v[i], inv[G::bin(l, i)]);
            if (a.cpe) {
                cf c = cf{0.f, 0.f};
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int code = map[G::bin(l, i)];
                    if (code < -1) c = cadd(c, cmulcf(v[i], to_cf(a.pilots[-2 - code])));
                }
#pragma unroll
                for (int off = 1; off < G::L; off <<= 1) c = cadd(c, cf{__shfl_xor(c.x, off), __shfl_xor(c.y, off)});
                c = of_scale(c, a.pol[s % a.n_pol]);
                const float mag = __fsqrt_rn(__fmaf_rn(c.x, c.x, __fmul_rn(c.y, c.y)));
                if (mag > 0.f && mag <= 3.402823466e38f) {
                    const cf r = cf{__fdiv_rn(c.x, mag), __fdiv_rn(c.y, mag)};
#pragma unroll
                    for (int i = 0; i < 16; ++i) v[i] = cmulcf(v[i], r);
                }
            }
            if (live) {
                float2* rec = a.out + (frame * a.S + s) * a.D;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int code = map[G::bin(l, i)];
                    if (code >= 0) rec[code] = to_f2(v[i]);
                }
            }
        }
    }
}

}  // namespace comms

using namespace comms;

struct comms_ofdm : Handle {
    unsigned N = 0, CP = 0, D = 0, Q = 0, T = 0, S = 0, n_pol = 1;
    int flags = 0;
    float tx_scale = 0.f;
    DevBuf<float2> tw, pilots, train, train_t;   // train_t: T train[k]
    DevBuf<float> pol, tt2;                      // tt2: |train_t[k]|^2
    DevBuf<int> map;
    unsigned max_grid = 1;
};
static_assert(!std::is_copy_constructible_v<comms_ofdm>, "a handle is never copied");

namespace {

size_t of_data_syms(const comms_ofdm* h) { return static_cast<size_t>(h->S) * h->D; }
size_t of_frame_samples(const comms_ofdm* h) { return static_cast<size_t>(h->T + h->S) * (h->N + h->CP); }

// The block rule.  `per_frame` symbols (T + S for the modulator, S for the demodulator) in rounds of 4 waves x 1024 / N: a call
// with at least max_grid frames takes one block per frame (the demodulator then estimates every frame's channel once); a
// call with fewer takes ceil(max_grid / n_frames) blocks per frame, if the frame has that many rounds, of whole rounds each.
void ofdm_block(const comms_ofdm* h, size_t n_frames, unsigned per_frame, unsigned* blk, unsigned* nblk) {
    const unsigned round = OF_WAVES * 1024u / h->N, rounds = (per_frame + round - 1) / round;
    size_t want = n_frames && n_frames < h->max_grid ? (h->max_grid + n_frames - 1) / n_frames : 1;
    if (want > rounds) want = rounds;
    *blk = static_cast<unsigned>((rounds + want - 1) / want) * round;
    *nblk = (per_frame + *blk - 1) / *blk;
}
size_t of_grid(const comms_ofdm* h, size_t items) { return capped_grid(items, h->max_grid); }
// data-carrier records in and frames of samples out (the modulator), or the other way round
FrameCall of_call(const comms_ofdm* h, int direction) {
    const size_t data = of_data_syms(h) * sizeof(comms_c32), frame = of_frame_samples(h) * sizeof(comms_c32);
    const bool mod = direction == COMMS_OFDM_MOD;
    return {mod ? data : frame, mod ? frame : data, 8, 8, (size_t(1) << 40) / of_frame_samples(h)};
}

template <int N>
comms_status_t of_launch_n(comms_ofdm* h, int direction, const OfdmArgs& a, dim3 grid, hipStream_t s) {
    if (direction == COMMS_OFDM_MOD)
        return launch_kernel<ofdm_mod_kernel<N>>("ofdm_mod_kernel", grid, dim3(OF_WG), ofdm_lds(N), s, h->take_events(), a);
    if (a.csi) return launch_kernel<ofdm_demod_kernel<N, true>>("ofdm_demod_kernel", grid, dim3(OF_WG), ofdm_lds(N), s, h->take_events(), a);
    return launch_kernel<ofdm_demod_kernel<N>>("ofdm_demod_kernel", grid, dim3(OF_WG), ofdm_lds(N), s, h->take_events(), a);
}

// `with_csi`: the demodulator's channel-state form, d_csi its n_frames records of D floats
comms_status_t of_run_dev(comms_ofdm* h, int direction, const comms_c32* d_in, size_t n_frames, comms_c32* d_out, void* stream,
                          bool with_csi = false, float* d_csi = nullptr) {
    COMMS_TRY(check_frame_call(h, [&](const comms_ofdm* o) { return of_call(o, direction); }, d_in, n_frames, d_out, true));
    if (with_csi) {
        COMMS_ARG(h->T >= 1, "the channel state comes from the training symbols: the handle has none");
        COMMS_ARG(!n_frames || d_csi, "NULL pointer");
        COMMS_ARG(aligned(d_csi, 4), "the channel-state records must be aligned to 4 bytes");
        const size_t csi_bytes = n_frames * h->D * sizeof(float);
        COMMS_ARG(!n_frames || (!ranges_overlap(d_csi, csi_bytes, d_in, n_frames * of_call(h, direction).in_bytes) &&
                                !ranges_overlap(d_csi, csi_bytes, d_out, n_frames * of_call(h, direction).out_bytes)),
                  "the channel-state records overlap the input or the output records");
    }
    if (!n_frames) return COMMS_OK;
    COMMS_TRY(use_device(h->device));
    const bool mod = direction == COMMS_OFDM_MOD;
    OfdmArgs a{};
    a.in = reinterpret_cast<const float2*>(d_in);
    a.out = reinterpret_cast<float2*>(d_out);
    a.tw = h->tw.get();
    a.map = h->map.get();
    a.pilots = h->pilots.get();
    a.pol = h->pol.get();
    a.train = mod ? h->train.get() : h->train_t.get();
    a.tt2 = h->tt2.get();
    a.csi = with_csi ? d_csi : nullptr;
    a.n_pol = h->n_pol;
    a.T = h->T;
    a.S = h->S;
    a.D = h->D;
    a.CP = h->CP;
    ofdm_block(h, n_frames, mod ? h->T + h->S : h->S, &a.blk, &a.nblk);
    a.items = n_frames * a.nblk;
    a.scale = mod ? h->tx_scale : static_cast<float>(1.0 / (static_cast<double>(h->N) * static_cast<double>(h->tx_scale)));
    a.cpe = (h->flags & COMMS_OFDM_CPE) != 0;
    const dim3 grid(static_cast<unsigned>(of_grid(h, a.items)));
    hipStream_t s = h->pick(stream);
    switch (h->N) {
        case 64: return of_launch_n<64>(h, direction, a, grid, s);
        case 128: return of_launch_n<128>(h, direction, a, grid, s);
        case 256: return of_launch_n<256>(h, direction, a, grid, s);
        case 512: return of_launch_n<512>(h, direction, a, grid, s);
        default: return of_launch_n<1024>(h, direction, a, grid, s);
    }
}

comms_status_t of_run(comms_ofdm* h, int direction, const comms_c32* in, size_t n_frames, comms_c32* out) {
    return run_frame_call(h, [&](const comms_ofdm* o) { return of_call(o, direction); }, in, n_frames, out, [&](void* d_in, void* d_out) {
        return of_run_dev(h, direction, static_cast<const comms_c32*>(d_in), n_frames, static_cast<comms_c32*>(d_out), COMMS_STREAM_HANDLE);
    });
}

}  // namespace

extern "C" {

comms_status_t comms_ofdm_create(int32_t n_fft, int32_t n_cp, const uint8_t* carrier_kind, const comms_c32* pilots, const float* polarity,
                                 size_t n_pol, const comms_c32* train, size_t n_train, size_t n_syms, int32_t flags, int32_t device,
                                 comms_ofdm_t** out) {
    COMMS_ARG(out != nullptr, "out is NULL");
    *out = nullptr;
    COMMS_ARG(n_fft == 64 || n_fft == 128 || n_fft == 256 || n_fft == 512 || n_fft == 1024, "n_fft must be 64, 128, 256, 512 or 1024 (got %d)",
              n_fft);
    COMMS_ARG(n_cp >= 0 && n_cp <= n_fft, "the prefix has 0 ... n_fft samples (got %d)", n_cp);
    COMMS_ARG(carrier_kind != nullptr, "carrier_kind is NULL");
    COMMS_ARG((flags & ~COMMS_OFDM_CPE) == 0, "flags must be 0 or COMMS_OFDM_CPE (got %d)", flags);
    const size_t N = static_cast<size_t>(n_fft);
    std::vector<int> map(N);
    unsigned D = 0, Q = 0;
    for (size_t k = 0; k < N; ++k) {
        COMMS_ARG(carrier_kind[k] <= COMMS_OFDM_PILOT, "carrier_kind[%zu] must be 0 (null), 1 (data) or 2 (pilot)", k);
        map[k] = carrier_kind[k] == COMMS_OFDM_DATA ? static_cast<int>(D++) : carrier_kind[k] == COMMS_OFDM_PILOT ? -2 - static_cast<int>(Q++) : -1;
    }
    COMMS_ARG(D >= 1, "the carrier map has no data carrier");
    COMMS_ARG(pilots || !Q, "pilots is NULL with %u pilot carriers", Q);
    COMMS_ARG(Q || !(flags & COMMS_OFDM_CPE), "COMMS_OFDM_CPE needs a pilot carrier");
    for (unsigned p = 0; p < Q; ++p) COMMS_ARG(std::isfinite(pilots[p].re) && std::isfinite(pilots[p].im), "pilot %u is not finite", p);
    COMMS_ARG(!polarity || (n_pol >= 1 && n_pol <= (size_t(1) << 20)), "polarity holds 1 ... 2^20 values (got %zu)", n_pol);
    std::vector<float> pol(1, 1.0f);
    if (polarity) {
        pol.assign(polarity, polarity + n_pol);
        for (size_t i = 0; i < n_pol; ++i) COMMS_ARG(std::isfinite(pol[i]), "polarity[%zu] is not finite", i);
    }
    COMMS_ARG(n_syms >= 1 && n_syms <= OF_MAX_FRAME && n_train <= OF_MAX_FRAME && (n_train + n_syms) * (N + static_cast<size_t>(n_cp)) <= OF_MAX_FRAME,
              "a frame has n_syms >= 1 and at most 2^24 samples (got n_train %zu, n_syms %zu)", n_train, n_syms);
    COMMS_ARG(train || !n_train, "train is NULL with n_train > 0");
    std::vector<float2> tr(N, make_float2(0.f, 0.f)), tr_t(N, make_float2(0.f, 0.f));
    std::vector<float> tt2(N, 0.f);
    if (n_train) {
        for (size_t k = 0; k < N; ++k) {
            COMMS_ARG(std::isfinite(train[k].re) && std::isfinite(train[k].im), "train[%zu] is not finite", k);
            COMMS_ARG(map[k] == -1 || train[k].re != 0.f || train[k].im != 0.f, "train[%zu] is zero on a data or pilot carrier", k);
            tr[k] = make_float2(train[k].re, train[k].im);
            tr_t[k] = make_float2(static_cast<float>(static_cast<double>(n_train) * train[k].re),
                                  static_cast<float>(static_cast<double>(n_train) * train[k].im));
            const double re = tr_t[k].x, im = tr_t[k].y;   // from the stored, rounded values: what the kernel multiplies by
            tt2[k] = static_cast<float>(re * re + im * im);
        }
    }
    std::vector<float2> tw(N);
    for (size_t j = 0; j < N; ++j) {
        const double t = 2.0 * 3.14159265358979323846 * static_cast<double>(j) / static_cast<double>(N);
        tw[j] = make_float2(static_cast<float>(std::cos(t)), static_cast<float>(-std::sin(t)));
    }
    HandlePtr<comms_ofdm> h;
    COMMS_TRY(make_handle(device, &h));
    h->N = static_cast<unsigned>(n_fft);
    h->CP = static_cast<unsigned>(n_cp);
    h->D = D;
    h->Q = Q;
    h->T = static_cast<unsigned>(n_train);
    h->S = static_cast<unsigned>(n_syms);
    h->n_pol = static_cast<unsigned>(pol.size());
    h->flags = flags;
    h->tx_scale = static_cast<float>(1.0 / std::sqrt(static_cast<double>(N)));
    COMMS_HIP_TRY(h->tw.upload(tw));
    COMMS_HIP_TRY(h->map.upload(map));
    COMMS_HIP_TRY(h->pol.upload(pol));
    COMMS_HIP_TRY(h->train.upload(tr));
    COMMS_HIP_TRY(h->train_t.upload(tr_t));
    COMMS_HIP_TRY(h->tt2.upload(tt2));
    if (Q) COMMS_HIP_TRY(h->pilots.upload(reinterpret_cast<const float2*>(pilots), Q));
    h->max_grid = resident_workgroups(ofdm_lds(n_fft));
    *out = h.release();
    return COMMS_OK;
}

comms_status_t comms_ofdm_set_scale(comms_ofdm_t* h, float tx_scale) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG(std::isfinite(tx_scale) && tx_scale > 0.f, "tx_scale must be finite and positive");
    h->tx_scale = tx_scale;
    return COMMS_OK;
}

size_t comms_ofdm_data_syms(const comms_ofdm_t* h) { return h ? of_data_syms(h) : 0; }
size_t comms_ofdm_frame_samples(const comms_ofdm_t* h) { return h ? of_frame_samples(h) : 0; }

comms_status_t comms_ofdm_mod_run_dev(comms_ofdm_t* h, const comms_c32* d_syms, size_t n_frames, comms_c32* d_out, void* stream) {
    return of_run_dev(h, COMMS_OFDM_MOD, d_syms, n_frames, d_out, stream);
}
comms_status_t comms_ofdm_mod_run(comms_ofdm_t* h, const comms_c32* syms, size_t n_frames, comms_c32* out) {
    return of_run(h, COMMS_OFDM_MOD, syms, n_frames, out);
}
comms_status_t comms_ofdm_demod_run_dev(comms_ofdm_t* h, const comms_c32* d_in, size_t n_frames, comms_c32* d_out, void* stream) {
    return of_run_dev(h, COMMS_OFDM_DEMOD, d_in, n_frames, d_out, stream);
}
comms_status_t comms_ofdm_demod_run(comms_ofdm_t* h, const comms_c32* in, size_t n_frames, comms_c32* out) {
    return of_run(h, COMMS_OFDM_DEMOD, in, n_frames, out);
}

comms_status_t comms_ofdm_demod_csi_run_dev(comms_ofdm_t* h, const comms_c32* d_in, size_t n_frames, comms_c32* d_out, float* d_csi,
                                           void* stream) {
    return of_run_dev(h, COMMS_OFDM_DEMOD, d_in, n_frames, d_out, stream, true, d_csi);
}
comms_status_t comms_ofdm_demod_csi_run(comms_ofdm_t* h, const comms_c32* in, size_t n_frames, comms_c32* out, float* csi) {
    COMMS_TRY(check_frame_call(h, [&](const comms_ofdm* o) { return of_call(o, COMMS_OFDM_DEMOD); }, in, n_frames, out, false));
    COMMS_ARG(h->T >= 1, "the channel state comes from the training symbols: the handle has none");
    COMMS_ARG(!n_frames || csi, "NULL pointer");
    if (!n_frames) return COMMS_OK;
    COMMS_TRY(use_device(h->device));
    // one device block for the outputs: the records, then the channel state
    const FrameCall c = of_call(h, COMMS_OFDM_DEMOD);
    const size_t in_b = n_frames * c.in_bytes, rec_b = n_frames * c.out_bytes, csi_b = n_frames * h->D * sizeof(float);
    COMMS_TRY(h->in_scratch.reserve(in_b));
    COMMS_TRY(h->out_scratch.reserve(rec_b + csi_b));
    char* d_out = static_cast<char*>(h->out_scratch.p);
    COMMS_HIP_TRY(hipMemcpyAsync(h->in_scratch.p, in, in_b, hipMemcpyHostToDevice, h->stream));
    COMMS_TRY(of_run_dev(h, COMMS_OFDM_DEMOD, static_cast<const comms_c32*>(h->in_scratch.p), n_frames, reinterpret_cast<comms_c32*>(d_out),
                         COMMS_STREAM_HANDLE, true, reinterpret_cast<float*>(d_out + rec_b)));
    COMMS_HIP_TRY(hipMemcpyAsync(out, d_out, rec_b, hipMemcpyDeviceToHost, h->stream));
    COMMS_HIP_TRY(hipMemcpyAsync(csi, d_out + rec_b, csi_b, hipMemcpyDeviceToHost, h->stream));
    COMMS_HIP_TRY(hipStreamSynchronize(h->stream));
    return COMMS_OK;
}

comms_status_t comms_ofdm_get_kernel(const comms_ofdm_t* h, int32_t direction, size_t n_frames, char* name, size_t name_len) {
    COMMS_ARG(h && name && name_len, "NULL argument");
    COMMS_ARG(direction == COMMS_OFDM_MOD || direction == COMMS_OFDM_DEMOD, "direction must be COMMS_OFDM_MOD or COMMS_OFDM_DEMOD (got %d)",
              direction);
    const bool mod = direction == COMMS_OFDM_MOD;
    unsigned blk, nblk;
    ofdm_block(h, n_frames, mod ? h->T + h->S : h->S, &blk, &nblk);
    const size_t items = n_frames * nblk;
    std::snprintf(name, name_len,
                  "ofdm_%s_kernel<%u> form=wave16 wg=%d n_fft=%u cp=%u data=%u pilots=%u train=%u syms=%u cpe=%d lanes_per_sym=%u syms_per_wave=%u "
                  "block=%u blocks=%u frames=%zu items=%zu grid=%zu max_grid=%u lds=%zu",
                  mod ? "mod" : "demod", h->N, OF_WG, h->N, h->CP, h->D, h->Q, h->T, h->S, (h->flags & COMMS_OFDM_CPE) != 0, h->N / 16, 1024 / h->N,
                  blk, nblk, n_frames, items, of_grid(h, items), h->max_grid, ofdm_lds(static_cast<int>(h->N)));
    return COMMS_OK;
}

comms_status_t comms_ofdm_set_timer(comms_ofdm_t* h, comms_timer_t* t) { return set_handle_timer(h, t); }

comms_status_t comms_ofdm_destroy(comms_ofdm_t* h) { return destroy_handle(h); }

}  // extern "C"
