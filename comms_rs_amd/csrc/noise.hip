// noise.hip -- the seeded noise source and the AWGN channel node (NormalNode, UniformNode, random_bit of
// src/util/rand_node.rs:26-152, which seed a host generator from entropy; here the generator is a contract).
//
// The word stream of a source (seed, stream) is Philox4x32-10: block b (64-bit) = philox(counter (b lo, b hi, stream lo,
// stream hi), key (seed lo, seed hi)), its four outputs are stream words 4b ... 4b+3.  Counter based, so there is no
// device state at all: a launch is a pure function of (seed, stream, first block, word offset in it, n), and the handle's
// position -- a 64-bit word count -- lives on the host (get_pos / set_pos / skip never wait for the device).
//
// One lane owns whole blocks, grid-stride.  Every draw kind turns a block into four output values (bits: four 32-bit
// words; uniform / normal: four floats; AWGN: the four floats of two complex samples, so AWGN IS the normal kernel with
// an input added), and value j of the call sits at word (offset + j) of the launch's first block.  A call that starts on
// a block boundary moves whole blocks as 16-byte accesses; one that starts on an even word moves pairs (8 bytes); any
// other start, and the first / last partial block of every call, goes value by value under a mask.  One launch per call.
//
// Box-Muller: z = sqrt(-2 ln u1) * (cos, sin)(2 pi u2) on the hardware's v_log_f32 / v_sqrt_f32 / v_cos_f32 / v_sin_f32 (the
// last two take their angle in revolutions: u2 itself).  Measured against the formula in f64 over 2^24 values this is
// 3.3e-7 * max(1, |z|) off at worst, against the contract's 2^-17 = 7.6e-6, and a tenth faster at 2^28 samples than
// logf / sqrtf / sincospif (2.1e-7), which the diagnostic build keeps selectable (COMMS_NOISE_FAST=0): NOTES.md, "Noise source".
#include "common.hpp"

namespace comms {

constexpr unsigned kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;
constexpr unsigned kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;

__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint2 k) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(kPhiloxM0, c.x), lo0 = kPhiloxM0 * c.x;
        const unsigned hi1 = __umulhi(kPhiloxM1, c.z), lo1 = kPhiloxM1 * c.z;
        c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
        k.x += kPhiloxW0;
        k.y += kPhiloxW1;
    }
    return c;
}

struct NoiseSrc {
    uint2 key;       // seed lo, hi
    uint2 strm;      // stream lo, hi
    uint64_t blk0;   // block of the call's first word
    unsigned off;    // word offset of the first value in that block, 0 ... 3
};
__device__ __forceinline__ uint4 noise_block(const NoiseSrc& s, size_t t) {
    const uint64_t b = (s.blk0 + t) & ((uint64_t{1} << 62) - 1);  // 2^64 words = 2^62 blocks: word 2^64 - 1 is followed by word 0
    return philox4x32_10(make_uint4(static_cast<unsigned>(b), static_cast<unsigned>(b >> 32), s.strm.x, s.strm.y), s.key);
}

// (a, b) -> the pair (r cos 2 pi u2, r sin 2 pi u2), u1 = ((a >> 8) + 1) 2^-24 in (0, 1], u2 = (b >> 8) 2^-24 in [0, 1)
template <bool FAST>
__device__ __forceinline__ void box_muller(unsigned a, unsigned b, float& zc, float& zs) {
    const float u1 = static_cast<float>((a >> 8) + 1u) * 0x1.0p-24f;
    const float u2 = static_cast<float>(b >> 8) * 0x1.0p-24f;
    if constexpr (FAST) {
        // ln u1 = ln 2 * log2 u1; u1 >= 2^-24 is a normal number, which is all v_log_f32 / v_sqrt_f32 need
        const float r = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u1));
        zc = r * __builtin_amdgcn_cosf(u2);
        zs = r * __builtin_amdgcn_sinf(u2);
    } else {
        const float r = sqrtf(-2.0f * logf(u1));
        float s, c;
        sincospif(2.0f * u2, &s, &c);
        zc = r * c;
        zs = r * s;
    }
}

// ---- loads of the AWGN input (IN: 0 none, 1 f32, 2 i16 times scale) and stores, 1 / 2 / 4 values at value index j
template <int IN>
__device__ __forceinline__ float in1(const void* in, size_t j, float scale) {
    if constexpr (IN == 1) return static_cast<const float*>(in)[j];
    else if constexpr (IN == 2) return static_cast<float>(static_cast<const short*>(in)[j]) * scale;
    else return 0.0f;
}
template <int IN>
__device__ __forceinline__ void in2(const void* in, size_t j, float scale, float* x) {
    if constexpr (IN == 1) {
        const float2 v = *reinterpret_cast<const float2*>(static_cast<const float*>(in) + j);
        x[0] = v.x, x[1] = v.y;
    } else if constexpr (IN == 2) {
        const short2 v = *reinterpret_cast<const short2*>(static_cast<const short*>(in) + j);
        x[0] = static_cast<float>(v.x) * scale, x[1] = static_cast<float>(v.y) * scale;
    }
}
template <int IN>
__device__ __forceinline__ void in4(const void* in, size_t j, float scale, float* x) {
    if constexpr (IN == 1) {
        const float4 v = *reinterpret_cast<const float4*>(static_cast<const float*>(in) + j);
        x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
    } else if constexpr (IN == 2) {
        const short4 v = *reinterpret_cast<const short4*>(static_cast<const short*>(in) + j);
        x[0] = static_cast<float>(v.x) * scale, x[1] = static_cast<float>(v.y) * scale;
        x[2] = static_cast<float>(v.z) * scale, x[3] = static_cast<float>(v.w) * scale;
    }
}
__device__ __forceinline__ void out2(float* o, float a, float b) { *reinterpret_cast<float2*>(o) = make_float2(a, b); }
__device__ __forceinline__ void out2(double* o, double a, double b) { *reinterpret_cast<double2*>(o) = make_double2(a, b); }
__device__ __forceinline__ void out4(float* o, const float* v) { *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]); }
__device__ __forceinline__ void out4(double* o, const double* v) {
    out2(o, v[0], v[1]);
    out2(o + 2, v[2], v[3]);
}

// Value j of a call sits at word q = off + j of the launch's first block; lane t holds words 4 t ... 4 t + 3.  q is compared
// against off before anything is subtracted (j is a signed quantity in the first block).  A whole block goes as one
// 16-byte access when the call starts on a block boundary (`wide`: and the pointers allow it).
__device__ __forceinline__ bool whole_block(size_t first, unsigned off, size_t n, bool wide = true) {
    return wide && off == 0 && first + 4 <= n;
}

// normal / AWGN: out[j] = base + sd * z_j with base = mu (IN == 0) or the input value j (sd == 0: the input itself).
// in == out is allowed (no __restrict__): a lane reads exactly the values it then writes.
template <int IN, class OutT, bool FAST>
__global__ __launch_bounds__(256) void noise_normal_kernel(NoiseSrc src, size_t n, OutT mu, OutT sd, float in_scale,
                                                           const void* in, OutT* out, bool wide) {
    const size_t nblk = (src.off + n + 3) / 4;
    const size_t stride = static_cast<size_t>(gridDim.x) * 256;
    const bool copy = IN != 0 && sd == OutT(0);
    for (size_t t = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; t < nblk; t += stride) {
        const uint4 w = noise_block(src, t);
        float z[4];
        box_muller<FAST>(w.x, w.y, z[0], z[1]);
        box_muller<FAST>(w.z, w.w, z[2], z[3]);
        const size_t first = 4 * t;
        float x[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        OutT v[4];
        auto mix = [&](int i) { return copy ? OutT(x[i]) : (IN ? OutT(x[i]) : mu) + sd * OutT(z[i]); };
        if (whole_block(first, src.off, n, wide)) {
            in4<IN>(in, first, in_scale, x);
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = mix(i);
            out4(out + first, v);
        } else if ((src.off & 1) == 0) {
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const size_t q = first + 2 * p;  // word of the launch; value index q - off
                if (q >= src.off && q - src.off + 2 <= n) {
                    const size_t j = q - src.off;
                    in2<IN>(in, j, in_scale, x + 2 * p);
                    out2(out + j, mix(2 * p), mix(2 * p + 1));
                } else {
#pragma unroll
                    for (int i = 2 * p; i < 2 * p + 2; ++i) {
                        const size_t qq = first + i;
                        if (qq >= src.off && qq - src.off < n) {
                            x[i] = in1<IN>(in, qq - src.off, in_scale);
                            out[qq - src.off] = mix(i);
                        }
                    }
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const size_t q = first + i;
                if (q >= src.off && q - src.off < n) {
                    x[i] = in1<IN>(in, q - src.off, in_scale);
                    out[q - src.off] = mix(i);
                }
            }
        }
    }
}

// uniform: lo + (hi - lo) u in f64 (exact up to the one rounding to f32, and no overflow of hi - lo), u = (w >> 8) 2^-24;
// a result that rounds to hi becomes `below` = the float just under hi
__global__ __launch_bounds__(256) void noise_uniform_kernel(NoiseSrc src, size_t n, float lo, float hi, float below,
                                                            float* __restrict__ out) {
    const size_t nblk = (src.off + n + 3) / 4;
    const size_t stride = static_cast<size_t>(gridDim.x) * 256;
    const double dlo = lo, span = static_cast<double>(hi) - static_cast<double>(lo);
    for (size_t t = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; t < nblk; t += stride) {
        const uint4 w = noise_block(src, t);
        const unsigned ww[4] = {w.x, w.y, w.z, w.w};
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float f = static_cast<float>(dlo + span * (static_cast<double>(ww[i] >> 8) * 0x1.0p-24));
            v[i] = f >= hi ? below : f;
        }
        const size_t first = 4 * t;
        if (whole_block(first, src.off, n)) {
            out4(out + first, v);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const size_t q = first + i;
                if (q >= src.off && q - src.off < n) out[q - src.off] = v[i];
            }
        }
    }
}

// one output bit per byte (0 / 1): four stream bits -> one dword
__device__ __forceinline__ unsigned noise_spread4(unsigned x) { return ((x & 0xFu) * 0x00204081u) & 0x01010101u; }

// bits: output word j (stream bits 32 j ... 32 j + 31 of the call) = word (off + j) of the launch; n bits in all.
// packed: bytes 4 j ... of out; u8: bytes 32 j ... .  Nothing past the last bit's byte is written; the bits past n in the
// last packed byte are 0.
__global__ __launch_bounds__(256) void noise_bits_kernel(NoiseSrc src, size_t n, int packed, uint8_t* __restrict__ out) {
    const size_t nw = (n + 31) / 32;
    const size_t nblk = (src.off + nw + 3) / 4;
    const size_t stride = static_cast<size_t>(gridDim.x) * 256;
    for (size_t t = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; t < nblk; t += stride) {
        const uint4 w = noise_block(src, t);
        const unsigned ww[4] = {w.x, w.y, w.z, w.w};
        const size_t first = 4 * t;
        if (packed && src.off == 0 && (first + 4) * 32 <= n) {
            *reinterpret_cast<uint4*>(out + first * 4) = w;
            continue;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const size_t q = first + i;
            if (q < src.off || q - src.off >= nw) continue;
            const size_t j = q - src.off;
            unsigned x = ww[i];
            const size_t left = n - j * 32;  // >= 1
            if (left >= 32) {
                if (packed) {
                    *reinterpret_cast<unsigned*>(out + j * 4) = x;
                } else {
                    uint4* o = reinterpret_cast<uint4*>(out + j * 32);
                    o[0] = make_uint4(noise_spread4(x), noise_spread4(x >> 4), noise_spread4(x >> 8), noise_spread4(x >> 12));
                    o[1] = make_uint4(noise_spread4(x >> 16), noise_spread4(x >> 20), noise_spread4(x >> 24), noise_spread4(x >> 28));
                }
            } else {
                const unsigned rem = static_cast<unsigned>(left);
                x &= (1u << rem) - 1u;
                if (packed) {
                    for (unsigned b = 0; b < (rem + 7) / 8; ++b) out[j * 4 + b] = static_cast<uint8_t>(x >> (8 * b));
                } else {
                    for (unsigned b = 0; b < rem; ++b) out[j * 32 + b] = static_cast<uint8_t>((x >> b) & 1u);
                }
            }
        }
    }
}

}  // namespace comms

using namespace comms;

struct comms_noise : Handle {
    uint64_t seed = 0, strm = 0;
    uint64_t pos = 0;  // next word of the stream
    int32_t in_format = COMMS_IQ_C32;
    float in_scale = 1.0f;
    NoiseSrc src_at(uint64_t p) const {
        NoiseSrc s;
        s.key = make_uint2(static_cast<unsigned>(seed), static_cast<unsigned>(seed >> 32));
        s.strm = make_uint2(static_cast<unsigned>(strm), static_cast<unsigned>(strm >> 32));
        s.blk0 = p >> 2;
        s.off = static_cast<unsigned>(p & 3);
        return s;
    }
};
static_assert(!std::is_copy_constructible_v<comms_noise>, "a handle is never copied");

// lanes own blocks; at most 8 workgroups of 256 per CU, the grid-stride loop takes the rest
static unsigned noise_grid(size_t n_values, unsigned off) {
    const size_t nblk = (off + n_values + 3) / 4;
    const size_t want = (nblk + 255) / 256;
    const size_t cap = static_cast<size_t>(kNumCU) * 8;
    return static_cast<unsigned>(want < cap ? (want ? want : 1) : cap);
}


template <int IN, class OutT>
static comms_status_t normal_launch(comms_noise* h, uint64_t p, size_t n_values, OutT mu, OutT sd, const void* d_in, OutT* d_out,
                                    hipStream_t s) {
    // whole blocks of i16 input are 8-byte loads; a 4-byte aligned input goes pair by pair (same values)
    const bool wide = IN != 2 || (reinterpret_cast<uintptr_t>(d_in) & 7) == 0;
    const NoiseSrc src = h->src_at(p);
    const dim3 grid(noise_grid(n_values, src.off)), block(256);
    h->tic(s);
#ifdef COMMS_DIAG  // the libm form, for scripts/bench_noise.py --forms
    if (!diag_knob("COMMS_NOISE_FAST", 1))
        noise_normal_kernel<IN, OutT, false><<<grid, block, 0, s>>>(src, n_values, mu, sd, h->in_scale, d_in, d_out, wide);
    else
#endif
        noise_normal_kernel<IN, OutT, true><<<grid, block, 0, s>>>(src, n_values, mu, sd, h->in_scale, d_in, d_out, wide);
    h->toc(s);
    return launch_ok("noise_normal_kernel");
}

// host-pointer form of a source: the values are produced into staging (host-mapped for short calls) and copied out
template <class F>
static comms_status_t source_run_host(comms_noise* h, void* out, size_t bytes, F&& launch) {
    if (bytes <= zero_copy_limit()) {
        COMMS_TRY(h->pin_out.reserve(bytes));
        COMMS_TRY(launch(h->pin_out.d));
        COMMS_HIP_TRY(hipStreamSynchronize(h->stream));
        std::memcpy(out, h->pin_out.h, bytes);
        return COMMS_OK;
    }
    COMMS_TRY(h->out_scratch.reserve(bytes));
    COMMS_TRY(launch(h->out_scratch.p));
    COMMS_HIP_TRY(hipMemcpyAsync(out, h->out_scratch.p, bytes, hipMemcpyDeviceToHost, h->stream));
    COMMS_HIP_TRY(hipStreamSynchronize(h->stream));
    return COMMS_OK;
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static bool sd_ok(double sd) { return std::isfinite(sd) && sd >= 0.0; }

extern "C" {

comms_status_t comms_noise_create(uint64_t seed, uint64_t stream, int32_t device, comms_noise_t** out) {
    COMMS_ARG(out != nullptr, "out is NULL");
    *out = nullptr;
    HandlePtr<comms_noise> h;
    COMMS_TRY(make_handle(device, &h));
    h->seed = seed;
    h->strm = stream;
    *out = h.release();
    return COMMS_OK;
}

comms_status_t comms_noise_destroy(comms_noise_t* h) { return destroy_handle(h); }

comms_status_t comms_noise_set_timer(comms_noise_t* h, comms_timer_t* t) { return set_handle_timer(h, t); }

comms_status_t comms_noise_get_pos(const comms_noise_t* h, uint64_t* pos) {
    COMMS_ARG(h && pos, "NULL argument");
    *pos = h->pos;
    return COMMS_OK;
}

comms_status_t comms_noise_set_pos(comms_noise_t* h, uint64_t pos) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    h->pos = pos;
    return COMMS_OK;
}

comms_status_t comms_noise_skip(comms_noise_t* h, uint64_t n_words) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    h->pos += n_words;
    return COMMS_OK;
}

// ---- bits
comms_status_t comms_noise_bits_run_dev(comms_noise_t* h, size_t n, int32_t format, uint8_t* d_out, void* stream) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG(format == COMMS_BITS_U8 || format == COMMS_BITS_PACKED, "format must be COMMS_BITS_U8 or COMMS_BITS_PACKED (got %d)", format);
    COMMS_ARG(d_out != nullptr || !n, "NULL device pointer");
    COMMS_ARG(aligned16(d_out), "d_out must be 16-byte aligned");
    COMMS_TRY(use_device(h->device));
    if (!n) return COMMS_OK;
    hipStream_t s = h->pick(stream);
    const NoiseSrc src = h->src_at(h->pos);
    const size_t nw = (n + 31) / 32;
    h->tic(s);
    noise_bits_kernel<<<dim3(noise_grid(nw, src.off)), dim3(256), 0, s>>>(src, n, format == COMMS_BITS_PACKED, d_out);
    h->toc(s);
    COMMS_TRY(launch_ok("noise_bits_kernel"));
    h->pos += nw;
    return COMMS_OK;
}

comms_status_t comms_noise_bits_run(comms_noise_t* h, size_t n, int32_t format, uint8_t* out) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG(format == COMMS_BITS_U8 || format == COMMS_BITS_PACKED, "format must be COMMS_BITS_U8 or COMMS_BITS_PACKED (got %d)", format);
    COMMS_ARG(out != nullptr || !n, "NULL host pointer");
    COMMS_TRY(use_device(h->device));
    if (!n) return COMMS_OK;
    const size_t bytes = format == COMMS_BITS_U8 ? n : (n + 7) / 8;
    return source_run_host(h, out, bytes, [&](void* d) { return comms_noise_bits_run_dev(h, n, format, static_cast<uint8_t*>(d), COMMS_STREAM_HANDLE); });
}

// ---- uniform
static comms_status_t uniform_args(float lo, float hi) {
    COMMS_ARG(std::isfinite(lo) && std::isfinite(hi), "uniform bounds must be finite");
    COMMS_ARG(lo < hi, "uniform needs lo < hi (got [%g, %g))", static_cast<double>(lo), static_cast<double>(hi));
    return COMMS_OK;
}

comms_status_t comms_noise_uniform_run_dev(comms_noise_t* h, size_t n, float lo, float hi, float* d_out, void* stream) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_TRY(uniform_args(lo, hi));
    COMMS_ARG(d_out != nullptr || !n, "NULL device pointer");
    COMMS_ARG(aligned16(d_out), "d_out must be 16-byte aligned");
    COMMS_TRY(use_device(h->device));
    if (!n) return COMMS_OK;
    hipStream_t s = h->pick(stream);
    const NoiseSrc src = h->src_at(h->pos);
    h->tic(s);
    noise_uniform_kernel<<<dim3(noise_grid(n, src.off)), dim3(256), 0, s>>>(src, n, lo, hi, std::nextafterf(hi, -INFINITY), d_out);
    h->toc(s);
    COMMS_TRY(launch_ok("noise_uniform_kernel"));
    h->pos += n;
    return COMMS_OK;
}

comms_status_t comms_noise_uniform_run(comms_noise_t* h, size_t n, float lo, float hi, float* out) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_TRY(uniform_args(lo, hi));
    COMMS_ARG(out != nullptr || !n, "NULL host pointer");
    COMMS_TRY(use_device(h->device));
    if (!n) return COMMS_OK;
    return source_run_host(h, out, n * sizeof(float), [&](void* d) { return comms_noise_uniform_run_dev(h, n, lo, hi, static_cast<float*>(d), COMMS_STREAM_HANDLE); });
}

// ---- normal
comms_status_t comms_noise_normal_run_dev(comms_noise_t* h, size_t n, double mu, double sd, float* d_out, void* stream) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG(std::isfinite(mu) && sd_ok(sd), "normal needs a finite mu and a finite sd >= 0");
    COMMS_ARG(d_out != nullptr || !n, "NULL device pointer");
    COMMS_ARG(aligned16(d_out), "d_out must be 16-byte aligned");
    COMMS_TRY(use_device(h->device));
    if (!n) return COMMS_OK;
    COMMS_TRY((normal_launch<0, float>(h, h->pos, n, static_cast<float>(mu), static_cast<float>(sd), nullptr, d_out, h->pick(stream))));
    h->pos += n;
    return COMMS_OK;
}

comms_status_t comms_noise_normal_run(comms_noise_t* h, size_t n, double mu, double sd, float* out) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG(std::isfinite(mu) && sd_ok(sd), "normal needs a finite mu and a finite sd >= 0");
    COMMS_ARG(out != nullptr || !n, "NULL host pointer");
    COMMS_TRY(use_device(h->device));
    if (!n) return COMMS_OK;
    return source_run_host(h, out, n * sizeof(float), [&](void* d) { return comms_noise_normal_run_dev(h, n, mu, sd, static_cast<float*>(d), COMMS_STREAM_HANDLE); });
}

comms_status_t comms_noise_normal_f64_run_dev(comms_noise_t* h, size_t n, double mu, double sd, double* d_out, void* stream) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG(std::isfinite(mu) && sd_ok(sd), "normal needs a finite mu and a finite sd >= 0");
    COMMS_ARG(d_out != nullptr || !n, "NULL device pointer");
    COMMS_ARG(aligned16(d_out), "d_out must be 16-byte aligned");
    COMMS_TRY(use_device(h->device));
    if (!n) return COMMS_OK;
    COMMS_TRY((normal_launch<0, double>(h, h->pos, n, mu, sd, nullptr, d_out, h->pick(stream))));
    h->pos += n;
    return COMMS_OK;
}

comms_status_t comms_noise_normal_f64_run(comms_noise_t* h, size_t n, double mu, double sd, double* out) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG(std::isfinite(mu) && sd_ok(sd), "normal needs a finite mu and a finite sd >= 0");
    COMMS_ARG(out != nullptr || !n, "NULL host pointer");
    COMMS_TRY(use_device(h->device));
    if (!n) return COMMS_OK;
    return source_run_host(h, out, n * sizeof(double), [&](void* d) { return comms_noise_normal_f64_run_dev(h, n, mu, sd, static_cast<double*>(d), COMMS_STREAM_HANDLE); });
}

// ---- AWGN
comms_status_t comms_awgn_set_input_format(comms_noise_t* h, int32_t format, float scale) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG(format == COMMS_IQ_C32 || format == COMMS_IQ_I16, "the AWGN node reads COMMS_IQ_C32 or COMMS_IQ_I16 (got %d)", format);
    COMMS_ARG(format != COMMS_IQ_I16 || std::isfinite(scale), "scale must be finite");
    h->in_format = format;
    h->in_scale = format == COMMS_IQ_I16 ? scale : 1.0f;
    return COMMS_OK;
}

comms_status_t comms_awgn_run_dev(comms_noise_t* h, const void* d_in, size_t n, float sigma, comms_c32* d_out, void* stream) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG(sd_ok(sigma), "sigma must be finite and >= 0");
    COMMS_ARG((d_in != nullptr && d_out != nullptr) || !n, "NULL device pointer");
    const bool i16 = h->in_format == COMMS_IQ_I16;
    COMMS_ARG((reinterpret_cast<uintptr_t>(d_in) & (i16 ? 3 : 15)) == 0, i16 ? "d_in must be 4-byte aligned" : "d_in must be 16-byte aligned");
    COMMS_ARG(aligned16(d_out), "d_out must be 16-byte aligned");
    COMMS_ARG(n <= (SIZE_MAX >> 4), "n is too large");
    // in place is the same address; any other overlap would let one lane overwrite another's input
    COMMS_ARG(static_cast<const void*>(d_out) == d_in || !ranges_overlap(d_in, n * (i16 ? 4 : 8), d_out, n * 8),
              "input and output overlap (in place means d_in == d_out)");
    COMMS_ARG(!(i16 && static_cast<const void*>(d_out) == d_in) || !n, "in place needs Complex<f32> input");
    COMMS_TRY(use_device(h->device));
    if (!n) return COMMS_OK;
    const uint64_t p = (h->pos + 1) & ~uint64_t{1};  // a complex draw starts on an even word
    hipStream_t s = h->pick(stream);
    if (i16) {
        COMMS_TRY((normal_launch<2, float>(h, p, 2 * n, 0.0f, sigma, d_in, reinterpret_cast<float*>(d_out), s)));
    } else {
        COMMS_TRY((normal_launch<1, float>(h, p, 2 * n, 0.0f, sigma, d_in, reinterpret_cast<float*>(d_out), s)));
    }
    h->pos = p + 2 * n;
    return COMMS_OK;
}

comms_status_t comms_awgn_run(comms_noise_t* h, const void* in, size_t n, float sigma, comms_c32* out) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG(sd_ok(sigma), "sigma must be finite and >= 0");
    COMMS_ARG((in != nullptr && out != nullptr) || !n, "NULL host pointer");
    COMMS_ARG(n <= (SIZE_MAX >> 4), "n is too large");
    COMMS_TRY(use_device(h->device));
    if (!n) return COMMS_OK;
    const size_t in_u = h->in_format == COMMS_IQ_I16 ? 4 : 8;
    // the pipeline's unit is one block = two samples, so that every chunk starts on a block boundary
    return h->run_host_units(in, n * in_u, 2 * in_u, out, n * 8, 16, [&](void* d_in, void* d_out, size_t, size_t out_bytes) {
        return comms_awgn_run_dev(h, d_in, out_bytes / 8, sigma, static_cast<comms_c32*>(d_out), COMMS_STREAM_HANDLE);
    });
}

}  // extern "C"
