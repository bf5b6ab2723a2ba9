// iqformat.hip -- raw IQ wire formats <-> Complex<f32>, the step either side of the hot path
// (SURVEY.md section 8f rank 2).  HBM-bound conversions, 16 B per lane where alignment allows.
//
//   i16 pairs (re, im, host byte order) -- src/io/raw_iq.rs:16,50-51,173-178 (IQInput / IQOutput);
//       to f32 it is cast_complex::<i16,f32> (src/util/math.rs:20-28) times a user scale,
//       back it is `(scale * x) as i16` (examples/single_thread_bpsk.rs:40-44: 8192.0 * x as i16;
//       Rust `as`: truncate toward zero, saturate, NaN -> 0);
//   u8 pairs from an RTL-SDR -- examples/fm_radio.rs:82-90: (x as f32 - 127.5) / 127.5.
// And the digital modulators of src/modulation/digital.rs: bits -> Complex<i16> symbols (bpsk/qpsk _bit_mod, _byte_mod).
#include "common.hpp"
#include "fir_handle.hpp"

namespace comms {

__global__ __launch_bounds__(256) void i16_to_c32_kernel(const short2* __restrict__ in, float2* __restrict__ out,
                                                         size_t n, float scale) {
    const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) {
        const short2 v = in[i];
        out[i] = make_float2(static_cast<float>(v.x) * scale, static_cast<float>(v.y) * scale);
    }
}

__global__ __launch_bounds__(256) void c32_to_i16_kernel(const float2* __restrict__ in, short2* __restrict__ out,
                                                         size_t n, float scale) {
    const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float2 v = in[i];
        out[i] = make_short2(rust_as_i16(scale * v.x), rust_as_i16(scale * v.y));
    }
}

__global__ __launch_bounds__(256) void u8_to_c32_kernel(const uchar2* __restrict__ in, float2* __restrict__ out,
                                                        size_t n) {
    const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uchar2 v = in[i];
        out[i] = make_float2((static_cast<float>(v.x) - 127.5f) / 127.5f, (static_cast<float>(v.y) - 127.5f) / 127.5f);
    }
}

// The casts examples/fm_radio.rs wraps around its second filter (Convert2Node :93-117: x -> Complex(x, 0);
// Convert3Node :119-141: x -> x.re), so that its whole chain can stay device-resident: two samples per lane.
__global__ __launch_bounds__(256) void real_to_c32_kernel(const float* __restrict__ in, float2* __restrict__ out, size_t n) {
    const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    const size_t pairs = n / 2;
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < pairs; i += stride) {
        const float2 v = reinterpret_cast<const float2*>(in)[i];
        reinterpret_cast<float4*>(out)[i] = make_float4(v.x, 0.f, v.y, 0.f);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) out[n - 1] = make_float2(in[n - 1], 0.f);
}
__global__ __launch_bounds__(256) void c32_re_kernel(const float2* __restrict__ in, float* __restrict__ out, size_t n) {
    const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    const size_t pairs = n / 2;
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < pairs; i += stride) {
        const float4 v = reinterpret_cast<const float4*>(in)[i];
        reinterpret_cast<float2*>(out)[i] = make_float2(v.x, v.z);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) out[n - 1] = in[n - 1].x;
}

// Digital modulation (src/modulation/digital.rs): bits -> Complex<i16> symbols, elementwise.  A symbol is one
// (re, im) pair of i16 = 4 B; a lane writes the 8 (BPSK) or 4 (QPSK) symbols of its byte as 16-byte stores.
// Out-of-range values of the *_bit_mod forms give (0,0) (the reference returns None; the host entries refuse them).
__device__ __forceinline__ unsigned bpsk_c16(unsigned b) {  // 0 -> (1,0), 1 -> (-1,0) as the dword {re, im}
    return b == 0u ? 0x00000001u : b == 1u ? 0x0000FFFFu : 0u;
}
__device__ __forceinline__ unsigned qpsk_c16(unsigned v) {  // 0 (1,1), 1 (-1,1), 2 (1,-1), 3 (-1,-1)
    const unsigned re = (v & 1u) ? 0xFFFFu : 0x0001u, im = (v & 2u) ? 0xFFFF0000u : 0x00010000u;
    return v < 4u ? (re | im) : 0u;
}
__global__ __launch_bounds__(256) void bpsk_byte_kernel(const uint8_t* __restrict__ in, uint4* __restrict__ out, size_t n) {
    const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) {
        const unsigned b = in[i];
        out[2 * i] = make_uint4(bpsk_c16(b & 1u), bpsk_c16((b >> 1) & 1u), bpsk_c16((b >> 2) & 1u), bpsk_c16((b >> 3) & 1u));
        out[2 * i + 1] = make_uint4(bpsk_c16((b >> 4) & 1u), bpsk_c16((b >> 5) & 1u), bpsk_c16((b >> 6) & 1u), bpsk_c16(b >> 7));
    }
}
__global__ __launch_bounds__(256) void qpsk_byte_kernel(const uint8_t* __restrict__ in, uint4* __restrict__ out, size_t n) {
    const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) {
        const unsigned b = in[i];
        out[i] = make_uint4(qpsk_c16(b & 3u), qpsk_c16((b >> 2) & 3u), qpsk_c16((b >> 4) & 3u), qpsk_c16(b >> 6));
    }
}
template <bool QPSK>
__global__ __launch_bounds__(256) void psk_bit_kernel(const uint8_t* __restrict__ in, unsigned* __restrict__ out, size_t n) {
    const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride)
        out[i] = QPSK ? qpsk_c16(in[i]) : bpsk_c16(in[i]);
}

// Hard decisions (comms_sym_to_bits; the pass behind the chain kinds without a fused store stage): Complex<f32> symbols ->
// packed bits, LSB first, by the rule of common.hpp's sym_decide.  8 B in, k/8 B out per symbol: a lane decides two
// consecutive symbols (one 16-byte load where the input allows it), groups of 32 / 2k lanes OR their bits into one 32-bit
// word, stored by the group's first lane.  Symbols past n add zero bits; the last word stops at the last byte.
template <int K>
__global__ __launch_bounds__(256) void sym_to_bits_kernel(const float2* __restrict__ sym, size_t n, const SymTable t,
                                                          uint8_t* __restrict__ out) {
    constexpr int GL = 32 / (2 * K);
    const size_t n_bytes = (n * K + 7) / 8;
    const size_t n_lanes = (((n + 1) / 2) + 63) & ~static_cast<size_t>(63);  // whole waves: every lane of one takes part in the OR
    const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    const bool wide = (reinterpret_cast<uintptr_t>(sym) & 15) == 0;
    const int l = threadIdx.x & 63;
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n_lanes; i += stride) {
        const size_t j = 2 * i;
        unsigned bits = 0;
        if (j + 1 < n) {
            float2 y0, y1;
            if (wide) {
                const float4 q = reinterpret_cast<const float4*>(sym)[i];
                y0 = make_float2(q.x, q.y);
                y1 = make_float2(q.z, q.w);
            } else {
                y0 = sym[j];
                y1 = sym[j + 1];
            }
            bits = sym_decide<K>(y0, t.c) | (sym_decide<K>(y1, t.c) << K);
        } else if (j < n) {
            bits = sym_decide<K>(sym[j], t.c);
        }
        bits = bits_gather<GL>(bits << (2 * K * (l % GL)));
        if (l % GL == 0 && j < n) bits_store_word(out, j * K / 8, n_bytes, bits);
    }
}

// popcount(a XOR b) over the first n_bits stream bits: 16-byte words where both inputs allow it, bytes otherwise, the
// partial last byte masked; a wave reduction, one 64-bit atomic add per workgroup
__global__ __launch_bounds__(256) void bit_errors_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, uint64_t n_bits,
                                                         unsigned long long* __restrict__ count) {
    const size_t n_full = static_cast<size_t>(n_bits / 8);
    const unsigned rb = static_cast<unsigned>(n_bits % 8);
    const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    const size_t tid = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    unsigned long long acc = 0;
    size_t done = 0;
    if (((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0) {
        const uint4* a4 = reinterpret_cast<const uint4*>(a);
        const uint4* b4 = reinterpret_cast<const uint4*>(b);
        const size_t nw = n_full / 16;
        for (size_t i = tid; i < nw; i += stride) {
            const uint4 x = a4[i], y = b4[i];
            acc += __popc(x.x ^ y.x) + __popc(x.y ^ y.y) + __popc(x.z ^ y.z) + __popc(x.w ^ y.w);
        }
        done = nw * 16;
    }
    for (size_t i = done + tid; i < n_full; i += stride) acc += __popc(static_cast<unsigned>(a[i] ^ b[i]));
    if (rb && tid == 0) acc += __popc(static_cast<unsigned>(a[n_full] ^ b[n_full]) & ((1u << rb) - 1u));
#pragma unroll
    for (int sft = 32; sft >= 1; sft >>= 1) acc += __shfl_xor(acc, sft);
    __shared__ unsigned long long part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long sum = part[0] + part[1] + part[2] + part[3];
        if (sum) atomicAdd(count, sum);
    }
}

static unsigned conv_grid(size_t n) {
    size_t b = (n + 255) / 256;
    if (b > 8u * kNumCU) b = 8u * kNumCU;
    return static_cast<unsigned>(b ? b : 1);
}

// run(d_in, d_out, samples, stream): the device form on the borrowed handle's stream; in_e / out_e bytes per sample (long
// captures go through the chunked host pipeline, common.hpp)
template <typename F>
static comms_status_t via_device(const void* in, size_t n, size_t in_e, void* out, size_t out_e, int32_t device, F run) {
    COMMS_TRY(use_device(device));
    Handle* h = nullptr;
    COMMS_TRY(thread_handle(device, &h));
    return h->run_host_units(in, n * in_e, in_e, out, n * out_e, out_e,
                             [&](void* d_in, void* d_out, size_t ib, size_t) { return run(d_in, d_out, ib / in_e, h->stream); });
}

// digital.rs: bpsk_bit_mod (:6-14), qpsk_bit_mod (:24-36) -- the pulse node's COMMS_SYM_BITS defaults
comms_status_t sym_table(int32_t bits_per_sym, const comms_c32* constellation, SymTable* out) {
    COMMS_ARG(bits_per_sym == 1 || bits_per_sym == 2, "bits_per_sym must be 1 or 2 (got %d)", bits_per_sym);
    static const float2 kBpsk[2] = {{1.f, 0.f}, {-1.f, 0.f}};
    static const float2 kQpsk[4] = {{1.f, 1.f}, {-1.f, 1.f}, {1.f, -1.f}, {-1.f, -1.f}};
    SymTable t{};
    t.k = bits_per_sym;
    for (int v = 0; v < (1 << bits_per_sym); ++v)
        t.c[v] = constellation ? make_float2(constellation[v].re, constellation[v].im) : bits_per_sym == 1 ? kBpsk[v] : kQpsk[v];
    *out = t;
    return COMMS_OK;
}

comms_status_t sym_to_bits_launch(const comms_c32* d_sym, size_t n_sym, const SymTable& t, uint8_t* d_out, hipStream_t s) {
    if (!n_sym) return COMMS_OK;
    const float2* in = reinterpret_cast<const float2*>(d_sym);
    const unsigned grid = conv_grid((n_sym + 1) / 2);
    if (t.k == 1)
        sym_to_bits_kernel<1><<<dim3(grid), dim3(256), 0, s>>>(in, n_sym, t, d_out);
    else
        sym_to_bits_kernel<2><<<dim3(grid), dim3(256), 0, s>>>(in, n_sym, t, d_out);
    return launch_ok("sym_to_bits_kernel");
}

}  // namespace comms

using namespace comms;

extern "C" {

comms_status_t comms_iq_i16_to_c32_dev(const int16_t* d_in, size_t n, float scale, comms_c32* d_out, int32_t device,
                                       void* stream) {
    COMMS_ARG((d_in && d_out) || !n, "NULL device pointer");
    COMMS_ARG((reinterpret_cast<uintptr_t>(d_in) & 3) == 0 && (reinterpret_cast<uintptr_t>(d_out) & 7) == 0,
              "pointers must be aligned to one IQ sample");
    COMMS_TRY(use_device(device));
    if (!n) return COMMS_OK;
    i16_to_c32_kernel<<<dim3(conv_grid(n)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream)>>>(
        reinterpret_cast<const short2*>(d_in), reinterpret_cast<float2*>(d_out), n, scale);
    return launch_ok("i16_to_c32_kernel");
}
comms_status_t comms_iq_c32_to_i16_dev(const comms_c32* d_in, size_t n, float scale, int16_t* d_out, int32_t device,
                                       void* stream) {
    COMMS_ARG((d_in && d_out) || !n, "NULL device pointer");
    COMMS_ARG((reinterpret_cast<uintptr_t>(d_in) & 7) == 0 && (reinterpret_cast<uintptr_t>(d_out) & 3) == 0,
              "pointers must be aligned to one IQ sample");
    COMMS_TRY(use_device(device));
    if (!n) return COMMS_OK;
    c32_to_i16_kernel<<<dim3(conv_grid(n)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream)>>>(
        reinterpret_cast<const float2*>(d_in), reinterpret_cast<short2*>(d_out), n, scale);
    return launch_ok("c32_to_i16_kernel");
}
comms_status_t comms_iq_u8_to_c32_dev(const uint8_t* d_in, size_t n, comms_c32* d_out, int32_t device, void* stream) {
    COMMS_ARG((d_in && d_out) || !n, "NULL device pointer");
    COMMS_ARG((reinterpret_cast<uintptr_t>(d_in) & 1) == 0 && (reinterpret_cast<uintptr_t>(d_out) & 7) == 0,
              "pointers must be aligned to one IQ sample");
    COMMS_TRY(use_device(device));
    if (!n) return COMMS_OK;
    u8_to_c32_kernel<<<dim3(conv_grid(n)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream)>>>(
        reinterpret_cast<const uchar2*>(d_in), reinterpret_cast<float2*>(d_out), n);
    return launch_ok("u8_to_c32_kernel");
}

comms_status_t comms_iq_real_to_c32_dev(const float* d_in, size_t n, comms_c32* d_out, int32_t device, void* stream) {
    COMMS_ARG((d_in && d_out) || !n, "NULL device pointer");
    COMMS_ARG((reinterpret_cast<uintptr_t>(d_in) & 7) == 0 && (reinterpret_cast<uintptr_t>(d_out) & 15) == 0,
              "input must be 8-byte aligned, output 16-byte aligned");
    COMMS_ARG(!ranges_overlap(d_in, n * 4, d_out, n * 8), "the cast cannot run in place");
    COMMS_TRY(use_device(device));
    if (!n) return COMMS_OK;
    real_to_c32_kernel<<<dim3(conv_grid((n + 1) / 2)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream)>>>(
        d_in, reinterpret_cast<float2*>(d_out), n);
    return launch_ok("real_to_c32_kernel");
}
comms_status_t comms_iq_c32_re_dev(const comms_c32* d_in, size_t n, float* d_out, int32_t device, void* stream) {
    COMMS_ARG((d_in && d_out) || !n, "NULL device pointer");
    COMMS_ARG((reinterpret_cast<uintptr_t>(d_in) & 15) == 0 && (reinterpret_cast<uintptr_t>(d_out) & 7) == 0,
              "input must be 16-byte aligned, output 8-byte aligned");
    COMMS_ARG(!ranges_overlap(d_in, n * 8, d_out, n * 4), "the cast cannot run in place");
    COMMS_TRY(use_device(device));
    if (!n) return COMMS_OK;
    c32_re_kernel<<<dim3(conv_grid((n + 1) / 2)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream)>>>(
        reinterpret_cast<const float2*>(d_in), d_out, n);
    return launch_ok("c32_re_kernel");
}

comms_status_t comms_iq_i16_to_c32(const int16_t* in, size_t n, float scale, comms_c32* out, int32_t device) {
    COMMS_ARG((in && out) || !n, "NULL host pointer");
    if (!n) return use_device(device);
    return via_device(in, n, 4, out, 8, device, [&](void* a, void* b, size_t m, void* st) {
        return comms_iq_i16_to_c32_dev(static_cast<const int16_t*>(a), m, scale, static_cast<comms_c32*>(b), device, st);
    });
}
comms_status_t comms_iq_c32_to_i16(const comms_c32* in, size_t n, float scale, int16_t* out, int32_t device) {
    COMMS_ARG((in && out) || !n, "NULL host pointer");
    if (!n) return use_device(device);
    return via_device(in, n, 8, out, 4, device, [&](void* a, void* b, size_t m, void* st) {
        return comms_iq_c32_to_i16_dev(static_cast<const comms_c32*>(a), m, scale, static_cast<int16_t*>(b), device, st);
    });
}
comms_status_t comms_iq_u8_to_c32(const uint8_t* in, size_t n, comms_c32* out, int32_t device) {
    COMMS_ARG((in && out) || !n, "NULL host pointer");
    if (!n) return use_device(device);
    return via_device(in, n, 2, out, 8, device, [&](void* a, void* b, size_t m, void* st) {
        return comms_iq_u8_to_c32_dev(static_cast<const uint8_t*>(a), m, static_cast<comms_c32*>(b), device, st);
    });
}

// ---- hard decisions and bit errors
comms_status_t comms_sym_to_bits_dev(const comms_c32* d_sym, size_t n_sym, int32_t bits_per_sym, const comms_c32* constellation,
                                     uint8_t* d_out, int32_t device, void* stream) {
    COMMS_ARG((d_sym && d_out) || !n_sym, "NULL device pointer");
    COMMS_ARG(n_sym <= SIZE_MAX / 16, "n_sym too large");
    SymTable t;
    COMMS_TRY(sym_table(bits_per_sym, constellation, &t));
    COMMS_ARG((reinterpret_cast<uintptr_t>(d_sym) & 7) == 0, "symbols must be 8-byte aligned");
    COMMS_ARG((reinterpret_cast<uintptr_t>(d_out) & 3) == 0, "d_out must be 4-byte aligned");
    COMMS_ARG(!ranges_overlap(d_sym, n_sym * 8, d_out, (n_sym * bits_per_sym + 7) / 8), "the decision cannot run in place");
    COMMS_TRY(use_device(device));
    return sym_to_bits_launch(d_sym, n_sym, t, d_out, reinterpret_cast<hipStream_t>(stream));
}
comms_status_t comms_sym_to_bits(const comms_c32* sym, size_t n_sym, int32_t bits_per_sym, const comms_c32* constellation,
                                 uint8_t* out, int32_t device) {
    COMMS_ARG((sym && out) || !n_sym, "NULL host pointer");
    COMMS_ARG(n_sym <= SIZE_MAX / 16, "n_sym too large");
    SymTable t;
    COMMS_TRY(sym_table(bits_per_sym, constellation, &t));
    COMMS_TRY(use_device(device));
    if (!n_sym) return COMMS_OK;
    Handle* h = nullptr;
    COMMS_TRY(thread_handle(device, &h));
    // chunks of 32 / k symbols = one whole output word each (the last chunk takes the rest)
    const size_t per_word = static_cast<size_t>(32 / bits_per_sym);
    return h->run_host_units(sym, n_sym * 8, per_word * 8, out, (n_sym * bits_per_sym + 7) / 8, 4,
                             [&](void* d_in, void* d_out, size_t ib, size_t) {
                                 return sym_to_bits_launch(static_cast<const comms_c32*>(d_in), ib / 8, t, static_cast<uint8_t*>(d_out), h->stream);
                             });
}

comms_status_t comms_bit_errors_dev(const uint8_t* d_a, const uint8_t* d_b, uint64_t n_bits, uint64_t* out_errors, int32_t device,
                                    void* stream) {
    COMMS_ARG(out_errors != nullptr && ((d_a && d_b) || !n_bits), "NULL argument");
    COMMS_ARG(device >= 0 && device < 64, "device index out of range");
    COMMS_TRY(use_device(device));
    *out_errors = 0;
    if (!n_bits) return COMMS_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // per-thread, per-device counter, allocated once (every call ends with a stream sync, as the block estimators)
    static thread_local unsigned long long* tl_count[64] = {};
    if (!tl_count[device]) COMMS_HIP_TRY(hipMalloc(&tl_count[device], sizeof(unsigned long long)));
    unsigned long long* d_count = tl_count[device];
    COMMS_HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), s));
    const uint64_t n_bytes = (n_bits + 7) / 8;
    bit_errors_kernel<<<dim3(conv_grid(static_cast<size_t>((n_bytes + 15) / 16))), dim3(256), 0, s>>>(d_a, d_b, n_bits, d_count);
    COMMS_TRY(launch_ok("bit_errors_kernel"));
    unsigned long long count = 0;
    hipError_t e = hipMemcpyAsync(&count, d_count, sizeof(count), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(COMMS_ERR_DEVICE, "bit error count copy-back: %s", hipGetErrorString(e));
    *out_errors = count;
    return COMMS_OK;
}
comms_status_t comms_bit_errors(const uint8_t* a, const uint8_t* b, uint64_t n_bits, uint64_t* out_errors, int32_t device) {
    COMMS_ARG(out_errors != nullptr && ((a && b) || !n_bits), "NULL argument");
    COMMS_TRY(use_device(device));
    *out_errors = 0;
    if (!n_bits) return COMMS_OK;
    Handle* h = nullptr;
    COMMS_TRY(thread_handle(device, &h));
    const size_t n_bytes = static_cast<size_t>((n_bits + 7) / 8);
    const size_t off = (n_bytes + 255) & ~static_cast<size_t>(255);  // b behind a, both 16-byte aligned
    COMMS_TRY(h->in_scratch.reserve(2 * off));
    uint8_t* d = static_cast<uint8_t*>(h->in_scratch.p);
    COMMS_HIP_TRY(hipMemcpyAsync(d, a, n_bytes, hipMemcpyHostToDevice, h->stream));
    COMMS_HIP_TRY(hipMemcpyAsync(d + off, b, n_bytes, hipMemcpyHostToDevice, h->stream));
    return comms_bit_errors_dev(d, d + off, n_bits, out_errors, device, h->stream);
}

// ---- digital modulation
static comms_status_t psk_dev_args(const uint8_t* d_in, size_t n, const comms_c16* d_out, size_t per, int32_t device) {
    COMMS_ARG((d_in && d_out) || !n, "NULL device pointer");
    COMMS_ARG(n <= SIZE_MAX / 32, "n too large");
    COMMS_ARG((reinterpret_cast<uintptr_t>(d_out) & (per > 1 ? 15 : 3)) == 0,
              per > 1 ? "d_out must be 16-byte aligned" : "d_out must be aligned to one Complex<i16>");
    COMMS_ARG(!ranges_overlap(d_in, n, d_out, n * per * 4), "modulation cannot run in place");
    return use_device(device);
}
comms_status_t comms_bpsk_byte_mod_dev(const uint8_t* d_in, size_t n, comms_c16* d_out, int32_t device, void* stream) {
    COMMS_TRY(psk_dev_args(d_in, n, d_out, 8, device));
    if (!n) return COMMS_OK;
    bpsk_byte_kernel<<<dim3(conv_grid(n)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream)>>>(d_in, reinterpret_cast<uint4*>(d_out), n);
    return launch_ok("bpsk_byte_kernel");
}
comms_status_t comms_qpsk_byte_mod_dev(const uint8_t* d_in, size_t n, comms_c16* d_out, int32_t device, void* stream) {
    COMMS_TRY(psk_dev_args(d_in, n, d_out, 4, device));
    if (!n) return COMMS_OK;
    qpsk_byte_kernel<<<dim3(conv_grid(n)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream)>>>(d_in, reinterpret_cast<uint4*>(d_out), n);
    return launch_ok("qpsk_byte_kernel");
}
comms_status_t comms_bpsk_bit_mod_dev(const uint8_t* d_in, size_t n, comms_c16* d_out, int32_t device, void* stream) {
    COMMS_TRY(psk_dev_args(d_in, n, d_out, 1, device));
    if (!n) return COMMS_OK;
    psk_bit_kernel<false><<<dim3(conv_grid(n)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream)>>>(d_in, reinterpret_cast<unsigned*>(d_out), n);
    return launch_ok("psk_bit_kernel");
}
comms_status_t comms_qpsk_bit_mod_dev(const uint8_t* d_in, size_t n, comms_c16* d_out, int32_t device, void* stream) {
    COMMS_TRY(psk_dev_args(d_in, n, d_out, 1, device));
    if (!n) return COMMS_OK;
    psk_bit_kernel<true><<<dim3(conv_grid(n)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream)>>>(d_in, reinterpret_cast<unsigned*>(d_out), n);
    return launch_ok("psk_bit_kernel");
}
comms_status_t comms_bpsk_byte_mod(const uint8_t* in, size_t n, comms_c16* out, int32_t device) {
    COMMS_ARG((in && out) || !n, "NULL host pointer");
    if (!n) return use_device(device);
    return via_device(in, n, 1, out, 32, device, [&](void* a, void* b, size_t m, void* st) {
        return comms_bpsk_byte_mod_dev(static_cast<const uint8_t*>(a), m, static_cast<comms_c16*>(b), device, st);
    });
}
comms_status_t comms_qpsk_byte_mod(const uint8_t* in, size_t n, comms_c16* out, int32_t device) {
    COMMS_ARG((in && out) || !n, "NULL host pointer");
    if (!n) return use_device(device);
    return via_device(in, n, 1, out, 16, device, [&](void* a, void* b, size_t m, void* st) {
        return comms_qpsk_byte_mod_dev(static_cast<const uint8_t*>(a), m, static_cast<comms_c16*>(b), device, st);
    });
}
// the reference returns None for a value the table does not hold: refused here before anything runs
static comms_status_t psk_bit_check(const uint8_t* in, size_t n, unsigned top, const char* what) {
    for (size_t i = 0; i < n; ++i)
        COMMS_ARG(in[i] <= top, "%s: value %u at index %zu is not a symbol (the reference returns None)", what, in[i], i);
    return COMMS_OK;
}
comms_status_t comms_bpsk_bit_mod(const uint8_t* in, size_t n, comms_c16* out, int32_t device) {
    COMMS_ARG((in && out) || !n, "NULL host pointer");
    COMMS_TRY(psk_bit_check(in, n, 1, "bpsk_bit_mod"));
    if (!n) return use_device(device);
    return via_device(in, n, 1, out, 4, device, [&](void* a, void* b, size_t m, void* st) {
        return comms_bpsk_bit_mod_dev(static_cast<const uint8_t*>(a), m, static_cast<comms_c16*>(b), device, st);
    });
}
comms_status_t comms_qpsk_bit_mod(const uint8_t* in, size_t n, comms_c16* out, int32_t device) {
    COMMS_ARG((in && out) || !n, "NULL host pointer");
    COMMS_TRY(psk_bit_check(in, n, 3, "qpsk_bit_mod"));
    if (!n) return use_device(device);
    return via_device(in, n, 1, out, 4, device, [&](void* a, void* b, size_t m, void* st) {
        return comms_qpsk_bit_mod_dev(static_cast<const uint8_t*>(a), m, static_cast<comms_c16*>(b), device, st);
    });
}

}  // extern "C"
