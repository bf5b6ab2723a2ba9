// fir_exact.hip -- FirNode / BatchFirNode / PulseNode over Complex<i16> and Complex<f64>: the two sample types whose
// outputs are BIT-IDENTICAL to the reference's (the tests compare for equality).
//
// The reference's fir(), batch_fir() and PulseNode are generic over T: Num + Copy (src/filter/fir.rs:43-54, :87-102;
// src/pulse.rs:38-93).  Its own tests run them on Complex<i16> (src/filter/fir_node.rs:259-313, src/pulse.rs:129-183); its
// doc example of batch_fir (fir.rs:68-86) and its timing estimator (src/demodulation/timing_estimator.rs:102-103)
// instantiate them on Complex<f64>.  Every BASELINE config is f32 -- those are the tuned kernels of fir.hip -- but a graph
// that carries integer or f64 samples must find its nodes too.  One kernel template, one handle and one set of host
// functions serve both; what differs per sample type sits in Exact<V> below.
//
// One kernel serves all three nodes: out[m * sps + p] = sum_j taps[p + j * sps] * x[m - j]  (sps = 1: the FIR; k = p + j * sps
// ascending, as fir() walks it).  The pulse shaper's zero-stuffed samples contribute products by zero, which leave every sum
// as it is, so they are skipped (f64: +0.0 or -0.0 terms added to a sum folded from +0.0 change at most the sign of an exactly
// zero result, which is +0.0 either way).  A plain tiled form -- taps in LDS, inputs through the cache, one output per
// thread -- and no claim on the roofline.
#include <vector>

#include "common.hpp"
#include "stream_call.hpp"

namespace comms {

// Per sample type: the device vector V, the ABI's complex C, the accumulator, the multiply-accumulate, the final pack,
// the taps staged in LDS per pass, and the names the error messages use.
template <class V>
struct Exact;

// Complex<i16>: products and sums wrap modulo 2^16 (Rust release builds; a debug build panics on overflow instead).
// Z / 2^16 is a ring quotient of Z / 2^32, so the kernel accumulates in 32-bit wrapping arithmetic and truncates once:
// bit-identical to wrapping at every step.
template <>
struct Exact<short2> {
    using C = comms_c16;
    using Acc = unsigned;
    static constexpr int kTapsLds = 4096;
    static constexpr const char* kNoun = "integer";
    static constexpr const char* kKernel = "fir_exact_kernel<short2>";
    static __host__ __device__ short2 make(short re, short im) { return make_short2(re, im); }
    static __device__ __forceinline__ void mac(Acc& ar, Acc& ai, short2 t, short2 x) {
        ar += static_cast<unsigned>(static_cast<int>(t.x) * x.x - static_cast<int>(t.y) * x.y);
        ai += static_cast<unsigned>(static_cast<int>(t.x) * x.y + static_cast<int>(t.y) * x.x);
    }
    static __device__ __forceinline__ short2 pack(Acc ar, Acc ai) {
        return make_short2(static_cast<short>(ar & 0xffffu), static_cast<short>(ai & 0xffffu));
    }
};

// Complex<f64>: exactly the reference's arithmetic.  Each product is num::Complex's (ar*br - ai*bi, ar*bi + ai*br) -- four
// multiplications, one subtraction, one addition, no FMA (-ffp-contract=off, Makefile) -- and the sum folds from zero with
// the taps ascending (`taps.iter().zip(state).map(|(x, y)| x * y).sum()`, fir.rs:53,99).  f64 has no tolerance to hide behind.
template <>
struct Exact<double2> {
    using C = comms_c64;
    using Acc = double;
    static constexpr int kTapsLds = 2048;  // 32 KiB
    static constexpr const char* kNoun = "f64";
    static constexpr const char* kKernel = "fir_exact_kernel<double2>";
    static __host__ __device__ double2 make(double re, double im) { return make_double2(re, im); }
    static __device__ __forceinline__ void mac(Acc& ar, Acc& ai, double2 t, double2 x) {
        const double pr = t.x * x.x - t.y * x.y;  // num::Complex Mul
        const double pi = t.x * x.y + t.y * x.x;
        ar = ar + pr;  // Sum
        ai = ai + pi;
    }
    static __device__ __forceinline__ double2 pack(Acc ar, Acc ai) { return make_double2(ar, ai); }
};

template <class V>
__device__ __forceinline__ V stream_at(const V* __restrict__ in, const V* __restrict__ hist, int hist_len, long long g, size_t n) {
    if (g >= 0) return static_cast<size_t>(g) < n ? in[g] : Exact<V>::make(0, 0);
    return g >= -static_cast<long long>(hist_len) ? hist[hist_len + g] : Exact<V>::make(0, 0);
}

template <class V>
__global__ __launch_bounds__(256) void fir_exact_kernel(const V* __restrict__ in, const V* __restrict__ hist, int hist_len,
                                                        const V* __restrict__ taps, int n_taps, int sps, V* __restrict__ out,
                                                        size_t n_in, V* __restrict__ new_hist) {
    using T = Exact<V>;
    constexpr int kLds = T::kTapsLds;  // taps staged per pass
    __shared__ V tp[kLds];
    if (blockIdx.x == 0)  // new_hist = last hist_len samples of concat(old_hist, in)
        for (int j = threadIdx.x; j < hist_len; j += blockDim.x) {
            const size_t p = n_in + static_cast<size_t>(j);
            new_hist[j] = p < static_cast<size_t>(hist_len) ? hist[p] : in[p - hist_len];
        }
    const size_t n_out = n_in * static_cast<size_t>(sps);
    const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    const size_t rounds = (n_out + stride - 1) / stride;
    for (size_t r = 0; r < rounds; ++r) {
        const size_t i = r * stride + static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
        const size_t m = i / sps;
        const int p = static_cast<int>(i - m * sps);
        typename T::Acc ar = 0, ai = 0;
        for (int k0 = 0; k0 < n_taps; k0 += kLds) {
            const int kc = n_taps - k0 < kLds ? n_taps - k0 : kLds;
            __syncthreads();
            for (int k = threadIdx.x; k < kc; k += blockDim.x) tp[k] = taps[k0 + k];
            __syncthreads();
            if (i < n_out) {
                // taps k = p + j * sps inside [k0, k0 + kc)
                int j = k0 > p ? (k0 - p + sps - 1) / sps : 0;
                for (int k = p + j * sps; k < k0 + kc; k += sps, ++j)
                    T::mac(ar, ai, tp[k - k0], stream_at(in, hist, hist_len, static_cast<long long>(m) - j, n_in));
            }
        }
        if (i < n_out) out[i] = T::pack(ar, ai);
    }
}

// one handle for both nodes (sps = 1: FIR with the reference's `state` semantics)
template <class V>
struct ExactFir : Handle {
    int n_eff = 0;      // taps that take part
    int sps = 1;
    int hist_len = 0;   // samples (FIR: n_eff) or symbols (pulse: ceil(n_taps / sps)) of history
    DevBuf<V> taps;
    History hist;
};
static_assert(!std::is_copy_constructible_v<ExactFir<short2>>, "a handle is never copied");

}  // namespace comms

using namespace comms;

struct comms_fir_i16 : ExactFir<short2> {};
struct comms_pulse_i16 : ExactFir<short2> {};
struct comms_fir_f64 : ExactFir<double2> {};
struct comms_pulse_f64 : ExactFir<double2> {};
static_assert(!std::is_copy_constructible_v<comms_fir_i16> && !std::is_copy_constructible_v<comms_pulse_i16> &&
                  !std::is_copy_constructible_v<comms_fir_f64> && !std::is_copy_constructible_v<comms_pulse_f64>,
              "a handle is never copied");

namespace {

template <class V>
using CxOf = typename Exact<V>::C;

template <class V, class H>
comms_status_t create(const CxOf<V>* taps, size_t n_eff, int sps, size_t hist_len, const CxOf<V>* state, size_t n_state,
                      int32_t device, H** out) {
    HandlePtr<H> h;
    COMMS_TRY(make_handle(device, &h));
    h->n_eff = static_cast<int>(n_eff);
    h->sps = sps;
    h->hist_len = static_cast<int>(hist_len);
    COMMS_HIP_TRY(h->taps.upload(reinterpret_cast<const V*>(taps), n_eff));
    COMMS_HIP_TRY(h->hist.alloc(hist_len, sizeof(V)));
    if (n_state) COMMS_HIP_TRY(h->hist.upload(state, n_state));
    *out = h.release();
    return COMMS_OK;
}

template <class V, class H>
comms_status_t fir_create(const CxOf<V>* taps, size_t n_taps, const CxOf<V>* state, size_t n_state, int32_t device, H** out) {
    COMMS_ARG(out != nullptr, "out is NULL");
    *out = nullptr;
    COMMS_ARG(taps != nullptr && n_taps > 0, "taps must hold at least one tap (the reference panics on an empty state)");
    COMMS_ARG(state == nullptr || n_state > 0, "a user state must hold at least one sample");
    size_t n_eff = n_taps;
    if (state && n_state < n_eff) n_eff = n_state;  // zip(taps, state), fir.rs:53
    COMMS_ARG(n_eff <= (1u << 20), "too many taps (%zu)", n_eff);
    return create<V>(taps, n_eff, 1, n_eff, state, state ? n_state : 0, device, out);
}

template <class V, class H>
comms_status_t pulse_create(const CxOf<V>* taps, size_t n_taps, size_t sam_per_sym, int32_t device, H** out) {
    COMMS_ARG(out != nullptr, "out is NULL");
    *out = nullptr;
    COMMS_ARG(taps != nullptr && n_taps > 0, "taps must hold at least one tap");
    COMMS_ARG(sam_per_sym >= 1 && sam_per_sym <= (1u << 16), "sam_per_sym must be in [1, 65536] (0 underflows in the reference)");
    COMMS_ARG(n_taps <= (1u << 20), "too many taps (%zu)", n_taps);
    const size_t hist = (n_taps + sam_per_sym - 1) / sam_per_sym;  // symbols the filter reaches back over
    return create<V>(taps, n_taps, static_cast<int>(sam_per_sym), hist, nullptr, 0, device, out);
}

template <class V>
comms_status_t run_dev(ExactFir<V>* h, const CxOf<V>* d_in, size_t n, CxOf<V>* d_out, void* stream) {
    constexpr size_t B = sizeof(V);  // bytes per sample
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG((d_in && d_out) || !n, "NULL device pointer");
    COMMS_TRY(use_device(h->device));
    if (!n) return COMMS_OK;
    COMMS_ARG(n <= SIZE_MAX / B / static_cast<size_t>(h->sps), "n * sam_per_sym overflows");
    COMMS_ARG(!ranges_overlap(d_in, n * B, d_out, n * h->sps * B), "the %s FIR cannot run in place", Exact<V>::kNoun);
    COMMS_ARG(((reinterpret_cast<uintptr_t>(d_in) | reinterpret_cast<uintptr_t>(d_out)) & (B - 1)) == 0, "pointers must be aligned to one sample");
    hipStream_t s = nullptr;
    COMMS_TRY(h->enter(stream, &s));
    const size_t n_out = n * static_cast<size_t>(h->sps);
    size_t blocks = (n_out + 255) / 256;
    if (blocks > 8u * kNumCU) blocks = 8u * kNumCU;
    h->tic(s);
    fir_exact_kernel<V><<<dim3(static_cast<unsigned>(blocks)), dim3(256), 0, s>>>(
        reinterpret_cast<const V*>(d_in), h->hist.template cur<V>(), h->hist_len, h->taps.get(), h->n_eff, h->sps,
        reinterpret_cast<V*>(d_out), n, h->hist.template next<V>());
    h->toc(s);
    COMMS_TRY(launch_ok(Exact<V>::kKernel));
    h->hist.flip();
    return COMMS_OK;
}

template <class V>
comms_status_t run_host(ExactFir<V>* h, const CxOf<V>* in, size_t n, CxOf<V>* out) {
    constexpr size_t B = sizeof(V);
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG((in && out) || !n, "NULL host pointer");
    COMMS_TRY(use_device(h->device));
    if (!n) return COMMS_OK;
    return h->run_host_units(in, n * B, B, out, n * h->sps * B, static_cast<size_t>(h->sps) * B, [&](void* d_in, void* d_out, size_t ib, size_t) {
        return run_dev(h, static_cast<const CxOf<V>*>(d_in), ib / B, static_cast<CxOf<V>*>(d_out), COMMS_STREAM_HANDLE);
    });
}

// (both refuse a NULL state outright: the shared rule would take one with an empty read)
template <class V>
comms_status_t get_state(ExactFir<V>* h, CxOf<V>* state, size_t n_state) {
    COMMS_ARG(h && state, "NULL argument");
    return get_history_state(h, state, n_state, "samples");
}

template <class V>
comms_status_t set_state(ExactFir<V>* h, const CxOf<V>* state, size_t n_state) {
    COMMS_ARG(h && state, "NULL argument");
    return set_history_state(h, state, n_state, "samples");
}

}  // namespace

extern "C" {

comms_status_t comms_fir_i16_create(const comms_c16* taps, size_t n_taps, const comms_c16* state, size_t n_state,
                                    int32_t device, comms_fir_i16_t** out) {
    return fir_create<short2>(taps, n_taps, state, n_state, device, out);
}
comms_status_t comms_fir_i16_run(comms_fir_i16_t* h, const comms_c16* in, size_t n, comms_c16* out) { return run_host(h, in, n, out); }
comms_status_t comms_fir_i16_run_dev(comms_fir_i16_t* h, const comms_c16* d_in, size_t n, comms_c16* d_out, void* stream) {
    return run_dev(h, d_in, n, d_out, stream);
}
comms_status_t comms_fir_i16_get_state(comms_fir_i16_t* h, comms_c16* state, size_t n_state) { return get_state(h, state, n_state); }
comms_status_t comms_fir_i16_destroy(comms_fir_i16_t* h) { return destroy_handle(h); }

comms_status_t comms_pulse_i16_create(const comms_c16* taps, size_t n_taps, size_t sam_per_sym, int32_t device,
                                      comms_pulse_i16_t** out) {
    return pulse_create<short2>(taps, n_taps, sam_per_sym, device, out);
}
comms_status_t comms_pulse_i16_run(comms_pulse_i16_t* h, const comms_c16* sym, size_t n_sym, comms_c16* out) {
    return run_host(h, sym, n_sym, out);
}
comms_status_t comms_pulse_i16_run_dev(comms_pulse_i16_t* h, const comms_c16* d_sym, size_t n_sym, comms_c16* d_out, void* stream) {
    return run_dev(h, d_sym, n_sym, d_out, stream);
}
comms_status_t comms_pulse_i16_destroy(comms_pulse_i16_t* h) { return destroy_handle(h); }

comms_status_t comms_fir_f64_create(const comms_c64* taps, size_t n_taps, const comms_c64* state, size_t n_state,
                                    int32_t device, comms_fir_f64_t** out) {
    return fir_create<double2>(taps, n_taps, state, n_state, device, out);
}
comms_status_t comms_fir_f64_run(comms_fir_f64_t* h, const comms_c64* in, size_t n, comms_c64* out) { return run_host(h, in, n, out); }
comms_status_t comms_fir_f64_run_dev(comms_fir_f64_t* h, const comms_c64* d_in, size_t n, comms_c64* d_out, void* stream) {
    return run_dev(h, d_in, n, d_out, stream);
}
comms_status_t comms_fir_f64_get_state(comms_fir_f64_t* h, comms_c64* state, size_t n_state) { return get_state(h, state, n_state); }
comms_status_t comms_fir_f64_set_state(comms_fir_f64_t* h, const comms_c64* state, size_t n_state) { return set_state(h, state, n_state); }
comms_status_t comms_fir_f64_destroy(comms_fir_f64_t* h) { return destroy_handle(h); }

comms_status_t comms_pulse_f64_create(const comms_c64* taps, size_t n_taps, size_t sam_per_sym, int32_t device,
                                      comms_pulse_f64_t** out) {
    return pulse_create<double2>(taps, n_taps, sam_per_sym, device, out);
}
comms_status_t comms_pulse_f64_run(comms_pulse_f64_t* h, const comms_c64* sym, size_t n_sym, comms_c64* out) {
    return run_host(h, sym, n_sym, out);
}
comms_status_t comms_pulse_f64_run_dev(comms_pulse_f64_t* h, const comms_c64* d_sym, size_t n_sym, comms_c64* d_out, void* stream) {
    return run_dev(h, d_sym, n_sym, d_out, stream);
}
comms_status_t comms_pulse_f64_destroy(comms_pulse_f64_t* h) { return destroy_handle(h); }

}  // extern "C"
