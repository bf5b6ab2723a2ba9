// prns.hip -- PrnGen / PrnsNode (src/prns.rs:64-71): a Fibonacci LFSR that emits one bit per step,
//   out = state >> (W-1);  fb = popcount(state & mask) & 1;  state = ((state << 1) | fb) mod 2^W
// for an unsigned register of W = 8, 16, 32 or 64 bits, generated on the device from a jump table.
//
// One step is linear over GF(2): S' = A S, A a W x W matrix whose row 0 is the mask and whose row i is
// bit i-1 (a shift).  Two facts make the kernel cheap:
//   * the next W outputs are the W bits of the current state, most significant first (the register
//     shifts left and the output is its top bit), i.e. the bit-reverse of the state;
//   * A^(2^i) for i < 64 is built once at create time (host, rows as 64-bit words, uploaded once), so the
//     state k steps ahead is at most popcount(k) mat-vecs of W row parities each.
// The kernel is therefore a pure function of (S0, n): lane g of a grid of G = 2^lg lanes jumps to bit
// 64 g, then writes the 64-bit words g, g + G, ... (64 consecutive outputs each, LSB first; consecutive
// lanes -> consecutive words), stepping W bits at a time with A^W and G words at a time with A^(64 G).
// The state itself lives on the host and advances by A^n after every call: get / set / skip are exact for
// any n < 2^64 and never touch the device.
#include "common.hpp"

namespace comms {

constexpr int kPrnsPowers = 64;  // A^(2^i), i < 64

// row-form mat-vec: y_i = parity(row_i & s)
template <int W, class T>
__device__ __forceinline__ T prns_matvec(const uint64_t* __restrict__ rows, T s) {
    T y = 0;
#pragma unroll
    for (int i = 0; i < W; ++i) {
        const int p = W == 64 ? __popcll(rows[i] & s) : __popc(static_cast<unsigned>(rows[i]) & static_cast<unsigned>(s));
        y |= static_cast<T>(p & 1) << i;
    }
    return y;
}

// the next 64 outputs from state s, stream bit t -> word bit t
template <int W, class T>
__device__ __forceinline__ uint64_t prns_word(const uint64_t* __restrict__ pw, T s) {
    if constexpr (W == 64) {
        return __builtin_bitreverse64(s);
    } else {
        constexpr int LW = W == 8 ? 3 : W == 16 ? 4 : 5;
        uint64_t w = 0;
#pragma unroll
        for (int c = 0; c < 64 / W; ++c) {
            w |= static_cast<uint64_t>(__builtin_bitreverse32(static_cast<unsigned>(s)) >> (32 - W)) << (c * W);
            if (c + 1 < 64 / W) s = prns_matvec<W>(pw + LW * 64, s);
        }
        return w;
    }
}

// one output bit per byte (0 / 1): four stream bits -> one dword
__device__ __forceinline__ unsigned prns_spread4(unsigned x) { return ((x & 0xFu) * 0x00204081u) & 0x01010101u; }

template <int W>
__global__ __launch_bounds__(256) void prns_kernel(const uint64_t* __restrict__ pw, uint64_t s0, size_t n,
                                                   uint8_t* __restrict__ out, int packed, int lg) {
    using T = typename std::conditional<W == 64, uint64_t, unsigned>::type;
    const size_t nw = (n + 63) / 64;
    const size_t gid = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
    if (gid >= nw) return;
    T s = static_cast<T>(s0);
    for (int i = 0; i < lg; ++i)  // jump to bit 64 gid: A^(64 * 2^i) for every set bit i of gid
        if ((gid >> i) & 1) s = prns_matvec<W>(pw + (6 + i) * 64, s);
    const size_t G = static_cast<size_t>(1) << lg;
    for (size_t g = gid; g < nw; g += G) {
        uint64_t w = prns_word<W>(pw, s);
        const size_t b0 = g * 64;
        if (b0 + 64 <= n) {
            if (packed) {
                reinterpret_cast<uint64_t*>(out)[g] = w;
            } else {
                uint4* o = reinterpret_cast<uint4*>(out + b0);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const unsigned lo = static_cast<unsigned>(w >> (16 * q)), hi = lo >> 8;
                    o[q] = make_uint4(prns_spread4(lo), prns_spread4(lo >> 4), prns_spread4(hi), prns_spread4(hi >> 4));
                }
            }
        } else {  // the stream's last, partial word: bits past n are not written (u8) / written as 0 (packed)
            const unsigned rem = static_cast<unsigned>(n - b0);
            w &= (1ull << rem) - 1;
            if (packed) {
                for (unsigned b = 0; b < (rem + 7) / 8; ++b) out[g * 8 + b] = static_cast<uint8_t>(w >> (8 * b));
            } else {
                for (unsigned b = 0; b < rem; ++b) out[b0 + b] = static_cast<uint8_t>((w >> b) & 1);
            }
        }
        if (g + G < nw) s = prns_matvec<W>(pw + (6 + lg) * 64, s);
    }
}

// ---- host side of the GF(2) algebra (rows as 64-bit words, W <= 64)
inline int parity64(uint64_t x) { return __builtin_parityll(x); }
inline uint64_t host_matvec(const uint64_t* rows, int W, uint64_t s) {
    uint64_t y = 0;
    for (int i = 0; i < W; ++i) y |= static_cast<uint64_t>(parity64(rows[i] & s)) << i;
    return y;
}
// Z = X Y: row i of Z = XOR of the rows j of Y for which X_ij = 1
inline void host_matmul(const uint64_t* X, const uint64_t* Y, int W, uint64_t* Z) {
    for (int i = 0; i < W; ++i) {
        uint64_t r = 0;
        for (int j = 0; j < W; ++j)
            if ((X[i] >> j) & 1) r ^= Y[j];
        Z[i] = r;
    }
}

}  // namespace comms

using namespace comms;

struct comms_prns : Handle {
    int W = 8;
    uint64_t mask = 0, state = 0;
    uint64_t pw[kPrnsPowers][64] = {};  // A^(2^i), rows (host copy)
    DevBuf<uint64_t> d_pw;              // the same table on the device
    void advance(uint64_t n) {
        for (int i = 0; i < kPrnsPowers; ++i)
            if ((n >> i) & 1) state = host_matvec(pw[i], W, state);
    }
};

static_assert(!std::is_copy_constructible_v<comms_prns>, "a handle is never copied");

static uint64_t width_mask(int W) { return W == 64 ? ~0ull : (1ull << W) - 1; }

extern "C" {

comms_status_t comms_prns_create(uint64_t poly_mask, uint64_t state, int32_t width_bits, int32_t device, comms_prns_t** out) {
    COMMS_ARG(out != nullptr, "out is NULL");
    *out = nullptr;
    COMMS_ARG(width_bits == 8 || width_bits == 16 || width_bits == 32 || width_bits == 64,
              "the register is 8, 16, 32 or 64 bits wide (got %d; signed types panic in the reference)", width_bits);
    COMMS_ARG((poly_mask & ~width_mask(width_bits)) == 0, "poly_mask does not fit %d bits", width_bits);
    COMMS_ARG((state & ~width_mask(width_bits)) == 0, "state does not fit %d bits", width_bits);
    HandlePtr<comms_prns> h;
    COMMS_TRY(make_handle(device, &h));
    const int W = width_bits;
    h->W = W;
    h->mask = poly_mask;
    h->state = state;
    h->pw[0][0] = poly_mask;
    for (int i = 1; i < W; ++i) h->pw[0][i] = 1ull << (i - 1);
    for (int k = 1; k < kPrnsPowers; ++k) host_matmul(h->pw[k - 1], h->pw[k - 1], W, h->pw[k]);
    COMMS_HIP_TRY(h->d_pw.upload(&h->pw[0][0], kPrnsPowers * 64));
    *out = h.release();
    return COMMS_OK;
}

comms_status_t comms_prns_run_dev(comms_prns_t* h, size_t n, int32_t format, uint8_t* d_out, void* stream) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG(format == COMMS_BITS_U8 || format == COMMS_BITS_PACKED, "format must be COMMS_BITS_U8 or COMMS_BITS_PACKED (got %d)", format);
    COMMS_ARG(d_out != nullptr || !n, "NULL device pointer");
    COMMS_ARG((reinterpret_cast<uintptr_t>(d_out) & 15) == 0, "d_out must be 16-byte aligned");
    COMMS_TRY(use_device(h->device));
    if (!n) return COMMS_OK;
    hipStream_t s = nullptr;
    COMMS_TRY(h->enter(stream, &s));
    const size_t nw = (n + 63) / 64;
    size_t want = (nw + 255) / 256;
    int lb = 0;  // blocks = 2^lb: a power-of-two grid, so that one grid sweep is one table entry
    while ((size_t{1} << lb) < want && lb < 10) ++lb;  // at most 1024 workgroups (4 per CU)
    const int lg = lb + 8;
    const int packed = format == COMMS_BITS_PACKED;
    h->tic(s);
#define COMMS_PRNS_GO(W) prns_kernel<W><<<dim3(1u << lb), dim3(256), 0, s>>>(h->d_pw.get(), h->state, n, d_out, packed, lg)
    switch (h->W) {
        case 8: COMMS_PRNS_GO(8); break;
        case 16: COMMS_PRNS_GO(16); break;
        case 32: COMMS_PRNS_GO(32); break;
        default: COMMS_PRNS_GO(64); break;
    }
#undef COMMS_PRNS_GO
    h->toc(s);
    COMMS_TRY(launch_ok("prns_kernel"));
    h->advance(n);
    return COMMS_OK;
}

comms_status_t comms_prns_run(comms_prns_t* h, size_t n, int32_t format, uint8_t* out) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG(format == COMMS_BITS_U8 || format == COMMS_BITS_PACKED, "format must be COMMS_BITS_U8 or COMMS_BITS_PACKED (got %d)", format);
    COMMS_ARG(out != nullptr || !n, "NULL host pointer");
    COMMS_TRY(use_device(h->device));
    if (!n) return COMMS_OK;
    const size_t bytes = format == COMMS_BITS_U8 ? n : (n + 7) / 8;
    COMMS_TRY(h->out_scratch.reserve(bytes));
    COMMS_TRY(comms_prns_run_dev(h, n, format, static_cast<uint8_t*>(h->out_scratch.p), COMMS_STREAM_HANDLE));
    COMMS_HIP_TRY(hipMemcpyAsync(out, h->out_scratch.p, bytes, hipMemcpyDeviceToHost, h->stream));
    COMMS_HIP_TRY(hipStreamSynchronize(h->stream));
    return COMMS_OK;
}

comms_status_t comms_prns_get_state(const comms_prns_t* h, uint64_t* state) {
    COMMS_ARG(h && state, "NULL argument");
    *state = h->state;
    return COMMS_OK;
}

comms_status_t comms_prns_set_state(comms_prns_t* h, uint64_t state) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG((state & ~width_mask(h->W)) == 0, "state does not fit %d bits", h->W);
    h->state = state;
    return COMMS_OK;
}

comms_status_t comms_prns_skip(comms_prns_t* h, uint64_t n_bits) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    h->advance(n_bits);
    return COMMS_OK;
}

comms_status_t comms_prns_set_timer(comms_prns_t* h, comms_timer_t* t) { return set_handle_timer(h, t); }

comms_status_t comms_prns_destroy(comms_prns_t* h) { return destroy_handle(h); }

}  // extern "C"
