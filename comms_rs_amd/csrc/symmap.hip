// symmap.hip -- the constellation stages of a coded link with up to 8 bits per symbol: packed bits -> frames of Complex<f32>
// symbols behind a known word (symmap_kernel), and Complex<f32> symbol records -> hard bits or max-log LLRs (demap_*_kernel),
// every frame of a call by ONE launch each.  Both nodes are stateless.
//
// The reference has no such block; the contract is include/comms_hip.h's ("symbol mapper and soft demapper"), and
// tests/symmap_ref.py restates its brute-force definition.  The decision rule is comms_sym_to_bits's over 2^m points.
//   symmap_kernel        one lane per output symbol of the flattened (frame, position) space: the word, the payload, the gap.
//                        A payload lane takes its m-bit field from the one or two 32-bit words it touches (no byte loads), masks
//                        the bits beyond E, reads the point from the table in LDS (2^m * 8 B, divergent indices) and issues
//                        one 8-byte store; consecutive lanes store consecutive symbols.
//   demap_table_kernel   any table.  A lane owns a symbol; the 2^m points are read at wave-uniform addresses (scalar loads) in a
//                        fully unrolled loop, so "bit b of i" is a constant: a point costs its distance and m minimum updates
//                        (LLR) or one compare and two selects (BITS).
//   demap_axis_kernel    a separable table, c[v] = (pI[v & (2^mI - 1)], pQ[v >> mI]): 2^mI + 2^mQ squared differences in place
//                        of 2^m distances.  f32 addition is monotone in each operand, so the minimum of fl(a_i + b_j) over a
//                        product set is fl(min a_i + min b_j) -- the definition's value bit for bit.  The hard decision is NOT
//                        the per-axis argmin (two different sums can round to the same float): with D = fl(a_min + b_min) it
//                        is the lowest j with fl(a_min + b_j) == D, then the lowest i with fl(a_i + b_j*) == D.
//   minima               with a finite table a distance is NaN for one point only if it is NaN for all of them, so the
//                        definition's strict-replace scan equals an IEEE minimum (fminf); every minimum starts from the first
//                        point of its class, not from +inf, so that a NaN symbol gives NaN values.
//   weighted LLRs        comms_demap_run_weighted: both forms again with FMT = SM_LLR_WEIGHTED.  A lane loads its symbol's weight
//                        w (4 bytes beside the symbol's 8), multiplies by c = fl(scale * w) where the plain form multiplies by
//                        scale, and writes +0.0 for a weight that is not finite and positive.  (frame, position) are carried
//                        from pass to pass, one 64-bit division per lane; P = F and P = 1 need no position at all.
//   LLR stores           a lane writes its symbol's 4 m bytes directly: 16-byte stores at m = 4 and 8, 8-byte stores at m = 2
//                        and 6, 4-byte stores at odd m.
//   BITS words           a wave takes 64 consecutive symbols of ONE frame, which are exactly 2 m whole 32-bit words of its
//                        record, so no word is shared between waves or frames.  Where m divides 32 the 32 / m lanes of a word
//                        OR their fields together by cross-lane swaps; otherwise lane k < 2 m gathers word k from the lanes
//                        whose fields touch it (at most ceil(32 / m) + 1 shuffles), shifting each into place.  Every word is
//                        written once; the lanes past F contribute zero bits, which is the record's padding.
// All kernels walk their items grid-stride under the library's grid cap.
#include <cmath>

#include "common.hpp"

namespace comms {

constexpr int SM_WG = 256;
constexpr int SM_MAX_BITS = 8;
constexpr size_t SM_MAX_E = size_t(1) << 20;      // bits per mapper record
constexpr size_t SM_MAX_F = size_t(1) << 20;      // symbols per demapper record
constexpr size_t SM_MAX_WORD = 512;
constexpr size_t SM_MAX_GAP = size_t(1) << 16;
constexpr size_t SM_TABLE_LDS = (size_t(1) << SM_MAX_BITS) * sizeof(float2);

// ---- mapper --------------------------------------------------------------------------------------------------------------
struct MapArgs {
    const unsigned* bits;   // records of in_words words
    float2* out;            // records of rec symbols
    const float2* table;    // 2^m points
    const float2* word;     // P symbols (never read when P = 0)
    size_t total;           // n_frames * rec
    unsigned in_words, E, m, P, F, rec;
};

__global__ __launch_bounds__(SM_WG) void symmap_kernel(const MapArgs a) {
    __shared__ float2 tab[1 << SM_MAX_BITS];
    for (unsigned i = threadIdx.x; i < (1u << a.m); i += SM_WG) tab[i] = a.table[i];
    __syncthreads();
    const unsigned stride = gridDim.x * SM_WG;
    const size_t l0 = static_cast<size_t>(blockIdx.x) * SM_WG + threadIdx.x;
    if (l0 >= a.total) return;
    const unsigned dq = stride / a.rec, dr = stride % a.rec;
    size_t frame = l0 / a.rec;
    unsigned pos = static_cast<unsigned>(l0 % a.rec);
    const unsigned vmask = (1u << a.m) - 1u;
    for (size_t l = l0; l < a.total; l += stride) {
        float2 y = make_float2(0.f, 0.f);
        if (pos < a.P) {
            y = a.word[pos];
        } else if (pos < a.P + a.F) {
            const unsigned* rec = a.bits + frame * a.in_words;
            const unsigned o = (pos - a.P) * a.m, w = o >> 5, s = o & 31u;   // o < E
            unsigned v = rec[w] >> s;
            if (s + a.m > 32u && w + 1u < a.in_words) v |= rec[w + 1u] << (32u - s);   // (s > 0 here)
            v &= vmask;
            const unsigned left = a.E - o;                                    // the bits of the record from o on: >= 1
            if (left < a.m) v &= (1u << left) - 1u;
            y = tab[v];
        }
        a.out[l] = y;
        frame += dq;
        pos += dr;
        if (pos >= a.rec) {
            pos -= a.rec;
            ++frame;
        }
    }
}

// ---- demapper ------------------------------------------------------------------------------------------------------------
struct DemapArgs {
    const float2* sym;      // n_frames records of F symbols: a flat stream
    void* out;
    const float2* table;    // 2^m points (table form)
    const float* pI;        // 2^mI real levels, then 2^mQ imaginary levels at pQ (per-axis form)
    const float* pQ;
    size_t n_frames;
    size_t items;           // LLR: symbols of the call; BITS: waves' worth of work, n_frames * chunks
    unsigned F, chunks;     // BITS: chunks = ceil(F / 64) per frame
    unsigned rec_words;     // BITS: 32-bit words per output record
    float scale;
    const float* weight;    // weighted LLR: n_frames records of P floats, symbol j of a frame takes weight[j mod P]
    unsigned P;
};
constexpr int SM_LLR_WEIGHTED = -1;   // the kernels' FMT of comms_demap_run_weighted: COMMS_SYM_LLR with a weight per symbol

__device__ __forceinline__ float sq_diff(float z, float p) {
    const float d = __fsub_rn(z, p);
    return __fmul_rn(d, d);
}

// LLRs of one symbol, table form: L[b] = s * (D1_b - D0_b)
template <int M>
__device__ __forceinline__ void llr_table(float2 z, const float2* __restrict__ tab, float s, float (&L)[M]) {
    float d0[M], d1[M];
#pragma unroll
    for (int i = 0; i < (1 << M); ++i) {
        const float d = sym_dist(z, tab[i]);
#pragma unroll
        for (int b = 0; b < M; ++b) {
            if ((i >> b) & 1)
                d1[b] = i == (1 << b) ? d : __builtin_fminf(d1[b], d);   // (1 << b is the first index with bit b set)
            else
                d0[b] = i == 0 ? d : __builtin_fminf(d0[b], d);
        }
    }
#pragma unroll
    for (int b = 0; b < M; ++b) L[b] = __fmul_rn(s, __fsub_rn(d1[b], d0[b]));
}

template <int M>
__device__ __forceinline__ unsigned decide_table(float2 z, const float2* __restrict__ tab) {
    unsigned v = 0;
    float best = sym_dist(z, tab[0]);
#pragma unroll
    for (int i = 1; i < (1 << M); ++i) {
        const float d = sym_dist(z, tab[i]);
        if (d < best) {
            best = d;
            v = static_cast<unsigned>(i);
        }
    }
    return v;
}

// One axis: the minimum of (z - p_i)^2 over all levels and over the levels whose index bit b is 0 / 1
template <int MB>
__device__ __forceinline__ void axis_minima(float z, const float* __restrict__ p, float& all, float* m0, float* m1) {
#pragma unroll
    for (int i = 0; i < (1 << MB); ++i) {
        const float a = sq_diff(z, p[i]);
        all = i == 0 ? a : __builtin_fminf(all, a);
#pragma unroll
        for (int b = 0; b < MB; ++b) {
            if ((i >> b) & 1)
                m1[b] = i == (1 << b) ? a : __builtin_fminf(m1[b], a);
            else
                m0[b] = i == 0 ? a : __builtin_fminf(m0[b], a);
        }
    }
}

template <int MI, int MQ>
__device__ __forceinline__ void llr_axis(float2 z, const float* __restrict__ pI, const float* __restrict__ pQ, float s,
                                         float (&L)[MI + MQ]) {
    float amin = 0.f, bmin = 0.f;
    float a0[MI + 1], a1[MI + 1], b0[MQ + 1], b1[MQ + 1];   // (+ 1: no zero-length arrays)
    axis_minima<MI>(z.x, pI, amin, a0, a1);
    axis_minima<MQ>(z.y, pQ, bmin, b0, b1);
#pragma unroll
    for (int b = 0; b < MI; ++b) L[b] = __fmul_rn(s, __fsub_rn(__fadd_rn(a1[b], bmin), __fadd_rn(a0[b], bmin)));
#pragma unroll
    for (int b = 0; b < MQ; ++b) L[MI + b] = __fmul_rn(s, __fsub_rn(__fadd_rn(amin, b1[b]), __fadd_rn(amin, b0[b])));
}

template <int MI, int MQ>
__device__ __forceinline__ unsigned decide_axis(float2 z, const float* __restrict__ pI, const float* __restrict__ pQ) {
    float amin = 0.f, bmin = 0.f;
#pragma unroll
    for (int i = 0; i < (1 << MI); ++i) {
        const float a = sq_diff(z.x, pI[i]);
        amin = i == 0 ? a : __builtin_fminf(amin, a);
    }
#pragma unroll
    for (int j = 0; j < (1 << MQ); ++j) {
        const float b = sq_diff(z.y, pQ[j]);
        bmin = j == 0 ? b : __builtin_fminf(bmin, b);
    }
    const float D = __fadd_rn(amin, bmin);
    // descending scans, so that the lowest index that reaches D is the one kept; a NaN D matches nothing: v = 0
    unsigned js = 0;
    float bs = 0.f;
#pragma unroll
    for (int j = (1 << MQ) - 1; j >= 0; --j) {
        const float b = sq_diff(z.y, pQ[j]);
        if (__fadd_rn(amin, b) == D) {
            js = static_cast<unsigned>(j);
            bs = b;
        }
    }
    unsigned is = 0;
#pragma unroll
    for (int i = (1 << MI) - 1; i >= 0; --i) {
        const float a = sq_diff(z.x, pI[i]);
        if (__fadd_rn(a, bs) == D) is = static_cast<unsigned>(i);
    }
    return D == D ? is | (js << MI) : 0u;
}

// a symbol's M LLRs at out + M * at: the widest stores the alignment of 4 M bytes allows
template <int M>
__device__ __forceinline__ void llr_store(float* out, size_t at, const float (&L)[M]) {
    float* p = out + static_cast<size_t>(M) * at;
    if constexpr (M % 4 == 0) {
#pragma unroll
        for (int b = 0; b < M; b += 4) *reinterpret_cast<float4*>(p + b) = make_float4(L[b], L[b + 1], L[b + 2], L[b + 3]);
    } else if constexpr (M % 2 == 0) {
#pragma unroll
        for (int b = 0; b < M; b += 2) *reinterpret_cast<float2*>(p + b) = make_float2(L[b], L[b + 1]);
    } else {
#pragma unroll
        for (int b = 0; b < M; ++b) p[b] = L[b];
    }
}

// The 2 M words of a wave's 64 symbols (lane l holds symbol l's M-bit value, 0 past the frame's end): word k in lane
// `word_lane(k)`; returns this lane's word and whether it holds one (k = its index among the 2 M)
template <int M>
__device__ __forceinline__ bool wave_words(unsigned v, unsigned lane, unsigned& word, unsigned& k) {
    if constexpr (32 % M == 0) {
        constexpr int G = 32 / M;
        word = bits_gather<G>(v << (M * (lane % G)));
        k = lane / G;
        return lane % G == 0;
    } else {
        constexpr int T = (32 + M - 1) / M + 1;   // fields that can touch one word
        k = lane;
        const int first = static_cast<int>(32u * lane) / M;   // the symbol that holds the word's bit 0 (lanes >= 2 M: unused)
        unsigned w = 0;
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int src = first + t;
            const unsigned u = static_cast<unsigned>(__shfl(static_cast<int>(v), src & 63));
            const int sh = src * M - 32 * static_cast<int>(lane);   // >= -(M - 1)
            if (src < 64 && sh < 32 && sh > -32) w |= sh >= 0 ? u << sh : u >> -sh;
        }
        word = w;
        return lane < 2u * M;
    }
}

// FORM 0: the table form (M = MI, MQ unused); FORM 1: the per-axis form (M = MI + MQ)
template <int FORM, int MI, int MQ>
__device__ __forceinline__ void demap_llr_one(const DemapArgs& a, size_t at, float scale, bool erase) {
    constexpr int M = FORM ? MI + MQ : MI;
    const float2 z = a.sym[at];
    float L[M];
    if constexpr (FORM)
        llr_axis<MI, MQ>(z, a.pI, a.pQ, scale, L);
    else
        llr_table<M>(z, a.table, scale, L);
    if (erase) {
#pragma unroll
        for (int b = 0; b < M; ++b) L[b] = 0.f;
    }
    llr_store<M>(static_cast<float*>(a.out), at, L);
}

template <int FORM, int MI, int MQ>
__device__ __forceinline__ void demap_llr_items(const DemapArgs& a) {
    const size_t stride = static_cast<size_t>(gridDim.x) * SM_WG;
    for (size_t at = static_cast<size_t>(blockIdx.x) * SM_WG + threadIdx.x; at < a.items; at += stride)
        demap_llr_one<FORM, MI, MQ>(a, at, a.scale, false);
}

// The weighted form: symbol `at` = frame * F + pos takes w = weight[frame * P + pos mod P] and c = fl(scale * w) in place of
// the scale; a weight that is not finite and positive erases the symbol (every LLR +0.0, whatever the symbol is).  P = F
// reads weight[at] and P = 1 weight[frame]; only the periods between need pos mod P (32-bit).  A lane divides once, by F,
// in front of its loop, and carries (frame, pos) from pass to pass as symmap_kernel does.
template <int FORM, int MI, int MQ>
__device__ __forceinline__ void demap_weighted_items(const DemapArgs& a) {
    const unsigned stride = gridDim.x * SM_WG;
    const size_t l0 = static_cast<size_t>(blockIdx.x) * SM_WG + threadIdx.x;
    if (l0 >= a.items) return;
    const unsigned dq = stride / a.F, dr = stride % a.F;
    size_t frame = l0 / a.F;
    unsigned pos = static_cast<unsigned>(l0 % a.F);
    for (size_t at = l0; at < a.items; at += stride) {
        const size_t wi = a.P == a.F ? at : a.P == 1u ? frame : frame * a.P + pos % a.P;
        const float w = a.weight[wi];
        const bool ok = w > 0.f && w <= 3.402823466e38f;   // (false for NaN)
        demap_llr_one<FORM, MI, MQ>(a, at, __fmul_rn(a.scale, w), !ok);
        frame += dq;
        pos += dr;
        if (pos >= a.F) {
            pos -= a.F;
            ++frame;
        }
    }
}

template <int FORM, int MI, int MQ>
__device__ __forceinline__ void demap_bits_items(const DemapArgs& a) {
    constexpr int M = FORM ? MI + MQ : MI;
    const unsigned lane = threadIdx.x & 63u;
    const size_t n_waves = static_cast<size_t>(gridDim.x) * (SM_WG / 64);
    // `it` is wave-uniform: every lane of a wave takes part in the swaps
    for (size_t it = static_cast<size_t>(blockIdx.x) * (SM_WG / 64) + threadIdx.x / 64u; it < a.items; it += n_waves) {
        const size_t frame = it / a.chunks;
        const unsigned chunk = static_cast<unsigned>(it % a.chunks);
        const unsigned pos = chunk * 64u + lane;
        unsigned v = 0;
        if (pos < a.F) {
            const float2 z = a.sym[frame * a.F + pos];
            if constexpr (FORM)
                v = decide_axis<MI, MQ>(z, a.pI, a.pQ);
            else
                v = decide_table<M>(z, a.table);
        }
        unsigned word, k;
        const bool mine = wave_words<M>(v, lane, word, k);
        const unsigned w = chunk * (2u * M) + k;
        if (mine && w < a.rec_words) static_cast<unsigned*>(a.out)[frame * a.rec_words + w] = word;
    }
}

template <int M, int FMT>
__global__ __launch_bounds__(SM_WG) void demap_table_kernel(const DemapArgs a) {
    if constexpr (FMT == COMMS_SYM_BITS)
        demap_bits_items<0, M, 0>(a);
    else if constexpr (FMT == SM_LLR_WEIGHTED)
        demap_weighted_items<0, M, 0>(a);
    else
        demap_llr_items<0, M, 0>(a);
}

template <int MI, int MQ, int FMT>
__global__ __launch_bounds__(SM_WG) void demap_axis_kernel(const DemapArgs a) {
    if constexpr (FMT == COMMS_SYM_BITS)
        demap_bits_items<1, MI, MQ>(a);
    else if constexpr (FMT == SM_LLR_WEIGHTED)
        demap_weighted_items<1, MI, MQ>(a);
    else
        demap_llr_items<1, MI, MQ>(a);
}

}  // namespace comms

using namespace comms;

struct comms_symmap : Handle {
    unsigned m = 0, E = 0, P = 0, F = 0, G = 0;
    DevBuf<float2> table, word;
    unsigned max_grid = 1;
};
struct comms_demap : Handle {
    unsigned m = 0, F = 0;
    int mI = -1, mQ = 0;       // the per-axis split, mI < 0: the table form
    int format = COMMS_SYM_LLR;
    float scale = 1.0f;
    DevBuf<float2> table;
    DevBuf<float> levels;      // pI then pQ
    unsigned max_grid = 1;
};
static_assert(!std::is_copy_constructible_v<comms_symmap> && !std::is_copy_constructible_v<comms_demap>, "a handle is never copied");

namespace {

const comms_c32 kBpsk[2] = {{1.f, 0.f}, {-1.f, 0.f}};
const comms_c32 kQpsk[4] = {{1.f, 1.f}, {-1.f, 1.f}, {1.f, -1.f}, {-1.f, -1.f}};

// the 2^m points of a create: the caller's, or digital.rs's for m <= 2; all finite
comms_status_t take_table(int32_t m, const comms_c32* constellation, std::vector<float2>* out) {
    COMMS_ARG(m >= 1 && m <= SM_MAX_BITS, "bits_per_sym must be 1 ... %d (got %d)", SM_MAX_BITS, m);
    COMMS_ARG(constellation || m <= 2, "a NULL constellation means digital.rs's tables: bits_per_sym 1 or 2 only (got %d)", m);
    const comms_c32* c = constellation ? constellation : m == 1 ? kBpsk : kQpsk;
    out->resize(size_t(1) << m);
    for (size_t v = 0; v < out->size(); ++v) {
        COMMS_ARG(std::isfinite(c[v].re) && std::isfinite(c[v].im), "constellation point %zu is not finite", v);
        (*out)[v] = make_float2(c[v].re, c[v].im);
    }
    return COMMS_OK;
}

// The separable split of a table with the fewest levels, or mI = -1.  Floats compare exactly.
void find_split(const std::vector<float2>& c, int m, int* mI, std::vector<float>* levels) {
    *mI = -1;
    size_t best = 0;
    for (int k = 0; k <= m; ++k) {
        const size_t nI = size_t(1) << k, nQ = size_t(1) << (m - k);
        bool ok = true;
        for (size_t v = 0; v < c.size() && ok; ++v) ok = c[v].x == c[v & (nI - 1)].x && c[v].y == c[(v >> k) << k].y;
        if (ok && (*mI < 0 || nI + nQ < best)) {
            *mI = k;
            best = nI + nQ;
        }
    }
    if (*mI < 0) return;
    const size_t nI = size_t(1) << *mI, nQ = c.size() >> *mI;
    levels->resize(nI + nQ);
    for (size_t i = 0; i < nI; ++i) (*levels)[i] = c[i].x;
    for (size_t j = 0; j < nQ; ++j) (*levels)[nI + j] = c[j << *mI].y;
}

size_t map_in_bytes(const comms_symmap* h) { return bit_record_bytes(h->E); }
size_t map_rec(const comms_symmap* h) { return static_cast<size_t>(h->P) + h->F + h->G; }
size_t map_grid(const comms_symmap* h, size_t n_frames) { return capped_grid((n_frames * map_rec(h) + SM_WG - 1) / SM_WG, h->max_grid); }
FrameCall map_call(const comms_symmap* h) { return {map_in_bytes(h), map_rec(h) * sizeof(comms_c32), 4, 8, (size_t(1) << 40) / map_rec(h)}; }

size_t demap_out_bytes(const comms_demap* h) {
    const size_t bits = static_cast<size_t>(h->F) * h->m;
    return h->format == COMMS_SYM_BITS ? bit_record_bytes(bits) : bits * sizeof(float);
}
size_t demap_chunks(const comms_demap* h) { return (static_cast<size_t>(h->F) + 63) / 64; }
// items of a call: symbols (LLR) or waves' worth of 64 symbols of one frame (BITS)
size_t demap_items(const comms_demap* h, size_t n_frames) {
    return h->format == COMMS_SYM_BITS ? n_frames * demap_chunks(h) : n_frames * h->F;
}
size_t demap_grid(const comms_demap* h, size_t n_frames) {
    const size_t per = h->format == COMMS_SYM_BITS ? SM_WG / 64 : SM_WG;
    return capped_grid((demap_items(h, n_frames) + per - 1) / per, h->max_grid);
}
FrameCall demap_call(const comms_demap* h) { return {h->F * sizeof(comms_c32), demap_out_bytes(h), 8, 16, (size_t(1) << 40) / h->F}; }

template <int M, int FMT>
comms_status_t demap_launch_table(comms_demap* h, const DemapArgs& a, dim3 grid, hipStream_t s) {
    return launch_kernel<demap_table_kernel<M, FMT>>("demap_table_kernel", grid, dim3(SM_WG), 0, s, h->take_events(), a);
}
template <int MI, int MQ, int FMT>
comms_status_t demap_launch_axis(comms_demap* h, const DemapArgs& a, dim3 grid, hipStream_t s) {
    if constexpr (MI + MQ >= 1 && MI + MQ <= SM_MAX_BITS)
        return launch_kernel<demap_axis_kernel<MI, MQ, FMT>>("demap_axis_kernel", grid, dim3(SM_WG), 0, s, h->take_events(), a);
    else
        return fail(COMMS_ERR_ARG, "no per-axis kernel for the split %d + %d", MI, MQ);
}
template <int MI, int FMT>
comms_status_t demap_pick_q(comms_demap* h, const DemapArgs& a, dim3 grid, hipStream_t s) {
    switch (h->mQ) {
        case 0: return demap_launch_axis<MI, 0, FMT>(h, a, grid, s);
        case 1: return demap_launch_axis<MI, 1, FMT>(h, a, grid, s);
        case 2: return demap_launch_axis<MI, 2, FMT>(h, a, grid, s);
        case 3: return demap_launch_axis<MI, 3, FMT>(h, a, grid, s);
        case 4: return demap_launch_axis<MI, 4, FMT>(h, a, grid, s);
        case 5: return demap_launch_axis<MI, 5, FMT>(h, a, grid, s);
        case 6: return demap_launch_axis<MI, 6, FMT>(h, a, grid, s);
        case 7: return demap_launch_axis<MI, 7, FMT>(h, a, grid, s);
        default: return demap_launch_axis<MI, 8, FMT>(h, a, grid, s);
    }
}
template <int FMT>
comms_status_t demap_launch(comms_demap* h, const DemapArgs& a, dim3 grid, hipStream_t s) {
    if (h->mI < 0) {
        switch (h->m) {
            case 1: return demap_launch_table<1, FMT>(h, a, grid, s);
            case 2: return demap_launch_table<2, FMT>(h, a, grid, s);
            case 3: return demap_launch_table<3, FMT>(h, a, grid, s);
            case 4: return demap_launch_table<4, FMT>(h, a, grid, s);
            case 5: return demap_launch_table<5, FMT>(h, a, grid, s);
            case 6: return demap_launch_table<6, FMT>(h, a, grid, s);
            case 7: return demap_launch_table<7, FMT>(h, a, grid, s);
            default: return demap_launch_table<8, FMT>(h, a, grid, s);
        }
    }
    switch (h->mI) {
        case 0: return demap_pick_q<0, FMT>(h, a, grid, s);
        case 1: return demap_pick_q<1, FMT>(h, a, grid, s);
        case 2: return demap_pick_q<2, FMT>(h, a, grid, s);
        case 3: return demap_pick_q<3, FMT>(h, a, grid, s);
        case 4: return demap_pick_q<4, FMT>(h, a, grid, s);
        case 5: return demap_pick_q<5, FMT>(h, a, grid, s);
        case 6: return demap_pick_q<6, FMT>(h, a, grid, s);
        case 7: return demap_pick_q<7, FMT>(h, a, grid, s);
        default: return demap_pick_q<8, FMT>(h, a, grid, s);
    }
}

// cos and sin of t sixteenths of a turn from first-octant values, so that the points of a PSK table are exactly symmetric
double cos16(int t) {
    static const double c[5] = {1.0, 0.92387953251128674, 0.70710678118654757, 0.38268343236508977, 0.0};
    t &= 15;
    if (t > 8) t = 16 - t;
    return t > 4 ? -c[8 - t] : c[t];
}
double sin16(int t) { return cos16(t - 4); }

unsigned gray_rank(unsigned g) {
    unsigned r = 0;
    for (; g; g >>= 1) r ^= g;
    return r;
}

}  // namespace

extern "C" {

comms_status_t comms_constellation_qam(int32_t bits_per_sym, double scale, comms_c32* out) {
    COMMS_ARG(out != nullptr, "out is NULL");
    COMMS_ARG(bits_per_sym == 1 || (bits_per_sym >= 2 && bits_per_sym <= SM_MAX_BITS && bits_per_sym % 2 == 0),
              "a QAM table has bits_per_sym 1, 2, 4, 6 or 8 (got %d)", bits_per_sym);
    COMMS_ARG(std::isfinite(scale), "scale must be finite");
    const unsigned k = bits_per_sym == 1 ? 1u : static_cast<unsigned>(bits_per_sym) / 2u, top = (1u << k) - 1u;
    for (unsigned v = 0; v < (1u << bits_per_sym); ++v) {
        const double re = (static_cast<double>(top) - 2.0 * gray_rank(v & top)) * scale;
        const double im = bits_per_sym == 1 ? 0.0 : (static_cast<double>(top) - 2.0 * gray_rank(v >> k)) * scale;
        out[v].re = static_cast<float>(re);
        out[v].im = static_cast<float>(im);
    }
    return COMMS_OK;
}

comms_status_t comms_constellation_psk(int32_t bits_per_sym, double scale, comms_c32* out) {
    COMMS_ARG(out != nullptr, "out is NULL");
    COMMS_ARG(bits_per_sym >= 1 && bits_per_sym <= 4, "a PSK table has bits_per_sym 1 ... 4 (got %d)", bits_per_sym);
    COMMS_ARG(std::isfinite(scale), "scale must be finite");
    const int step = 16 >> bits_per_sym, phi = bits_per_sym == 2 ? 2 : 0;   // in sixteenths of a turn
    for (unsigned v = 0; v < (1u << bits_per_sym); ++v) {
        const int t = static_cast<int>(gray_rank(v)) * step + phi;
        out[v].re = static_cast<float>(scale * cos16(t));
        out[v].im = static_cast<float>(scale * sin16(t));
    }
    return COMMS_OK;
}

// ---- mapper
comms_status_t comms_symmap_create(int32_t bits_per_sym, const comms_c32* constellation, size_t n_bits, const comms_c32* word, size_t n_word,
                                   size_t gap, int32_t device, comms_symmap_t** out) {
    COMMS_ARG(out != nullptr, "out is NULL");
    *out = nullptr;
    std::vector<float2> table;
    COMMS_TRY(take_table(bits_per_sym, constellation, &table));
    COMMS_ARG(n_bits >= 1 && n_bits <= SM_MAX_E, "a record has 1 <= n_bits <= 2^20 bits (got %zu)", n_bits);
    COMMS_ARG(n_word <= SM_MAX_WORD, "the word has at most %zu symbols (got %zu)", SM_MAX_WORD, n_word);
    COMMS_ARG(word || !n_word, "word is NULL with n_word > 0");
    COMMS_ARG(gap <= SM_MAX_GAP, "the gap has at most 2^16 symbols (got %zu)", gap);
    HandlePtr<comms_symmap> h;
    COMMS_TRY(make_handle(device, &h));
    h->m = static_cast<unsigned>(bits_per_sym);
    h->E = static_cast<unsigned>(n_bits);
    h->P = static_cast<unsigned>(n_word);
    h->F = static_cast<unsigned>((n_bits + h->m - 1) / h->m);
    h->G = static_cast<unsigned>(gap);
    COMMS_HIP_TRY(h->table.upload(table));
    if (n_word) COMMS_HIP_TRY(h->word.upload(reinterpret_cast<const float2*>(word), n_word));
    h->max_grid = resident_workgroups(SM_TABLE_LDS);
    *out = h.release();
    return COMMS_OK;
}

size_t comms_symmap_in_frame_bytes(const comms_symmap_t* h) { return h ? map_in_bytes(h) : 0; }
size_t comms_symmap_out_frame_syms(const comms_symmap_t* h) { return h ? map_rec(h) : 0; }

comms_status_t comms_symmap_run_dev(comms_symmap_t* h, const void* d_bits, size_t n_frames, comms_c32* d_out, void* stream) {
    COMMS_TRY(check_frame_call(h, map_call, d_bits, n_frames, d_out, true));
    if (!n_frames) return COMMS_OK;
    COMMS_TRY(use_device(h->device));
    MapArgs a{};
    a.bits = static_cast<const unsigned*>(d_bits);
    a.out = reinterpret_cast<float2*>(d_out);
    a.table = h->table.get();
    a.word = h->word.get();
    a.total = n_frames * map_rec(h);
    a.in_words = static_cast<unsigned>(map_in_bytes(h) / 4);
    a.E = h->E;
    a.m = h->m;
    a.P = h->P;
    a.F = h->F;
    a.rec = static_cast<unsigned>(map_rec(h));
    return launch_kernel<symmap_kernel>("symmap_kernel", dim3(static_cast<unsigned>(map_grid(h, n_frames))), dim3(SM_WG), 0, h->pick(stream),
                                        h->take_events(), a);
}

comms_status_t comms_symmap_run(comms_symmap_t* h, const void* bits, size_t n_frames, comms_c32* out) {
    return run_frame_call(h, map_call, bits, n_frames, out, [&](void* d_in, void* d_out) {
        return comms_symmap_run_dev(h, d_in, n_frames, static_cast<comms_c32*>(d_out), COMMS_STREAM_HANDLE);
    });
}

comms_status_t comms_symmap_get_kernel(const comms_symmap_t* h, size_t n_frames, char* name, size_t name_len) {
    COMMS_ARG(h && name && name_len, "NULL argument");
    std::snprintf(name, name_len, "symmap_kernel wg=%d bits=%u n_bits=%u word=%u payload=%u gap=%u syms=%zu frames=%zu grid=%zu max_grid=%u lds=%zu",
                  SM_WG, h->m, h->E, h->P, h->F, h->G, n_frames * map_rec(h), n_frames, map_grid(h, n_frames), h->max_grid, SM_TABLE_LDS);
    return COMMS_OK;
}

comms_status_t comms_symmap_set_timer(comms_symmap_t* h, comms_timer_t* t) { return set_handle_timer(h, t); }

comms_status_t comms_symmap_destroy(comms_symmap_t* h) { return destroy_handle(h); }

// ---- demapper
comms_status_t comms_demap_create(int32_t bits_per_sym, const comms_c32* constellation, size_t n_payload, int32_t flags, int32_t device,
                                  comms_demap_t** out) {
    COMMS_ARG(out != nullptr, "out is NULL");
    *out = nullptr;
    std::vector<float2> table;
    COMMS_TRY(take_table(bits_per_sym, constellation, &table));
    COMMS_ARG(n_payload >= 1 && n_payload <= SM_MAX_F, "a record has 1 <= n_payload <= 2^20 symbols (got %zu)", n_payload);
    COMMS_ARG((flags & ~COMMS_DEMAP_TABLE) == 0, "flags must be 0 or COMMS_DEMAP_TABLE (got %d)", flags);
    int mI = -1;
    std::vector<float> levels;
    if (!(flags & COMMS_DEMAP_TABLE)) find_split(table, bits_per_sym, &mI, &levels);
    HandlePtr<comms_demap> h;
    COMMS_TRY(make_handle(device, &h));
    h->m = static_cast<unsigned>(bits_per_sym);
    h->F = static_cast<unsigned>(n_payload);
    h->mI = mI;
    h->mQ = mI < 0 ? 0 : bits_per_sym - mI;
    COMMS_HIP_TRY(h->table.upload(table));
    if (mI >= 0) COMMS_HIP_TRY(h->levels.upload(levels));
    h->max_grid = resident_workgroups(0);
    *out = h.release();
    return COMMS_OK;
}

comms_status_t comms_demap_set_output_format(comms_demap_t* h, int32_t format) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG(format == COMMS_SYM_BITS || format == COMMS_SYM_LLR, "format must be COMMS_SYM_BITS or COMMS_SYM_LLR (got %d)", format);
    h->format = format;
    return COMMS_OK;
}

comms_status_t comms_demap_set_llr_scale(comms_demap_t* h, float scale) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG(std::isfinite(scale), "the LLR scale must be finite");
    h->scale = scale;
    return COMMS_OK;
}

size_t comms_demap_in_frame_bytes(const comms_demap_t* h) { return h ? static_cast<size_t>(h->F) * sizeof(comms_c32) : 0; }
size_t comms_demap_out_frame_bytes(const comms_demap_t* h) { return h ? demap_out_bytes(h) : 0; }

// the arguments of either device form behind its checks
static DemapArgs demap_args(const comms_demap* h, const comms_c32* d_sym, size_t n_frames, void* d_out) {
    DemapArgs a{};
    a.sym = reinterpret_cast<const float2*>(d_sym);
    a.out = d_out;
    a.table = h->table.get();
    a.pI = h->levels.get();
    a.pQ = h->mI < 0 ? nullptr : h->levels.get() + (size_t(1) << h->mI);
    a.n_frames = n_frames;
    a.items = demap_items(h, n_frames);
    a.F = h->F;
    a.chunks = static_cast<unsigned>(demap_chunks(h));
    a.rec_words = static_cast<unsigned>(bit_record_bytes(static_cast<size_t>(h->F) * h->m) / 4);
    a.scale = h->scale;
    return a;
}

comms_status_t comms_demap_run_dev(comms_demap_t* h, const comms_c32* d_sym, size_t n_frames, void* d_out, void* stream) {
    COMMS_TRY(check_frame_call(h, demap_call, d_sym, n_frames, d_out, true));
    if (!n_frames) return COMMS_OK;
    COMMS_TRY(use_device(h->device));
    const DemapArgs a = demap_args(h, d_sym, n_frames, d_out);
    const dim3 grid(static_cast<unsigned>(demap_grid(h, n_frames)));
    hipStream_t s = h->pick(stream);
    return h->format == COMMS_SYM_BITS ? demap_launch<COMMS_SYM_BITS>(h, a, grid, s) : demap_launch<COMMS_SYM_LLR>(h, a, grid, s);
}

// what both weighted forms check behind check_frame_call
static comms_status_t check_weights(const comms_demap* h, const float* weight, size_t weight_period, size_t n_frames) {
    COMMS_ARG(h->format == COMMS_SYM_LLR, "weighted demapping gives LLRs: the handle's output format is COMMS_SYM_BITS");
    COMMS_ARG(weight_period >= 1 && weight_period <= h->F, "weight_period must be 1 ... n_payload = %u (got %zu)", h->F, weight_period);
    COMMS_ARG(!n_frames || weight, "NULL pointer");
    return COMMS_OK;
}

comms_status_t comms_demap_run_weighted_dev(comms_demap_t* h, const comms_c32* d_sym, const float* d_weight, size_t weight_period,
                                            size_t n_frames, void* d_out, void* stream) {
    COMMS_TRY(check_frame_call(h, demap_call, d_sym, n_frames, d_out, true));
    COMMS_TRY(check_weights(h, d_weight, weight_period, n_frames));
    COMMS_ARG(aligned(d_weight, 4), "the weights must be aligned to 4 bytes");
    if (!n_frames) return COMMS_OK;
    COMMS_ARG(!ranges_overlap(d_weight, n_frames * weight_period * sizeof(float), d_out, n_frames * demap_out_bytes(h)),
              "the weights and the output records overlap");
    COMMS_TRY(use_device(h->device));
    DemapArgs a = demap_args(h, d_sym, n_frames, d_out);
    a.weight = d_weight;
    a.P = static_cast<unsigned>(weight_period);
    return demap_launch<SM_LLR_WEIGHTED>(h, a, dim3(static_cast<unsigned>(demap_grid(h, n_frames))), h->pick(stream));
}

comms_status_t comms_demap_run_weighted(comms_demap_t* h, const comms_c32* sym, const float* weight, size_t weight_period, size_t n_frames,
                                        void* out) {
    COMMS_TRY(check_frame_call(h, demap_call, sym, n_frames, out, false));
    COMMS_TRY(check_weights(h, weight, weight_period, n_frames));
    if (!n_frames) return COMMS_OK;
    COMMS_TRY(use_device(h->device));
    // one device block for the inputs: the symbol records, then the weights
    const size_t sym_b = n_frames * h->F * sizeof(comms_c32), w_b = n_frames * weight_period * sizeof(float), out_b = n_frames * demap_out_bytes(h);
    COMMS_TRY(h->in_scratch.reserve(sym_b + w_b));
    COMMS_TRY(h->out_scratch.reserve(out_b));
    char* d_in = static_cast<char*>(h->in_scratch.p);
    COMMS_HIP_TRY(hipMemcpyAsync(d_in, sym, sym_b, hipMemcpyHostToDevice, h->stream));
    COMMS_HIP_TRY(hipMemcpyAsync(d_in + sym_b, weight, w_b, hipMemcpyHostToDevice, h->stream));
    COMMS_TRY(comms_demap_run_weighted_dev(h, reinterpret_cast<const comms_c32*>(d_in), reinterpret_cast<const float*>(d_in + sym_b),
                                           weight_period, n_frames, h->out_scratch.p, COMMS_STREAM_HANDLE));
    COMMS_HIP_TRY(hipMemcpyAsync(out, h->out_scratch.p, out_b, hipMemcpyDeviceToHost, h->stream));
    COMMS_HIP_TRY(hipStreamSynchronize(h->stream));
    return COMMS_OK;
}

comms_status_t comms_demap_run(comms_demap_t* h, const comms_c32* sym, size_t n_frames, void* out) {
    return run_frame_call(h, demap_call, sym, n_frames, out, [&](void* d_in, void* d_out) {
        return comms_demap_run_dev(h, static_cast<const comms_c32*>(d_in), n_frames, d_out, COMMS_STREAM_HANDLE);
    });
}

comms_status_t comms_demap_get_kernel(const comms_demap_t* h, size_t n_frames, char* name, size_t name_len) {
    COMMS_ARG(h && name && name_len, "NULL argument");
    const bool bits = h->format == COMMS_SYM_BITS;
    char form[64];
    if (h->mI < 0)
        std::snprintf(form, sizeof form, "demap_table_kernel<%u,%s> form=table points=%u", h->m, bits ? "bits" : "llr", 1u << h->m);
    else
        std::snprintf(form, sizeof form, "demap_axis_kernel<%d,%d,%s> form=axis points=%u", h->mI, h->mQ, bits ? "bits" : "llr",
                      (1u << h->mI) + (1u << h->mQ));
    std::snprintf(name, name_len, "%s wg=%d bits=%u payload=%u items=%zu lanes=%zu frames=%zu grid=%zu max_grid=%u lds=0", form, SM_WG, h->m,
                  h->F, demap_items(h, n_frames), demap_items(h, n_frames) * (bits ? 64 : 1), n_frames, demap_grid(h, n_frames), h->max_grid);
    return COMMS_OK;
}

comms_status_t comms_demap_set_timer(comms_demap_t* h, comms_timer_t* t) { return set_handle_timer(h, t); }

comms_status_t comms_demap_destroy(comms_demap_t* h) { return destroy_handle(h); }

}  // extern "C"
