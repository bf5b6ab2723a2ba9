// convcode.hip -- convolutional FEC: the rate-1/n encoder (conv_encode_kernel) and the Viterbi decoder (viterbi_kernel) of
// one code description, every frame of a call by ONE launch each.
//
// The reference has no such blocks; the contract is include/comms_hip.h's ("convolutional code").  In short:
//   register   r_t = (u_t << (K-1)) | s_t,  s_0 = 0,  s_{t+1} = r_t >> 1;  coded bit j of step t = parity(r_t & g_j) at t n + j.
//   decoder    q = clamp(rint(L * qscale), -127, 127) (NaN: 0), int32 path metrics, maximised, M_0 = {0, -2^30 ...};
//              state s' has the predecessors p_b = ((s' << 1) | b) & (S-1), input bit u = s' >> (K-2); b = 1 only on a
//              strictly greater candidate; traceback bit of step t = s >> (K-2), then s = ((s << 1) | d_t[s]) & (S-1).
// Everything below is integer once the LLRs are quantised, so the bits are those of tests/viterbi_ref.py exactly.
//
// conv_encode_kernel: a lane makes one 32-bit output word.  The word's coded bits belong to at most 17 steps, which read at most
// 17 + K - 1 <= 23 information bits: one 32-bit window cut from two input words (zeros in front of the frame, and from bit T
// on, whatever the record's padding holds).  Step k of the window has r = (window >> k) & (2^K - 1).  Grid-stride loop under
// the library's grid cap.
//
// viterbi_kernel<N, WS>: ONE WAVE DECODES ONE FRAME, lane s' holds the metric of state s' (lanes >= S idle along for K < 7:
// they read valid lanes and nobody reads them).  Persistent loop over the frames, VT_WAVES waves per workgroup, no barrier
// anywhere -- the waves of a workgroup never meet.
//   * exchange: the two predecessors' metrics come by two ds_bpermute_b32 of the metric register (addresses fixed per
//     launch).  The hinted alternative, one LDS write and one 8-byte read, needs a wave-scope fence per step to keep the
//     compiler from moving a lane's read over its own write; the permutes need none and no LDS.
//   * the signs 1 - 2c of a lane's two branches are 2 N masks (0 / -1) computed once per launch: +-q is (q ^ m) - m.
//   * LLRs: lane l loads and quantises the N values of step 64 blk + l (the block's 256 N bytes are read whole by the N
//     loads together), the next block's loads are in flight while this one is stepped; step tt takes them by v_readlane.
//   * the decision word of a step IS the 64-bit compare mask; lane tt keeps it, and the block's 64 words leave in one
//     8-byte-per-lane store: to LDS where the frame fits (steps <= VT_LDS_STEPS), else to the handle's device workspace.
//   * traceback: serial, scalar.  A block's 64 decision words are read back by one load (the block before it is already in
//     flight), the walk takes word tt by v_readlane and keeps the state in scalar registers; lanes 0 and 1 write the
//     block's two output words.  The parallelism is across frames.
// Bounds: |q| <= 127, N <= 3, at most 2^16 steps: a path gathers less than 2^16 * 3 * 127 < 2^25, and -2^30 - 2^25 > -2^31:
// nothing overflows and no normalisation is needed.
#include <algorithm>
#include <cmath>

#include "common.hpp"

namespace comms {

constexpr int CC_WG = 256;
constexpr int VT_WAVES = CC_WG / 64;
constexpr unsigned CC_MAX_STEPS = 1u << 16;
constexpr unsigned VT_LDS_STEPS = 2048;                 // frames up to here keep their survivors in LDS: 16 KiB per wave
constexpr size_t VT_WS_BUDGET = size_t(256) << 20;      // the device workspace of longer frames stays under this
constexpr size_t CC_MAX_FRAMES = size_t(1) << 32;

struct ConvCode {
    int K, n;
    unsigned g[3];
    unsigned T, steps;   // information bits, trellis steps (T + K - 1 terminated)
    bool terminated;
};

struct CeArgs {
    const unsigned* in;
    unsigned* out;
    size_t n_frames;
    unsigned in_words, out_words, T, steps;
    int K, n;
    unsigned g[3];
};

__global__ __launch_bounds__(CC_WG) void conv_encode_kernel(const CeArgs a) {
    const size_t stride = static_cast<size_t>(gridDim.x) * CC_WG;
    const size_t items = a.n_frames * a.out_words;
    const unsigned rmask = (1u << a.K) - 1u;
    for (size_t i = static_cast<size_t>(blockIdx.x) * CC_WG + threadIdx.x; i < items; i += stride) {
        const size_t f = i / a.out_words;
        const unsigned w = static_cast<unsigned>(i % a.out_words);
        const unsigned c0 = 32u * w, t0 = c0 / static_cast<unsigned>(a.n);
        unsigned j = c0 % static_cast<unsigned>(a.n);
        const int start = static_cast<int>(t0) - (a.K - 1);   // information bit at bit 0 of the window
        const int ws = start >> 5;
        const unsigned sh = static_cast<unsigned>(start) & 31u;
        unsigned word[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int at = ws + k;
            unsigned v = 0;
            if (at >= 0 && static_cast<unsigned>(at) < a.in_words) {
                v = a.in[f * a.in_words + static_cast<unsigned>(at)];
                const unsigned first = 32u * static_cast<unsigned>(at);          // bits from T on do not count
                if (a.T < first + 32u) v &= a.T > first ? (1u << (a.T - first)) - 1u : 0u;
            }
            word[k] = v;
        }
        const unsigned win = static_cast<unsigned>(((static_cast<unsigned long long>(word[1]) << 32) | word[0]) >> sh);
        unsigned out = 0, k = 0;
#pragma unroll
        for (int b = 0; b < 32; ++b) {
            const unsigned g = j == 0 ? a.g[0] : j == 1 ? a.g[1] : a.g[2];
            const unsigned bit = t0 + k < a.steps ? static_cast<unsigned>(__popc((win >> k) & rmask & g)) & 1u : 0u;
            out |= bit << b;
            if (++j == static_cast<unsigned>(a.n)) {
                j = 0;
                ++k;
            }
        }
        a.out[f * a.out_words + w] = out;
    }
}

struct VtArgs {
    const float* llr;
    unsigned* bits;
    int* metrics;                  // may be null
    unsigned long long* ws;        // WS: grid * VT_WAVES slots of blocks * 64 words
    size_t n_frames, record_llrs;
    unsigned steps, T, out_words, blocks;   // blocks = ceil(steps / 64)
    int K, terminated;
    unsigned g[3];
    float qscale;
};

template <int N, bool WS>
__global__ __launch_bounds__(CC_WG) void viterbi_kernel(const VtArgs a) {
    extern __shared__ unsigned long long vt_lds[];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned S = 1u << (a.K - 1);
    const size_t slot = static_cast<size_t>(a.blocks) * 64;
    unsigned long long* const surv = WS ? a.ws + (static_cast<size_t>(blockIdx.x) * VT_WAVES + wave) * slot : vt_lds + wave * slot;
    // the lane's two branches: where the predecessors' metrics are, and the signs of their coded bits
    const unsigned sp = lane & (S - 1u);
    const unsigned u = sp >> (a.K - 2);
    int from[2], neg[2][N];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const unsigned p = ((sp << 1) | static_cast<unsigned>(b)) & (S - 1u);
        from[b] = static_cast<int>(4u * p);
        const unsigned r = (u << (a.K - 1)) | p;
#pragma unroll
        for (int j = 0; j < N; ++j) neg[b][j] = -static_cast<int>(static_cast<unsigned>(__popc(r & a.g[j])) & 1u);
    }
    const unsigned total = static_cast<unsigned>(N) * a.steps;
    const size_t n_waves = static_cast<size_t>(gridDim.x) * VT_WAVES;
    for (size_t f = static_cast<size_t>(blockIdx.x) * VT_WAVES + wave; f < a.n_frames; f += n_waves) {  // wave-uniform
        const float* L = a.llr + f * a.record_llrs;
        int M = lane == 0 ? 0 : -(1 << 30);
        float x[N];
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const unsigned at = lane * N + static_cast<unsigned>(j);
            x[j] = at < total ? L[at] : 0.f;
        }
        for (unsigned blk = 0; blk < a.blocks; ++blk) {
            int q[N];
#pragma unroll
            for (int j = 0; j < N; ++j) q[j] = quantise_llr(x[j], a.qscale);
            if (blk + 1 < a.blocks) {
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    const unsigned at = ((blk + 1) * 64u + lane) * N + static_cast<unsigned>(j);
                    x[j] = at < total ? L[at] : 0.f;
                }
            }
            const unsigned left = a.steps - blk * 64u;
            const unsigned cnt = left < 64u ? left : 64u;
            unsigned long long dw = 0;
            for (unsigned tt = 0; tt < cnt; ++tt) {
                int m0 = __builtin_amdgcn_ds_bpermute(from[0], M);
                int m1 = __builtin_amdgcn_ds_bpermute(from[1], M);
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    const int qj = __builtin_amdgcn_readlane(q[j], static_cast<int>(tt));
                    m0 += (qj ^ neg[0][j]) - neg[0][j];
                    m1 += (qj ^ neg[1][j]) - neg[1][j];
                }
                const bool take = m1 > m0;                     // b = 1 only when strictly greater
                const unsigned long long mask = __ballot(take);
                M = take ? m1 : m0;
                dw = lane == tt ? mask : dw;
            }
            surv[static_cast<size_t>(blk) * 64 + lane] = dw;   // all 64 words: the walk reads whole blocks
        }
        // where the path ends
        int s_end = 0;
        if (!a.terminated) {
            int best = lane < S ? M : INT32_MIN;
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                const int other = __shfl_xor(best, o);
                best = other > best ? other : best;
            }
            const unsigned long long at_best = __ballot(lane < S && M == best);
            s_end = __ffsll(static_cast<long long>(at_best)) - 1;   // the lowest index among equal metrics
        }
        s_end = __builtin_amdgcn_readfirstlane(s_end);
        const int metric = __builtin_amdgcn_readlane(M, s_end);
        if (a.metrics != nullptr && lane == 0) a.metrics[f] = metric;
        __threadfence_block();   // the survivors were written by other lanes of this wave
        unsigned s = static_cast<unsigned>(s_end);
        unsigned long long d = surv[static_cast<size_t>(a.blocks - 1) * 64 + lane];
        for (int blk = static_cast<int>(a.blocks) - 1; blk >= 0; --blk) {
            const unsigned long long dn = blk > 0 ? surv[static_cast<size_t>(blk - 1) * 64 + lane] : 0ull;
            const int lo = static_cast<int>(static_cast<unsigned>(d)), hi = static_cast<int>(static_cast<unsigned>(d >> 32));
            const unsigned left = a.steps - static_cast<unsigned>(blk) * 64u;
            unsigned long long out = 0;
            for (int tt = static_cast<int>(left < 64u ? left : 64u) - 1; tt >= 0; --tt) {
                const unsigned long long w = (static_cast<unsigned long long>(static_cast<unsigned>(__builtin_amdgcn_readlane(hi, tt))) << 32) |
                                             static_cast<unsigned>(__builtin_amdgcn_readlane(lo, tt));
                out |= static_cast<unsigned long long>(s >> (a.K - 2)) << tt;
                s = ((s << 1) | static_cast<unsigned>((w >> s) & 1ull)) & (S - 1u);
            }
            const unsigned first = static_cast<unsigned>(blk) * 64u;          // bits from T on (the tail, padding) are 0
            if (a.T < first + 64u) out &= a.T > first ? (1ull << (a.T - first)) - 1ull : 0ull;
            const unsigned wi = 2u * static_cast<unsigned>(blk) + lane;
            if (lane < 2u && wi < a.out_words) a.bits[f * a.out_words + wi] = static_cast<unsigned>(lane ? out >> 32 : out);
            d = dn;
        }
    }
}

// The code of a create call, or COMMS_ERR_ARG: host arithmetic only
inline comms_status_t conv_code(int32_t K, int32_t n, const uint32_t* gens, int32_t flags, size_t n_info_bits, ConvCode* out) {
    COMMS_ARG(K >= 3 && K <= 7, "constraint length K must be 3 ... 7 (got %d)", K);
    COMMS_ARG(n == 2 || n == 3, "a code has n = 2 or 3 generators (got %d)", n);
    COMMS_ARG(flags == COMMS_CONV_TERMINATED || flags == COMMS_CONV_TRUNCATED, "flags must be COMMS_CONV_TERMINATED or COMMS_CONV_TRUNCATED (got 0x%x)", flags);
    COMMS_ARG(gens != nullptr || (K == 7 && n == 2), "gens is NULL: the default generators are those of K = 7, n = 2");
    ConvCode c{};
    c.K = K;
    c.n = n;
    for (int j = 0; j < n; ++j) {
        c.g[j] = gens ? gens[j] : (j == 0 ? 0171u : 0133u);
        COMMS_ARG(c.g[j] > 0 && c.g[j] < (1u << K), "generator %d must be 0 < g < 2^K (got %u)", j, c.g[j]);
    }
    c.terminated = flags == COMMS_CONV_TERMINATED;
    const size_t steps = n_info_bits + (c.terminated ? static_cast<size_t>(K - 1) : 0);
    COMMS_ARG(n_info_bits >= 1 && n_info_bits <= CC_MAX_STEPS && steps <= CC_MAX_STEPS, "a frame has 1 <= n_info_bits and at most %u steps (got %zu bits)",
              CC_MAX_STEPS, n_info_bits);
    c.T = static_cast<unsigned>(n_info_bits);
    c.steps = static_cast<unsigned>(steps);
    *out = c;
    return COMMS_OK;
}

}  // namespace comms

using namespace comms;

struct comms_convenc : Handle {
    ConvCode code{};
    unsigned max_grid = 1;
};
struct comms_viterbi : Handle {
    ConvCode code{};
    size_t record_llrs = 0;
    float qscale = 1.0f;
    bool in_lds = true;
    size_t lds = 0;             // bytes of dynamic LDS per workgroup
    unsigned max_grid = 1;
    Scratch workspace;          // survivors of the frames in flight where they do not fit the LDS
};
static_assert(!std::is_copy_constructible_v<comms_viterbi> && !std::is_copy_constructible_v<comms_convenc>, "a handle is never copied");

namespace {

size_t enc_in_bytes(const comms_convenc* h) { return bit_record_bytes(h->code.T); }
size_t enc_out_bytes(const comms_convenc* h) { return bit_record_bytes(static_cast<size_t>(h->code.n) * h->code.steps); }
size_t enc_grid(const comms_convenc* h, size_t n_frames) { return capped_grid((n_frames * (enc_out_bytes(h) / 4) + CC_WG - 1) / CC_WG, h->max_grid); }
FrameCall enc_call(const comms_convenc* h) { return {enc_in_bytes(h), enc_out_bytes(h), 4, 4, CC_MAX_FRAMES}; }

size_t vt_blocks(const comms_viterbi* h) { return (h->code.steps + 63) / 64; }
size_t vt_slot_bytes(const comms_viterbi* h) { return vt_blocks(h) * 64 * sizeof(unsigned long long); }
size_t vt_grid(const comms_viterbi* h, size_t n_frames) { return capped_grid((n_frames + VT_WAVES - 1) / VT_WAVES, h->max_grid); }
// the LLR records and the bit records; the metrics are the decoder's own
FrameCall vt_call(const comms_viterbi* h) { return {h->record_llrs * sizeof(float), bit_record_bytes(h->code.T), 4, 4, CC_MAX_FRAMES}; }

}  // namespace

extern "C" {

// ---- encoder
comms_status_t comms_convenc_create(int32_t K, int32_t n, const uint32_t* gens, int32_t flags, size_t n_info_bits, int32_t device,
                                    comms_convenc_t** out) {
    COMMS_ARG(out != nullptr, "out is NULL");
    *out = nullptr;
    ConvCode c{};
    COMMS_TRY(conv_code(K, n, gens, flags, n_info_bits, &c));
    HandlePtr<comms_convenc> h;
    COMMS_TRY(make_handle(device, &h));
    h->code = c;
    h->max_grid = resident_workgroups(0);
    *out = h.release();
    return COMMS_OK;
}

size_t comms_convenc_in_frame_bytes(const comms_convenc_t* h) { return h ? enc_in_bytes(h) : 0; }
size_t comms_convenc_out_frame_bytes(const comms_convenc_t* h) { return h ? enc_out_bytes(h) : 0; }

comms_status_t comms_convenc_run_dev(comms_convenc_t* h, const void* d_in, size_t n_frames, void* d_out, void* stream) {
    COMMS_TRY(check_frame_call(h, enc_call, d_in, n_frames, d_out, true));
    if (!n_frames) return COMMS_OK;
    COMMS_TRY(use_device(h->device));
    CeArgs a{};
    a.in = static_cast<const unsigned*>(d_in);
    a.out = static_cast<unsigned*>(d_out);
    a.n_frames = n_frames;
    a.in_words = static_cast<unsigned>(enc_in_bytes(h) / 4);
    a.out_words = static_cast<unsigned>(enc_out_bytes(h) / 4);
    a.T = h->code.T;
    a.steps = h->code.steps;
    a.K = h->code.K;
    a.n = h->code.n;
    for (int j = 0; j < 3; ++j) a.g[j] = h->code.g[j];
    const dim3 grid(static_cast<unsigned>(enc_grid(h, n_frames))), wg(CC_WG);
    return launch_kernel<conv_encode_kernel>("conv_encode_kernel", grid, wg, 0, h->pick(stream), h->take_events(), a);
}

comms_status_t comms_convenc_run(comms_convenc_t* h, const void* in, size_t n_frames, void* out) {
    return run_frame_call(h, enc_call, in, n_frames, out,
                          [&](void* d_in, void* d_out) { return comms_convenc_run_dev(h, d_in, n_frames, d_out, COMMS_STREAM_HANDLE); });
}

comms_status_t comms_convenc_get_kernel(const comms_convenc_t* h, size_t n_frames, char* name, size_t name_len) {
    COMMS_ARG(h && name && name_len, "NULL argument");
    std::snprintf(name, name_len, "conv_encode_kernel wg=%d K=%d n=%d steps=%u words=%zu grid=%zu max_grid=%u lds=0", CC_WG, h->code.K, h->code.n,
                  h->code.steps, n_frames * (enc_out_bytes(h) / 4), enc_grid(h, n_frames), h->max_grid);
    return COMMS_OK;
}

comms_status_t comms_convenc_set_timer(comms_convenc_t* h, comms_timer_t* t) { return set_handle_timer(h, t); }

comms_status_t comms_convenc_destroy(comms_convenc_t* h) { return destroy_handle(h); }

// ---- decoder
comms_status_t comms_viterbi_create(int32_t K, int32_t n, const uint32_t* gens, int32_t flags, size_t n_info_bits, size_t record_llrs,
                                    int32_t device, comms_viterbi_t** out) {
    COMMS_ARG(out != nullptr, "out is NULL");
    *out = nullptr;
    ConvCode c{};
    COMMS_TRY(conv_code(K, n, gens, flags, n_info_bits, &c));
    const size_t used = static_cast<size_t>(c.n) * c.steps;
    COMMS_ARG(record_llrs == 0 || record_llrs >= used, "record_llrs must be 0 or at least n * steps = %zu (got %zu)", used, record_llrs);
    COMMS_ARG(record_llrs <= (size_t(1) << 32), "record_llrs must be at most 2^32 (got %zu)", record_llrs);
    HandlePtr<comms_viterbi> h;
    COMMS_TRY(make_handle(device, &h));
    h->code = c;
    h->record_llrs = record_llrs ? record_llrs : used;
    h->in_lds = c.steps <= VT_LDS_STEPS;
    h->lds = h->in_lds ? VT_WAVES * vt_slot_bytes(h.get()) : 0;
    h->max_grid = resident_workgroups(h->lds);
    if (!h->in_lds) {  // as many waves in flight as the workspace budget holds slots
        const size_t fit = VT_WS_BUDGET / (VT_WAVES * vt_slot_bytes(h.get()));
        if (fit < h->max_grid) h->max_grid = static_cast<unsigned>(fit < 1 ? 1 : fit);
    }
    *out = h.release();
    return COMMS_OK;
}

comms_status_t comms_viterbi_set_quant_scale(comms_viterbi_t* h, float qscale) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG(std::isfinite(qscale), "qscale must be finite");
    h->qscale = qscale;
    return COMMS_OK;
}

size_t comms_viterbi_in_frame_bytes(const comms_viterbi_t* h) { return h ? h->record_llrs * sizeof(float) : 0; }
size_t comms_viterbi_out_frame_bytes(const comms_viterbi_t* h) { return h ? bit_record_bytes(h->code.T) : 0; }

comms_status_t comms_viterbi_run_dev(comms_viterbi_t* h, const float* d_llr, size_t n_frames, void* d_bits, int32_t* d_metrics, void* stream) {
    COMMS_TRY(check_frame_call(h, vt_call, d_llr, n_frames, d_bits, true));
    COMMS_ARG(aligned(d_metrics, 4), "d_metrics must be aligned to 4 bytes");
    if (!n_frames) return COMMS_OK;
    COMMS_TRY(use_device(h->device));
    const size_t grid_n = vt_grid(h, n_frames);
    if (!h->in_lds) {
        const size_t need = grid_n * VT_WAVES * vt_slot_bytes(h);
        if (need > h->workspace.cap) {  // growing frees the old block: nothing of this handle may still be running on it
            COMMS_TRY(h->quiesce());
            COMMS_TRY(h->workspace.reserve(need));
        }
    }
    hipStream_t s = nullptr;
    COMMS_TRY(h->enter(stream, &s));  // the workspace belongs to one stream at a time
    VtArgs a{};
    a.llr = d_llr;
    a.bits = static_cast<unsigned*>(d_bits);
    a.metrics = d_metrics;
    a.ws = static_cast<unsigned long long*>(h->workspace.p);
    a.n_frames = n_frames;
    a.record_llrs = h->record_llrs;
    a.steps = h->code.steps;
    a.T = h->code.T;
    a.out_words = static_cast<unsigned>(comms_viterbi_out_frame_bytes(h) / 4);
    a.blocks = static_cast<unsigned>(vt_blocks(h));
    a.K = h->code.K;
    a.terminated = h->code.terminated ? 1 : 0;
    for (int j = 0; j < 3; ++j) a.g[j] = h->code.g[j];
    a.qscale = h->qscale;
    const dim3 grid(static_cast<unsigned>(grid_n)), wg(CC_WG);
    if (h->code.n == 2)
        return h->in_lds ? launch_kernel<viterbi_kernel<2, false>>("viterbi_kernel", grid, wg, h->lds, s, h->take_events(), a)
                         : launch_kernel<viterbi_kernel<2, true>>("viterbi_kernel", grid, wg, 0, s, h->take_events(), a);
    return h->in_lds ? launch_kernel<viterbi_kernel<3, false>>("viterbi_kernel", grid, wg, h->lds, s, h->take_events(), a)
                     : launch_kernel<viterbi_kernel<3, true>>("viterbi_kernel", grid, wg, 0, s, h->take_events(), a);
}

comms_status_t comms_viterbi_run(comms_viterbi_t* h, const float* llr, size_t n_frames, void* bits, int32_t* metrics) {
    COMMS_TRY(check_frame_call(h, vt_call, llr, n_frames, bits, false));
    const size_t in_b = vt_call(h).in_bytes, out_b = vt_call(h).out_bytes;
    if (!n_frames) return COMMS_OK;
    COMMS_TRY(use_device(h->device));
    // the records, then the metrics, in one device block
    const size_t bits_bytes = n_frames * out_b;
    COMMS_TRY(h->in_scratch.reserve(n_frames * in_b));
    COMMS_TRY(h->out_scratch.reserve(bits_bytes + n_frames * sizeof(int32_t)));
    char* d_out = static_cast<char*>(h->out_scratch.p);
    int32_t* d_metrics = metrics ? reinterpret_cast<int32_t*>(d_out + bits_bytes) : nullptr;
    COMMS_HIP_TRY(hipMemcpyAsync(h->in_scratch.p, llr, n_frames * in_b, hipMemcpyHostToDevice, h->stream));
    COMMS_TRY(comms_viterbi_run_dev(h, static_cast<const float*>(h->in_scratch.p), n_frames, d_out, d_metrics, COMMS_STREAM_HANDLE));
    COMMS_HIP_TRY(hipMemcpyAsync(bits, d_out, bits_bytes, hipMemcpyDeviceToHost, h->stream));
    if (metrics) COMMS_HIP_TRY(hipMemcpyAsync(metrics, d_metrics, n_frames * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    COMMS_HIP_TRY(hipStreamSynchronize(h->stream));
    return COMMS_OK;
}

comms_status_t comms_viterbi_get_kernel(const comms_viterbi_t* h, size_t n_frames, char* name, size_t name_len) {
    COMMS_ARG(h && name && name_len, "NULL argument");
    const size_t grid = vt_grid(h, n_frames);
    std::snprintf(name, name_len, "viterbi_kernel<%d,%s> wg=%d waves=%d K=%d steps=%u seam=%u grid=%zu max_grid=%u lds=%zu workspace=%zu", h->code.n,
                  h->in_lds ? "lds" : "workspace", CC_WG, VT_WAVES, h->code.K, h->code.steps, VT_LDS_STEPS, grid, h->max_grid, h->lds,
                  h->in_lds ? size_t(0) : grid * VT_WAVES * vt_slot_bytes(h));
    return COMMS_OK;
}

comms_status_t comms_viterbi_set_timer(comms_viterbi_t* h, comms_timer_t* t) { return set_handle_timer(h, t); }

comms_status_t comms_viterbi_destroy(comms_viterbi_t* h) { return destroy_handle(h); }

}  // extern "C"
