// deframe.hip -- deframer: the payloads behind the frame synchroniser's detections, derotated (and scaled) and written as
// packed bits, max-log LLRs or Complex<f32> symbols, every frame that becomes complete in a call by ONE launch.
//
// The reference has no such block; the contract is include/comms_hip.h's.  Per frame, on the host in f64, rounded once:
//   u = conj(c) / |c|,  g = Ep_word / |c| (COMMS_DEFRAME_NORMALISE) -- the descriptor {start, u, g} of the frame.
// Per payload symbol y, f32:  zr = fma(-yi, ui, yr ur),  zi = fma(yi, ur, yr ui),  then z *= g where normalising.
// The route it replaces is, per frame, comms_mixer_run_dev on a pointer offset and comms_sym_to_bits_dev: two launches and
// a host loop per detection, hard bits only, and nothing for a payload that ends in a later call.
//
// deframe_kernel<K, FMT>, one persistent launch over the flattened (frame, lane) space:
//   * a frame owns LPF lanes: its F symbols for C32 and LLR (an item is a symbol); for BITS its record's 32-bit words times
//     the 32 / K lanes that make one word (an item is a word), so that lane `pos` of a frame holds symbol `pos` -- the lanes
//     past F add zero bits -- and a word never straddles two frames (records are multiples of four bytes).  Short frames
//     share a workgroup, long ones span many; a lane takes (start, u, g) of its frame from the descriptor table.
//   * grid-stride loop under the library's grid cap; a lane divides once and then steps (frame, pos) by the stride's
//     quotient and remainder.  The lane count is rounded up to whole waves: every lane of a wave takes part in the OR.
//   * symbol loads are 8 bytes per lane, contiguous within a frame, from history-then-block (stream_at); stores are one
//     8-byte (C32, LLR at K = 2) or 4-byte (BITS word, LLR at K = 1) vector store per item.
//   * workgroup 0 writes the advanced history to the other half of the ping-pong pair (History, common.hpp).
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.hpp"
#include "fir_handle.hpp"
#include "stream_call.hpp"

namespace comms {

constexpr int DF_WG = 256;
constexpr size_t DF_MAX_PAYLOAD = size_t(1) << 20;   // symbols per frame
constexpr size_t DF_MAX_REACH = size_t(1) << 20;     // offset, lookback

struct DfDesc {
    long long start;  // first payload symbol, counted from the call's first symbol (negative: in the history)
    float ur, ui, g;
    float pad;
};

struct DfArgs {
    const float2* in;      // n symbols
    const float2* hist;    // the H symbols in front of them, time order
    float2* new_hist;
    const DfDesc* desc;    // n_frames descriptors
    void* out;
    size_t n, n_frames;
    size_t lanes;          // n_frames * lpf rounded up to whole waves
    size_t frame_bytes;
    unsigned F, lpf;       // payload symbols, lanes per frame
    int H;
    int normalise;
    float scale;           // LLR
    SymTable t;
};

template <int K, int FMT>
__global__ __launch_bounds__(DF_WG) void deframe_kernel(const DfArgs a) {
    constexpr int GL = 32 / K;  // lanes that make one packed word
    const unsigned stride = gridDim.x * DF_WG;
    const unsigned l0 = blockIdx.x * DF_WG + threadIdx.x;
    if (l0 < a.lanes) {  // wave-uniform: the lane count is whole waves
        const unsigned dq = stride / a.lpf, dr = stride % a.lpf;
        size_t frame = l0 / a.lpf;
        unsigned pos = l0 % a.lpf;
        for (size_t l = l0; l < a.lanes; l += stride) {
            const bool live = frame < a.n_frames && pos < a.F;
            float2 z = make_float2(0.f, 0.f);
            if (live) {
                const DfDesc d = a.desc[frame];
                const float2 y = stream_at(a.in, a.hist, a.H, d.start + static_cast<long long>(pos), a.n);
                z.x = __builtin_fmaf(-y.y, d.ui, __fmul_rn(y.x, d.ur));
                z.y = __builtin_fmaf(y.y, d.ur, __fmul_rn(y.x, d.ui));
                if (a.normalise) {
                    z.x = __fmul_rn(z.x, d.g);
                    z.y = __fmul_rn(z.y, d.g);
                }
            }
            if (FMT == COMMS_SYM_BITS) {
                unsigned bits = live ? sym_decide<K>(z, a.t.c) << (K * (pos % GL)) : 0u;
                bits = bits_gather<GL>(bits);
                if (frame < a.n_frames && pos % GL == 0)
                    bits_store_word(static_cast<uint8_t*>(a.out), frame * a.frame_bytes + 4 * static_cast<size_t>(pos / GL),
                                    a.n_frames * a.frame_bytes, bits);
            } else if (live) {
                const size_t at = frame * a.F + pos;
                if (FMT == COMMS_SYM_C32) {
                    static_cast<float2*>(a.out)[at] = z;
                } else if (K == 1) {
                    const float d0 = sym_dist(z, a.t.c[0]), d1 = sym_dist(z, a.t.c[1]);
                    static_cast<float*>(a.out)[at] = __fmul_rn(a.scale, __fsub_rn(d1, d0));
                } else {
                    const float d0 = sym_dist(z, a.t.c[0]), d1 = sym_dist(z, a.t.c[1]);
                    const float d2 = sym_dist(z, a.t.c[2]), d3 = sym_dist(z, a.t.c[3]);
                    // minima scanned ascending, replaced on a strictly smaller distance (as sym_decide)
                    const float b0z = d2 < d0 ? d2 : d0, b0o = d3 < d1 ? d3 : d1;   // bit 0: points 0, 2 against 1, 3
                    const float b1z = d1 < d0 ? d1 : d0, b1o = d3 < d2 ? d3 : d2;   // bit 1: points 0, 1 against 2, 3
                    static_cast<float2*>(a.out)[at] =
                        make_float2(__fmul_rn(a.scale, __fsub_rn(b0o, b0z)), __fmul_rn(a.scale, __fsub_rn(b1o, b1z)));
                }
            }
            frame += dq;
            pos += dr;
            if (pos >= a.lpf) {
                pos -= a.lpf;
                ++frame;
            }
        }
    }
    hist_advance(a.hist, a.in, a.n, a.new_hist, a.H);
}

}  // namespace comms

using namespace comms;

struct comms_deframe : Handle {
    size_t F = 0, offset = 0, lookback = 0;
    int H = 0;
    int format = COMMS_SYM_C32;
    bool normalise = false;
    double Ep = 0.0;           // energy of the word (0: not set)
    float scale = 1.0f;        // LLR
    SymTable table{};
    uint64_t T = 0;            // symbols seen: the stream index of the next one
    unsigned max_grid = 1;
    std::vector<comms_deframe_header_t> pending;   // ascending index; every one incomplete after a call
    Pinned desc_host;          // the descriptor table of a call as the host writes it ...
    Scratch desc_dev;          // ... and where the launch reads it
    History hist;              // last H symbols
};
static_assert(!std::is_copy_constructible_v<comms_deframe>, "a handle is never copied");

namespace {

comms_status_t check_shape(size_t n_payload, size_t lookback) {
    COMMS_ARG(n_payload >= 1 && n_payload <= DF_MAX_PAYLOAD, "n_payload must be 1 ... %zu symbols (got %zu)", DF_MAX_PAYLOAD, n_payload);
    COMMS_ARG(lookback <= DF_MAX_REACH, "lookback must be at most %zu symbols (got %zu)", DF_MAX_REACH, lookback);
    return COMMS_OK;
}

size_t frame_bytes_of(const comms_deframe* h) {
    const size_t k = static_cast<size_t>(h->table.k);
    switch (h->format) {
        case COMMS_SYM_BITS: return bit_record_bytes(h->F * k);
        case COMMS_SYM_LLR: return h->F * k * sizeof(float);
        default: return h->F * sizeof(comms_c32);
    }
}

// lanes per frame of the launch (see the head of the file)
size_t lanes_per_frame(const comms_deframe* h) {
    return h->format == COMMS_SYM_BITS ? frame_bytes_of(h) / 4 * (32 / static_cast<size_t>(h->table.k)) : h->F;
}

size_t deframe_lanes(const comms_deframe* h, size_t n_frames) { return (n_frames * lanes_per_frame(h) + 63) / 64 * 64; }

size_t deframe_grid(const comms_deframe* h, size_t n_frames) { return capped_grid((deframe_lanes(h, n_frames) + DF_WG - 1) / DF_WG, h->max_grid); }

// The detections of a call as pending entries behind h->pending, or COMMS_ERR_ARG; nothing of the handle changes.
comms_status_t admit(const comms_deframe* h, const comms_frame_detection_t* dets, size_t n_dets,
                     std::vector<comms_deframe_header_t>* fresh) {
    COMMS_ARG(dets != nullptr || !n_dets, "dets is NULL with n_dets > 0");
    if (n_dets && h->normalise)
        COMMS_ARG(std::isfinite(h->Ep) && h->Ep > 0.0, "COMMS_DEFRAME_NORMALISE needs the word energy (comms_deframe_set_word_energy)");
    bool have_last = !h->pending.empty();
    uint64_t last = have_last ? h->pending.back().index : 0;
    const long long oldest = static_cast<long long>(h->T) - static_cast<long long>(h->lookback);
    fresh->reserve(n_dets);
    for (size_t i = 0; i < n_dets; ++i) {
        const comms_frame_detection_t& d = dets[i];
        COMMS_ARG(std::isfinite(d.corr_re) && std::isfinite(d.corr_im), "detection %zu: corr is not finite", i);
        const double cr = d.corr_re, ci = d.corr_im;
        const double mag = std::hypot(cr, ci);
        COMMS_ARG(mag > 0.0, "detection %zu: corr is zero", i);
        COMMS_ARG(d.index <= (1ull << 62), "detection %zu: index is out of range", i);
        COMMS_ARG(!have_last || d.index > last, "detection %zu: index %llu is out of ascending order", i, static_cast<unsigned long long>(d.index));
        const uint64_t start = d.index + h->offset;
        COMMS_ARG(static_cast<long long>(start) >= oldest, "detection %zu: its payload starts at %llu, more than lookback = %zu symbols before the call (stale)",
                  i, static_cast<unsigned long long>(start), h->lookback);
        comms_deframe_header_t e;
        e.index = d.index;
        e.start = start;
        e.rot_re = static_cast<float>(cr / mag);
        e.rot_im = static_cast<float>(-ci / mag);
        e.gain = h->normalise ? static_cast<float>(h->Ep / mag) : 1.0f;
        e.metric = d.metric;
        fresh->push_back(e);
        last = d.index;
        have_last = true;
    }
    return COMMS_OK;
}

size_t count_ready(const comms_deframe* h, const std::vector<comms_deframe_header_t>& fresh, uint64_t T_after) {
    size_t c = 0;
    for (const auto& e : h->pending) c += e.start + h->F <= T_after;
    for (const auto& e : fresh) c += e.start + h->F <= T_after;
    return c;
}

// What both run entries do once their arguments hold: admit, count, one launch, bookkeeping.  Ends synchronised.
comms_status_t deframe_step(comms_deframe* h, const comms_c32* d_in, size_t n, const comms_frame_detection_t* dets, size_t n_dets,
                            void* d_out, size_t cap_frames, comms_deframe_header_t* headers, size_t* n_frames, void* stream) {
    std::vector<comms_deframe_header_t> fresh;
    COMMS_TRY(admit(h, dets, n_dets, &fresh));
    const uint64_t T_after = h->T + n;
    const size_t ready = count_ready(h, fresh, T_after);
    COMMS_ARG(ready <= cap_frames, "%zu frames become complete in this call, more than cap_frames = %zu", ready, cap_frames);
    COMMS_ARG(d_out != nullptr || !ready, "d_out is NULL");
    if (!n && !ready) {  // nothing to read or write: the detections join the list
        h->pending.insert(h->pending.end(), fresh.begin(), fresh.end());
        return COMMS_OK;
    }
    hipStream_t s = nullptr;
    COMMS_TRY(h->enter(stream, &s));
    // completion is monotone in the index (one F, one offset): the frames of this call are a prefix of pending + fresh
    std::vector<comms_deframe_header_t> all(h->pending);
    all.insert(all.end(), fresh.begin(), fresh.end());
    COMMS_TRY(h->desc_host.reserve((ready ? ready : 1) * sizeof(DfDesc)));
    COMMS_TRY(h->desc_dev.reserve((ready ? ready : 1) * sizeof(DfDesc)));
    DfDesc* hd = static_cast<DfDesc*>(h->desc_host.h);
    for (size_t f = 0; f < ready; ++f) {
        hd[f].start = static_cast<long long>(all[f].start) - static_cast<long long>(h->T);
        hd[f].ur = all[f].rot_re;
        hd[f].ui = all[f].rot_im;
        hd[f].g = all[f].gain;
        hd[f].pad = 0.f;
    }
    if (ready) COMMS_HIP_TRY(hipMemcpyAsync(h->desc_dev.p, hd, ready * sizeof(DfDesc), hipMemcpyHostToDevice, s));
    DfArgs a{};
    a.in = reinterpret_cast<const float2*>(d_in);
    a.hist = h->hist.cur<float2>();
    a.new_hist = h->hist.next<float2>();
    a.desc = static_cast<const DfDesc*>(h->desc_dev.p);
    a.out = d_out;
    a.n = n;
    a.n_frames = ready;
    a.lanes = deframe_lanes(h, ready);
    a.frame_bytes = frame_bytes_of(h);
    a.F = static_cast<unsigned>(h->F);
    a.lpf = static_cast<unsigned>(lanes_per_frame(h));
    a.H = h->H;
    a.normalise = h->normalise ? 1 : 0;
    a.scale = h->scale;
    a.t = h->table;
    const dim3 grid(static_cast<unsigned>(deframe_grid(h, ready))), wg(DF_WG);
    h->tic(s);
    if (h->format == COMMS_SYM_C32)
        deframe_kernel<1, COMMS_SYM_C32><<<grid, wg, 0, s>>>(a);
    else if (h->format == COMMS_SYM_BITS && h->table.k == 1)
        deframe_kernel<1, COMMS_SYM_BITS><<<grid, wg, 0, s>>>(a);
    else if (h->format == COMMS_SYM_BITS)
        deframe_kernel<2, COMMS_SYM_BITS><<<grid, wg, 0, s>>>(a);
    else if (h->table.k == 1)
        deframe_kernel<1, COMMS_SYM_LLR><<<grid, wg, 0, s>>>(a);
    else
        deframe_kernel<2, COMMS_SYM_LLR><<<grid, wg, 0, s>>>(a);
    h->toc(s);
    COMMS_TRY(launch_ok("deframe_kernel"));
    h->hist.flip();
    h->T = T_after;
    if (headers) std::copy(all.begin(), all.begin() + static_cast<std::ptrdiff_t>(ready), headers);
    h->pending.assign(all.begin() + static_cast<std::ptrdiff_t>(ready), all.end());
    *n_frames = ready;
    const hipError_t e = hipStreamSynchronize(s);  // the descriptor table is rewritten by the next call
    if (e != hipSuccess) return fail(COMMS_ERR_DEVICE, "deframer: %s", hipGetErrorString(e));
    return COMMS_OK;
}

}  // namespace

extern "C" {

comms_status_t comms_deframe_state_len(size_t n_payload, size_t lookback, size_t* out_len) {
    COMMS_ARG(out_len != nullptr, "out_len is NULL");
    COMMS_TRY(check_shape(n_payload, lookback));
    *out_len = lookback > n_payload - 1 ? lookback : n_payload - 1;
    return COMMS_OK;
}

comms_status_t comms_deframe_create(size_t n_payload, size_t offset, size_t lookback, int32_t bits_per_sym, const comms_c32* constellation,
                                    int32_t flags, int32_t device, comms_deframe_t** out) {
    COMMS_ARG(out != nullptr, "out is NULL");
    *out = nullptr;
    COMMS_TRY(check_shape(n_payload, lookback));
    COMMS_ARG(offset <= DF_MAX_REACH, "offset must be at most %zu symbols (got %zu)", DF_MAX_REACH, offset);
    COMMS_ARG((flags & ~COMMS_DEFRAME_NORMALISE) == 0, "unknown flags 0x%x", flags);
    SymTable t{};
    COMMS_TRY(sym_table(bits_per_sym, constellation, &t));
    HandlePtr<comms_deframe> h;
    COMMS_TRY(make_handle(device, &h));
    h->F = n_payload;
    h->offset = offset;
    h->lookback = lookback;
    h->H = static_cast<int>(lookback > n_payload - 1 ? lookback : n_payload - 1);
    h->normalise = (flags & COMMS_DEFRAME_NORMALISE) != 0;
    h->table = t;
    h->max_grid = resident_workgroups(0);
    COMMS_HIP_TRY(h->hist.alloc(static_cast<size_t>(h->H), sizeof(comms_c32)));
    *out = h.release();
    return COMMS_OK;
}

comms_status_t comms_deframe_set_word_energy(comms_deframe_t* h, double word_energy) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG(std::isfinite(word_energy) && word_energy > 0.0, "word_energy must be finite and > 0 (got %g)", word_energy);
    h->Ep = word_energy;
    return COMMS_OK;
}

comms_status_t comms_deframe_set_output_format(comms_deframe_t* h, int32_t format) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG(format == COMMS_SYM_C32 || format == COMMS_SYM_BITS || format == COMMS_SYM_LLR,
              "format must be COMMS_SYM_C32, COMMS_SYM_BITS or COMMS_SYM_LLR (got %d)", format);
    h->format = format;
    return COMMS_OK;
}

comms_status_t comms_deframe_set_llr_scale(comms_deframe_t* h, float scale) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG(std::isfinite(scale), "scale must be finite");
    h->scale = scale;
    return COMMS_OK;
}

size_t comms_deframe_frame_bytes(const comms_deframe_t* h) { return h ? frame_bytes_of(h) : 0; }

comms_status_t comms_deframe_frames_ready(const comms_deframe_t* h, size_t n, const comms_frame_detection_t* dets, size_t n_dets,
                                          size_t* out_count) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG(out_count != nullptr, "out_count is NULL");
    COMMS_ARG(n <= SIZE_MAX / 8, "n overflows");
    std::vector<comms_deframe_header_t> fresh;
    COMMS_TRY(admit(h, dets, n_dets, &fresh));
    *out_count = count_ready(h, fresh, h->T + n);
    return COMMS_OK;
}

comms_status_t comms_deframe_run_dev(comms_deframe_t* h, const comms_c32* d_in, size_t n, const comms_frame_detection_t* dets, size_t n_dets,
                                     void* d_out, size_t cap_frames, comms_deframe_header_t* headers, size_t* n_frames, void* stream) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG(n_frames != nullptr, "n_frames is NULL");
    COMMS_ARG(d_in || !n, "d_in is NULL");
    COMMS_ARG(aligned(d_in, 8), "d_in must be aligned to one symbol (8 bytes)");
    const bool wide = h->format == COMMS_SYM_C32 || (h->format == COMMS_SYM_LLR && h->table.k == 2);  // 8-byte stores
    COMMS_ARG(aligned(d_out, wide ? 8 : 4), "d_out must be aligned to %d bytes", wide ? 8 : 4);
    COMMS_ARG(n <= SIZE_MAX / 8, "n overflows");
    *n_frames = 0;
    COMMS_TRY(use_device(h->device));
    return deframe_step(h, d_in, n, dets, n_dets, d_out, cap_frames, headers, n_frames, stream);
}

comms_status_t comms_deframe_run(comms_deframe_t* h, const comms_c32* in, size_t n, const comms_frame_detection_t* dets, size_t n_dets,
                                 void* out, size_t cap_frames, comms_deframe_header_t* headers, size_t* n_frames) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG(n_frames != nullptr, "n_frames is NULL");
    COMMS_ARG(in || !n, "in is NULL");
    COMMS_ARG(n <= SIZE_MAX / 8, "n overflows");
    *n_frames = 0;
    size_t ready = 0;
    COMMS_TRY(comms_deframe_frames_ready(h, n, dets, n_dets, &ready));
    COMMS_ARG(ready <= cap_frames, "%zu frames become complete in this call, more than cap_frames = %zu", ready, cap_frames);
    COMMS_ARG(out != nullptr || !ready, "out is NULL");
    COMMS_TRY(use_device(h->device));
    const void* d = nullptr;
    if (n) COMMS_TRY(stage_input(h, in, n * 8, &d));
    const size_t bytes = ready * frame_bytes_of(h);
    COMMS_TRY(h->out_scratch.reserve(bytes ? bytes : 8));
    COMMS_TRY(deframe_step(h, static_cast<const comms_c32*>(d), n, dets, n_dets, h->out_scratch.p, cap_frames, headers, n_frames,
                           COMMS_STREAM_HANDLE));
    if (bytes) COMMS_HIP_TRY(hipMemcpy(out, h->out_scratch.p, bytes, hipMemcpyDeviceToHost));  // the step ended synchronised
    return COMMS_OK;
}

comms_status_t comms_deframe_flush(comms_deframe_t* h, size_t* n_dropped) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_TRY(use_device(h->device));
    COMMS_TRY(h->quiesce());
    COMMS_HIP_TRY(h->hist.upload(nullptr, 0));  // zeros
    if (n_dropped) *n_dropped = h->pending.size();
    h->pending.clear();
    return COMMS_OK;
}

comms_status_t comms_deframe_get_state(comms_deframe_t* h, comms_c32* state, size_t n_state) {
    return get_history_state(h, state, n_state, "symbols");
}

comms_status_t comms_deframe_set_state(comms_deframe_t* h, const comms_c32* state, size_t n_state) {
    return set_history_state(h, state, n_state, "symbols");
}

comms_status_t comms_deframe_get_position(const comms_deframe_t* h, uint64_t* out_position) { return get_position(h, out_position); }

comms_status_t comms_deframe_set_position(comms_deframe_t* h, uint64_t position) {
    return set_position(h, position, [&] { h->pending.clear(); });
}

comms_status_t comms_deframe_get_pending(const comms_deframe_t* h, comms_deframe_header_t* out, size_t cap, size_t* n_pending) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG(n_pending != nullptr, "n_pending is NULL");
    COMMS_ARG(out != nullptr || !cap, "out is NULL with cap > 0");
    const size_t take = h->pending.size() < cap ? h->pending.size() : cap;
    if (take) std::memcpy(out, h->pending.data(), take * sizeof(comms_deframe_header_t));
    *n_pending = h->pending.size();
    return COMMS_OK;
}

comms_status_t comms_deframe_set_pending(comms_deframe_t* h, const comms_deframe_header_t* pending, size_t n_pending) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG(pending != nullptr || !n_pending, "pending is NULL");
    for (size_t i = 0; i < n_pending; ++i) {
        const comms_deframe_header_t& e = pending[i];
        COMMS_ARG(e.index <= (1ull << 62) && e.start == e.index + h->offset, "pending %zu: start is not index + offset", i);
        COMMS_ARG(!i || e.index > pending[i - 1].index, "pending %zu: out of ascending index order", i);
        COMMS_ARG(e.start + h->F > h->T, "pending %zu: the frame is complete at position %llu", i, static_cast<unsigned long long>(h->T));
        COMMS_ARG(static_cast<long long>(e.start) >= static_cast<long long>(h->T) - h->H, "pending %zu: the frame starts before the state", i);
        COMMS_ARG(std::isfinite(e.rot_re) && std::isfinite(e.rot_im) && std::isfinite(e.gain), "pending %zu: not finite", i);
    }
    h->pending.assign(pending, pending + n_pending);
    return COMMS_OK;
}

comms_status_t comms_deframe_get_kernel(const comms_deframe_t* h, size_t n_frames, char* name, size_t name_len) {
    COMMS_ARG(h && name && name_len, "NULL argument");
    const size_t per = h->format == COMMS_SYM_BITS ? frame_bytes_of(h) / 4 : h->F;
    std::snprintf(name, name_len, "deframe_kernel wg=%d items=%zu lanes=%zu grid=%zu max_grid=%u lds=0", DF_WG, n_frames * per,
                  deframe_lanes(h, n_frames), deframe_grid(h, n_frames), h->max_grid);
    return COMMS_OK;
}

comms_status_t comms_deframe_set_timer(comms_deframe_t* h, comms_timer_t* t) { return set_handle_timer(h, t); }

comms_status_t comms_deframe_destroy(comms_deframe_t* h) { return destroy_handle(h); }

}  // extern "C"
