// ratematch.hip -- rate matching between the convolutional code and the air: puncturer, interleaver and scrambler of one frame
// format, transmit (ratematch_tx_kernel) and receive (ratematch_rx_kernel), every frame of a call by ONE launch each.
//
// The reference has no such block; the contract is include/comms_hip.h's ("rate matching").  In short, with kept[] the coded
// positions the pattern keeps (ascending) and pi[] the interleaver over the E kept bits:
//   src[k] = kept[pi[k]]                                  the coded position that feeds transmitted bit k
//   tx     tx_bit[k] = in_bit[src[k]] ^ scramble_bit[k]   records of N packed bits -> records of E packed bits
//   rx     out[i] = +0.0f where i is punctured, else in[inv[i]] with its sign bit toggled where scramble bit inv[i] is 1
// Only bits and words move, so the records are those of tests/ratematch_ref.py exactly.
//
// The host builds the tables once at create; they are read-only afterwards and the node keeps no other state.
//   tx table: src padded with zeros to 32 entries per output word, and the scramble words next to it.  A lane makes one
//     32-bit output word: 32 table reads, 32 gathered bit extracts from the frame's input record, one XOR with the scramble
//     word; the record's last word is masked to the bits below E.  Lane l takes the word's bits in the order (b + l) mod 32:
//     the lanes of a wave hold consecutive words, which lie 32 entries apart, and the rotation spreads them over the banks.
//   rx table: one int32 per coded position: -1 where punctured, else inv[i] with the scramble bit of that transmitted bit at
//     bit 30 (E < 2^18), so that a value costs ONE table read, one gathered 4-byte load and one coalesced 4-byte store.  The
//     store stays 4 bytes wide: a record is 4 N bytes behind a 4-byte aligned pointer, so a 16-byte store would need a second,
//     alignment-dependent path and a tail of its own.
// Table form.  Up to RM_LDS_SEAM entries (E for tx, N for rx) a workgroup copies the table to LDS once and walks its items
// from there; beyond it the lanes read the table from global memory, where every frame re-reads it from L2.  The seam is where
// staging stops being repaid: a workgroup's 256 lanes make 8192 transmitted bits per pass, four frames at the seam, and the
// receive grid is sized so that a workgroup walks at least as many values as it staged entries.  The input record's words
// are not staged: a frame's gathers hit lines its neighbours in the wave have just pulled in.
// Both kernels walk grid-stride under the library's grid cap and keep (frame, position) by addition: one 64-bit division per
// lane, not per item.
#include <algorithm>

#include "common.hpp"

namespace comms {

constexpr int RM_WG = 256;
constexpr unsigned RM_MAX_CODED = 3u << 16;             // the encoder's n * steps at most
constexpr unsigned RM_MAX_PATTERN = 256;
constexpr unsigned RM_LDS_SEAM = 2048;                  // table entries up to here are staged in LDS: 8 KiB per workgroup
constexpr size_t RM_MAX_FRAMES = size_t(1) << 32;
constexpr unsigned RM_FLIP = 1u << 30;                  // rx table: the scramble bit of the entry

struct RmTxArgs {
    const unsigned* in;
    unsigned* out;
    const unsigned* src;        // out_words * 32 entries
    const unsigned* scramble;   // out_words words
    size_t n_frames;
    unsigned in_words, out_words, tail_mask;
};

struct RmRxArgs {
    const unsigned* in;         // f32 records, moved as words
    unsigned* out;
    const int* inv;             // n_coded entries
    size_t n_frames, record_llrs;
    unsigned n_coded;
};

// (frame, position) of a lane's items: item i = frame * per + pos, advanced by the grid's stride without dividing again
struct RmWalk {
    size_t frame, stride_frames;
    unsigned pos, stride_pos, per;
    __device__ RmWalk(size_t first, size_t stride, unsigned per_frame)
        : frame(first / per_frame), stride_frames(stride / per_frame), pos(static_cast<unsigned>(first % per_frame)),
          stride_pos(static_cast<unsigned>(stride % per_frame)), per(per_frame) {}
    __device__ void next() {
        frame += stride_frames;
        pos += stride_pos;       // both below per <= 3 * 2^16: no overflow
        if (pos >= per) {
            pos -= per;
            ++frame;
        }
    }
};

template <bool LDS>
__global__ __launch_bounds__(RM_WG) void ratematch_tx_kernel(const RmTxArgs a) {
    extern __shared__ unsigned rm_lds[];
    const unsigned* table = a.src;
    if (LDS) {
        for (unsigned k = threadIdx.x; k < 32u * a.out_words; k += RM_WG) rm_lds[k] = a.src[k];
        __syncthreads();
        table = rm_lds;
    }
    const size_t stride = static_cast<size_t>(gridDim.x) * RM_WG;
    const size_t items = a.n_frames * a.out_words;
    const size_t first = static_cast<size_t>(blockIdx.x) * RM_WG + threadIdx.x;
    RmWalk at(first, stride, a.out_words);
    for (size_t i = first; i < items; i += stride, at.next()) {
        const unsigned* rec = a.in + at.frame * a.in_words;
        const unsigned* t = table + 32u * at.pos;
        unsigned word = 0;
#pragma unroll
        for (unsigned b = 0; b < 32u; ++b) {
            const unsigned bb = (b + threadIdx.x) & 31u;
            const unsigned s = t[bb];
            word |= ((rec[s >> 5] >> (s & 31u)) & 1u) << bb;
        }
        word ^= a.scramble[at.pos];
        if (at.pos + 1u == a.out_words) word &= a.tail_mask;
        a.out[at.frame * a.out_words + at.pos] = word;
    }
}

template <bool LDS>
__global__ __launch_bounds__(RM_WG) void ratematch_rx_kernel(const RmRxArgs a) {
    extern __shared__ unsigned rm_lds[];
    const int* table = a.inv;
    if (LDS) {
        int* staged = reinterpret_cast<int*>(rm_lds);
        for (unsigned k = threadIdx.x; k < a.n_coded; k += RM_WG) staged[k] = a.inv[k];
        __syncthreads();
        table = staged;
    }
    const size_t stride = static_cast<size_t>(gridDim.x) * RM_WG;
    const size_t items = a.n_frames * a.n_coded;
    const size_t first = static_cast<size_t>(blockIdx.x) * RM_WG + threadIdx.x;
    RmWalk at(first, stride, a.n_coded);
    for (size_t i = first; i < items; i += stride, at.next()) {
        const int e = table[at.pos];
        unsigned v = 0;                                   // +0.0f: an erasure
        if (e >= 0) {
            const unsigned u = static_cast<unsigned>(e);
            v = a.in[at.frame * a.record_llrs + (u & (RM_FLIP - 1u))] ^ ((u & RM_FLIP) << 1);
        }
        a.out[i] = v;
    }
}

// The frame format of a create call, or COMMS_ERR_ARG: host arithmetic only
struct RmFormat {
    unsigned n_coded = 0, n_tx = 0;
    size_t record_llrs = 0;
    std::vector<unsigned> src;        // n_tx entries
    std::vector<unsigned> tx_table;   // src, zero-padded to 32 entries per output word
    std::vector<unsigned> scramble;   // one word per output word, bits from n_tx on 0
    std::vector<int> rx_table;        // n_coded entries
};

inline comms_status_t rm_format(size_t n_coded, const uint8_t* pattern, size_t pattern_len, size_t cols, const uint32_t* perm,
                                const void* scramble, size_t record_llrs, RmFormat* out) {
    COMMS_ARG(n_coded >= 1 && n_coded <= RM_MAX_CODED, "a frame has 1 <= n_coded <= 3 * 2^16 coded bits (got %zu)", n_coded);
    COMMS_ARG(pattern ? (pattern_len >= 1 && pattern_len <= RM_MAX_PATTERN) : pattern_len == 0,
              "a pattern has 1 ... %u bytes, and NULL goes with pattern_len = 0 (got %zu)", RM_MAX_PATTERN, pattern_len);
    bool any = pattern == nullptr;
    for (size_t i = 0; i < pattern_len; ++i) {
        COMMS_ARG(pattern[i] <= 1, "pattern byte %zu must be 0 or 1 (got %u)", i, static_cast<unsigned>(pattern[i]));
        any = any || pattern[i] == 1;
    }
    COMMS_ARG(any, "the pattern keeps no position");
    RmFormat f;
    f.n_coded = static_cast<unsigned>(n_coded);
    std::vector<unsigned> kept;
    kept.reserve(n_coded);
    for (unsigned i = 0; i < f.n_coded; ++i)
        if (!pattern || pattern[i % pattern_len]) kept.push_back(i);
    const size_t E = kept.size();
    COMMS_ARG(E >= 1, "the pattern keeps no position below n_coded = %zu", n_coded);
    f.n_tx = static_cast<unsigned>(E);
    COMMS_ARG(record_llrs == 0 || record_llrs >= E, "record_llrs must be 0 or at least the %zu transmitted bits (got %zu)", E, record_llrs);
    COMMS_ARG(record_llrs <= (size_t(1) << 32), "record_llrs must be at most 2^32 (got %zu)", record_llrs);
    f.record_llrs = record_llrs ? record_llrs : E;
    // pi: the kept-bit index that is transmitted k-th
    std::vector<unsigned> pi(E);
    if (perm) {
        COMMS_ARG(cols == 0, "cols must be 0 with an explicit perm (got %zu)", cols);
        std::vector<char> seen(E, 0);
        for (size_t k = 0; k < E; ++k) {
            COMMS_ARG(perm[k] < E && !seen[perm[k]], "perm is not a permutation of 0 ... %zu (entry %zu = %u)", E - 1, k, perm[k]);
            seen[perm[k]] = 1;
            pi[k] = perm[k];
        }
    } else if (cols <= 1) {
        for (size_t k = 0; k < E; ++k) pi[k] = static_cast<unsigned>(k);
    } else {
        COMMS_ARG(cols <= E, "the interleaver has at most as many columns as transmitted bits, %zu (got %zu)", E, cols);
        const size_t C = cols, R = (E + C - 1) / C, rem = E - (R - 1) * C;   // columns below rem hold R cells, the rest R - 1
        for (size_t m = 0; m < E; ++m) {
            const size_t r = m / C, c = m % C;
            pi[c * R - (c > rem ? c - rem : 0) + r] = static_cast<unsigned>(m);
        }
    }
    const size_t words = bit_record_bytes(E) / 4;
    f.src.resize(E);
    f.tx_table.assign(words * 32, 0u);
    f.scramble.assign(words, 0u);
    f.rx_table.assign(n_coded, -1);
    const uint8_t* sc = static_cast<const uint8_t*>(scramble);
    for (size_t k = 0; k < E; ++k) {
        const unsigned s = kept[pi[k]];
        const unsigned flip = sc ? (sc[k / 8] >> (k % 8)) & 1u : 0u;
        f.src[k] = f.tx_table[k] = s;
        f.scramble[k / 32] |= flip << (k % 32);
        f.rx_table[s] = static_cast<int>(static_cast<unsigned>(k) | (flip ? RM_FLIP : 0u));
    }
    *out = std::move(f);
    return COMMS_OK;
}

}  // namespace comms

using namespace comms;

struct comms_ratematch : Handle {
    unsigned n_coded = 0, n_tx = 0;
    size_t record_llrs = 0;
    std::vector<unsigned> src;                  // host copy, for comms_ratematch_get_map
    DevBuf<unsigned> tx_table, scramble;
    DevBuf<int> rx_table;
    size_t tx_lds = 0, rx_lds = 0;              // bytes of dynamic LDS per workgroup (0: the table is read from global memory)
    unsigned tx_max_grid = 1, rx_max_grid = 1;
};
static_assert(!std::is_copy_constructible_v<comms_ratematch>, "a handle is never copied");

namespace {

size_t tx_in_bytes(const comms_ratematch* h) { return bit_record_bytes(h->n_coded); }
size_t tx_out_bytes(const comms_ratematch* h) { return bit_record_bytes(h->n_tx); }
size_t rx_in_bytes(const comms_ratematch* h) { return h->record_llrs * sizeof(float); }
size_t rx_out_bytes(const comms_ratematch* h) { return static_cast<size_t>(h->n_coded) * sizeof(float); }

FrameCall tx_call(const comms_ratematch* h) { return {tx_in_bytes(h), tx_out_bytes(h), 4, 4, RM_MAX_FRAMES}; }
FrameCall rx_call(const comms_ratematch* h) { return {rx_in_bytes(h), rx_out_bytes(h), 4, 4, RM_MAX_FRAMES}; }

size_t tx_grid(const comms_ratematch* h, size_t n_frames) {
    return capped_grid((n_frames * (tx_out_bytes(h) / 4) + RM_WG - 1) / RM_WG, h->tx_max_grid);
}
// a workgroup that stages the table walks at least as many values as it staged entries
size_t rx_grid(const comms_ratematch* h, size_t n_frames) {
    const size_t per = h->rx_lds && h->n_coded > RM_WG ? h->n_coded : RM_WG;
    return capped_grid((n_frames * h->n_coded + per - 1) / per, h->rx_max_grid);
}

}  // namespace

extern "C" {

comms_status_t comms_ratematch_create(size_t n_coded, const uint8_t* pattern, size_t pattern_len, size_t cols, const uint32_t* perm,
                                      const void* scramble, size_t record_llrs, int32_t device, comms_ratematch_t** out) {
    COMMS_ARG(out != nullptr, "out is NULL");
    *out = nullptr;
    RmFormat f;
    COMMS_TRY(rm_format(n_coded, pattern, pattern_len, cols, perm, scramble, record_llrs, &f));
    HandlePtr<comms_ratematch> h;
    COMMS_TRY(make_handle(device, &h));
    h->n_coded = f.n_coded;
    h->n_tx = f.n_tx;
    h->record_llrs = f.record_llrs;
    COMMS_HIP_TRY(h->tx_table.upload(f.tx_table));
    COMMS_HIP_TRY(h->scramble.upload(f.scramble));
    COMMS_HIP_TRY(h->rx_table.upload(f.rx_table));
    h->src = std::move(f.src);
    h->tx_lds = h->n_tx <= RM_LDS_SEAM ? f.tx_table.size() * sizeof(unsigned) : 0;
    h->rx_lds = h->n_coded <= RM_LDS_SEAM ? f.rx_table.size() * sizeof(int) : 0;
    h->tx_max_grid = resident_workgroups(h->tx_lds);
    h->rx_max_grid = resident_workgroups(h->rx_lds);
    *out = h.release();
    return COMMS_OK;
}

size_t comms_ratematch_n_tx_bits(const comms_ratematch_t* h) { return h ? h->n_tx : 0; }
size_t comms_ratematch_tx_in_frame_bytes(const comms_ratematch_t* h) { return h ? tx_in_bytes(h) : 0; }
size_t comms_ratematch_tx_out_frame_bytes(const comms_ratematch_t* h) { return h ? tx_out_bytes(h) : 0; }
size_t comms_ratematch_rx_in_frame_bytes(const comms_ratematch_t* h) { return h ? rx_in_bytes(h) : 0; }
size_t comms_ratematch_rx_out_frame_bytes(const comms_ratematch_t* h) { return h ? rx_out_bytes(h) : 0; }

comms_status_t comms_ratematch_get_map(const comms_ratematch_t* h, uint32_t* src, size_t cap) {
    COMMS_ARG(h && src, "NULL argument");
    COMMS_ARG(cap >= h->n_tx, "src must hold the %u transmitted bits (cap %zu)", h->n_tx, cap);
    std::copy(h->src.begin(), h->src.end(), src);
    return COMMS_OK;
}

comms_status_t comms_ratematch_tx_run_dev(comms_ratematch_t* h, const void* d_in, size_t n_frames, void* d_out, void* stream) {
    COMMS_TRY(check_frame_call(h, tx_call, d_in, n_frames, d_out, true));
    if (!n_frames) return COMMS_OK;
    COMMS_TRY(use_device(h->device));
    RmTxArgs a{};
    a.in = static_cast<const unsigned*>(d_in);
    a.out = static_cast<unsigned*>(d_out);
    a.src = h->tx_table.get();
    a.scramble = h->scramble.get();
    a.n_frames = n_frames;
    a.in_words = static_cast<unsigned>(tx_in_bytes(h) / 4);
    a.out_words = static_cast<unsigned>(tx_out_bytes(h) / 4);
    const unsigned last = h->n_tx - 32u * (a.out_words - 1u);   // bits of the record's last word: 1 ... 32 (n_tx <= 32 words' worth)
    a.tail_mask = last >= 32u ? 0xFFFFFFFFu : (1u << last) - 1u;
    const dim3 grid(static_cast<unsigned>(tx_grid(h, n_frames))), wg(RM_WG);
    return h->tx_lds ? launch_kernel<ratematch_tx_kernel<true>>("ratematch_tx_kernel", grid, wg, h->tx_lds, h->pick(stream), h->take_events(), a)
                     : launch_kernel<ratematch_tx_kernel<false>>("ratematch_tx_kernel", grid, wg, 0, h->pick(stream), h->take_events(), a);
}

comms_status_t comms_ratematch_rx_run_dev(comms_ratematch_t* h, const float* d_llr_in, size_t n_frames, float* d_llr_out, void* stream) {
    COMMS_TRY(check_frame_call(h, rx_call, d_llr_in, n_frames, d_llr_out, true));
    if (!n_frames) return COMMS_OK;
    COMMS_TRY(use_device(h->device));
    RmRxArgs a{};
    a.in = reinterpret_cast<const unsigned*>(d_llr_in);
    a.out = reinterpret_cast<unsigned*>(d_llr_out);
    a.inv = h->rx_table.get();
    a.n_frames = n_frames;
    a.record_llrs = h->record_llrs;
    a.n_coded = h->n_coded;
    const dim3 grid(static_cast<unsigned>(rx_grid(h, n_frames))), wg(RM_WG);
    return h->rx_lds ? launch_kernel<ratematch_rx_kernel<true>>("ratematch_rx_kernel", grid, wg, h->rx_lds, h->pick(stream), h->take_events(), a)
                     : launch_kernel<ratematch_rx_kernel<false>>("ratematch_rx_kernel", grid, wg, 0, h->pick(stream), h->take_events(), a);
}

comms_status_t comms_ratematch_tx_run(comms_ratematch_t* h, const void* in, size_t n_frames, void* out) {
    return run_frame_call(h, tx_call, in, n_frames, out,
                          [&](void* d_in, void* d_out) { return comms_ratematch_tx_run_dev(h, d_in, n_frames, d_out, COMMS_STREAM_HANDLE); });
}

comms_status_t comms_ratematch_rx_run(comms_ratematch_t* h, const float* llr_in, size_t n_frames, float* llr_out) {
    return run_frame_call(h, rx_call, llr_in, n_frames, llr_out, [&](void* d_in, void* d_out) {
        return comms_ratematch_rx_run_dev(h, static_cast<const float*>(d_in), n_frames, static_cast<float*>(d_out), COMMS_STREAM_HANDLE);
    });
}

comms_status_t comms_ratematch_get_kernel(const comms_ratematch_t* h, int32_t direction, size_t n_frames, char* name, size_t name_len) {
    COMMS_ARG(h && name && name_len, "NULL argument");
    COMMS_ARG(direction == COMMS_RATEMATCH_TX || direction == COMMS_RATEMATCH_RX, "direction must be COMMS_RATEMATCH_TX or COMMS_RATEMATCH_RX (got %d)",
              direction);
    if (direction == COMMS_RATEMATCH_TX)
        std::snprintf(name, name_len, "ratematch_tx_kernel wg=%d table=%s seam=%u n_coded=%u n_tx=%u words=%zu grid=%zu max_grid=%u lds=%zu", RM_WG,
                      h->tx_lds ? "lds" : "global", RM_LDS_SEAM, h->n_coded, h->n_tx, n_frames * (tx_out_bytes(h) / 4), tx_grid(h, n_frames),
                      h->tx_max_grid, h->tx_lds);
    else
        std::snprintf(name, name_len, "ratematch_rx_kernel wg=%d table=%s seam=%u n_coded=%u n_tx=%u values=%zu grid=%zu max_grid=%u lds=%zu", RM_WG,
                      h->rx_lds ? "lds" : "global", RM_LDS_SEAM, h->n_coded, h->n_tx, n_frames * h->n_coded, rx_grid(h, n_frames), h->rx_max_grid,
                      h->rx_lds);
    return COMMS_OK;
}

comms_status_t comms_ratematch_set_timer(comms_ratematch_t* h, comms_timer_t* t) { return set_handle_timer(h, t); }

comms_status_t comms_ratematch_destroy(comms_ratematch_t* h) { return destroy_handle(h); }

}  // extern "C"
