// crc.hip -- the frame check: a W-bit CRC attached to every frame (crc_attach_kernel) and checked behind the decoder
// (crc_check_kernel), every frame of a call by ONE launch each.
//
// The reference has no such block; the contract is include/comms_hip.h's ("frame check (CRC)"), a bit-serial register, and
// tests/crc_ref.py restates it.  The kernels do not run that register: a CRC is linear, the frame length is fixed per handle,
// and so everything that depends on a bit's position is a constant the host builds at create (crc_tables.hpp, which also
// derives the combination and whose crc_combine is these kernels' arithmetic on the host).
//   lane     one 32-bit word of a record, by a coalesced load: the bits beyond T masked off, the word bit-reversed (records are
//            LSB first, the register takes the high coefficient first) and multiplied mod P by the power of x that belongs to
//            its distance from the end of the payload: 32 shift-and-xor steps in registers, gfx950 has no carry-less multiply.
//            The multiplier is one table word per lane, read once per launch.
//   group    G lanes serve a frame, G the smallest power of two >= the words of a payload record, at most 64; their products
//            XOR-reduce by cross-lane swaps, no LDS.  A wave therefore holds 64 / G frames side by side.  A payload of more than
//            64 words is walked in chunks of 64 that end at its last word: acc = acc * x^(32 * 64) + chunk over all chunks but
//            the last, which has multipliers of its own (crc_tables.hpp says why).
//   attach   the same lanes copy the payload words; the lane of the last payload word splices the W bits in, across the word
//            boundary where they cross it.
//   check    the lanes write the stripped payload; the lane of the last payload word takes the received W bits from its word
//            and the next and compares; one atomic add per wave carries the failed frames of everything the wave walked.
// Both directions walk wave-items (64 / G frames) grid-stride under the library's grid cap.  No LDS, no scratch.
#include "common.hpp"
#include "crc_tables.hpp"

namespace comms {

constexpr int CRC_WG = 256;
constexpr int CRC_WAVES = CRC_WG / 64;
constexpr size_t CRC_MAX_FRAMES = (size_t(1) << 32) - 1;   // the failed frames of a call fit the 32-bit counter

struct CrcArgs {
    const unsigned* in;       // records of in_words words
    unsigned* out;            // attach: records of cw words; check: records of np words, or NULL
    int* pass;                // check only, each may be NULL
    unsigned* crc;
    unsigned* n_failed;
    const unsigned* mult;     // CrcPlan::mult
    size_t n_frames;
    unsigned T, np, cw, s, tail_shift, sh, rounds;
    unsigned polyL, strideL, finalL, mask;
};

template <int G>
__device__ __forceinline__ unsigned group_xor(unsigned v) {
#pragma unroll
    for (int s = G / 2; s >= 1; s >>= 1) v ^= static_cast<unsigned>(__shfl_xor(static_cast<int>(v), s));
    return v;
}

template <int G, bool CHECK>
__device__ __forceinline__ void crc_frames(const CrcArgs& a) {
    constexpr unsigned FPW = 64u / G;                    // frames a wave holds side by side
    const unsigned lane = threadIdx.x & 63u, j = lane & (G - 1u), slot = lane / G;
    const size_t n_waves = static_cast<size_t>(gridDim.x) * CRC_WAVES;
    const size_t items = (a.n_frames + FPW - 1) / FPW;
    const unsigned in_words = CHECK ? a.cw : a.np, out_words = CHECK ? a.np : a.cw;
    const unsigned mL0 = a.mult[G - 1u - j];                                  // the last chunk's, and the earlier chunks'
    const unsigned mL1 = a.rounds > 1u ? a.mult[CRC_MAX_GROUP + G - 1u - j] : 0u;
    unsigned failed = 0;                                 // wave-uniform
    // every branch around a cross-lane swap is wave-uniform: `it`, the rounds; the lanes of a frame past the end idle inside
    for (size_t it = static_cast<size_t>(blockIdx.x) * CRC_WAVES + threadIdx.x / 64u; it < items; it += n_waves) {
        const size_t frame = it * FPW + slot;
        const bool live = frame < a.n_frames;
        const unsigned* rec = a.in + frame * in_words;
        unsigned* orec = a.out ? a.out + frame * out_words : nullptr;   // (the check's payload may be NULL)
        unsigned acc = 0, word = 0, data = 0;
        for (unsigned c = a.rounds; c-- > 0;) {
            const int w = static_cast<int>(a.np) - G * static_cast<int>(c + 1u) + static_cast<int>(j);   // below np
            const bool mine = live && w >= 0;
            word = mine ? rec[w] : 0u;
            const int nbits = static_cast<int>(a.T) - 32 * w;                                             // above 0
            data = nbits >= 32 ? word : word & ((1u << nbits) - 1u);
            // the last payload word is written behind the loop: attach splices into it
            if (orec && mine && (CHECK || w + 1 < static_cast<int>(a.np))) orec[w] = data;
            unsigned v = __brev(data);
            if (w + 1 == static_cast<int>(a.np)) v >>= a.tail_shift;
            const unsigned chunk = group_xor<G>(crc_mul(v, c ? mL1 : mL0, a.polyL));
            acc = (c && c + 1u < a.rounds ? crc_mul(acc >> a.sh, a.strideL, a.polyL) : acc) ^ chunk;
        }
        const unsigned crcL = acc ^ a.finalL;
        const unsigned tail = __brev(crcL);              // the attached bits in stream order: W low bits, the rest 0
        // lane G - 1 holds the last payload word, np - 1, of the last chunk in `word` and `data`; the attached bits start at bit s
        // of it, or fill word np from bit 0 where s = 0, and reach into word np where cw > np
        const bool last = live && j == G - 1u;
        if (CHECK) {
            bool bad = false;
            if (last) {
                const unsigned next = a.cw > a.np ? rec[a.np] : 0u;
                const unsigned rx = a.s ? (word >> a.s) | (next << (32u - a.s)) : next;
                bad = ((rx ^ tail) & a.mask) != 0u;
                if (a.pass) a.pass[frame] = bad ? 0 : 1;
                if (a.crc) a.crc[frame] = crcL >> a.sh;
            }
            failed += static_cast<unsigned>(__popcll(__ballot(bad)));
        } else if (last) {
            orec[a.np - 1u] = a.s ? data | (tail << a.s) : data;
            if (a.cw > a.np) orec[a.np] = a.s ? tail >> (32u - a.s) : tail;
        }
    }
    if (CHECK && a.n_failed && failed && lane == 0u) atomicAdd(a.n_failed, failed);
}

template <int G>
__global__ __launch_bounds__(CRC_WG) void crc_attach_kernel(const CrcArgs a) {
    crc_frames<G, false>(a);
}
template <int G>
__global__ __launch_bounds__(CRC_WG) void crc_check_kernel(const CrcArgs a) {
    crc_frames<G, true>(a);
}

}  // namespace comms

using namespace comms;

struct comms_crc : Handle {
    CrcPlan plan;
    DevBuf<unsigned> mult;
    unsigned max_grid = 1;
};
static_assert(!std::is_copy_constructible_v<comms_crc>, "a handle is never copied");

namespace {

size_t payload_bytes(const comms_crc* h) { return bit_record_bytes(h->plan.T); }
size_t coded_bytes(const comms_crc* h) { return bit_record_bytes(static_cast<size_t>(h->plan.T) + h->plan.W); }

size_t crc_grid(const comms_crc* h, size_t n_frames) {
    const size_t fpw = 64 / h->plan.group, items = (n_frames + fpw - 1) / fpw;
    return capped_grid((items + CRC_WAVES - 1) / CRC_WAVES, h->max_grid);
}

FrameCall attach_call(const comms_crc* h) { return {payload_bytes(h), coded_bytes(h), 4, 4, CRC_MAX_FRAMES}; }
// the coded records and the stripped payload, which a caller may leave out; the other outputs are the check's own
FrameCall check_call(const comms_crc* h, const void* payload) { return {coded_bytes(h), payload ? payload_bytes(h) : 0, 4, 4, CRC_MAX_FRAMES}; }

template <int G, bool CHECK>
comms_status_t crc_launch_group(comms_crc* h, const CrcArgs& a, hipStream_t s) {
    const dim3 grid(static_cast<unsigned>(crc_grid(h, a.n_frames))), wg(CRC_WG);
    if (CHECK) return launch_kernel<crc_check_kernel<G>>("crc_check_kernel", grid, wg, 0, s, h->take_events(), a);
    return launch_kernel<crc_attach_kernel<G>>("crc_attach_kernel", grid, wg, 0, s, h->take_events(), a);
}

template <bool CHECK>
comms_status_t crc_launch(comms_crc* h, const CrcArgs& a, hipStream_t s) {
    switch (h->plan.group) {
        case 1: return crc_launch_group<1, CHECK>(h, a, s);
        case 2: return crc_launch_group<2, CHECK>(h, a, s);
        case 4: return crc_launch_group<4, CHECK>(h, a, s);
        case 8: return crc_launch_group<8, CHECK>(h, a, s);
        case 16: return crc_launch_group<16, CHECK>(h, a, s);
        case 32: return crc_launch_group<32, CHECK>(h, a, s);
        default: return crc_launch_group<64, CHECK>(h, a, s);
    }
}

CrcArgs crc_args(const comms_crc* h, const void* in, size_t n_frames) {
    const CrcPlan& p = h->plan;
    CrcArgs a{};
    a.in = static_cast<const unsigned*>(in);
    a.mult = h->mult.get();
    a.n_frames = n_frames;
    a.T = p.T;
    a.np = p.np;
    a.cw = p.cw;
    a.s = p.s;
    a.tail_shift = p.tail_shift;
    a.sh = p.sh;
    a.rounds = p.rounds;
    a.polyL = p.polyL;
    a.strideL = p.strideL;
    a.finalL = p.finalL;
    a.mask = p.mask;
    return a;
}

}  // namespace

extern "C" {

comms_status_t comms_crc_create(int32_t width, uint32_t poly, uint32_t init, uint32_t xorout, size_t n_payload_bits, int32_t device,
                                comms_crc_t** out) {
    COMMS_ARG(out != nullptr, "out is NULL");
    *out = nullptr;
    COMMS_ARG(width >= 1 && width <= 32, "a CRC has 1 <= width <= 32 bits (got %d)", width);
    const uint64_t lim = uint64_t(1) << width;
    COMMS_ARG(poly < lim && init < lim && xorout < lim, "poly, init and xorout must be below 2^width (got 0x%X, 0x%X, 0x%X at width %d)", poly,
              init, xorout, width);
    COMMS_ARG(n_payload_bits >= 1 && n_payload_bits <= CRC_MAX_BITS && n_payload_bits + static_cast<size_t>(width) <= CRC_MAX_BITS,
              "a frame has 1 <= n_payload_bits and n_payload_bits + width <= 2^16 (got %zu + %d)", n_payload_bits, width);
    HandlePtr<comms_crc> h;
    COMMS_TRY(make_handle(device, &h));
    h->plan = crc_plan(static_cast<unsigned>(width), poly, init, xorout, static_cast<unsigned>(n_payload_bits));
    COMMS_HIP_TRY(h->mult.upload(h->plan.mult, 2 * CRC_MAX_GROUP));
    h->max_grid = resident_workgroups(0);
    *out = h.release();
    return COMMS_OK;
}

size_t comms_crc_payload_frame_bytes(const comms_crc_t* h) { return h ? payload_bytes(h) : 0; }
size_t comms_crc_coded_frame_bytes(const comms_crc_t* h) { return h ? coded_bytes(h) : 0; }

comms_status_t comms_crc_attach_run_dev(comms_crc_t* h, const void* d_in, size_t n_frames, void* d_out, void* stream) {
    COMMS_TRY(check_frame_call(h, attach_call, d_in, n_frames, d_out, true));
    if (!n_frames) return COMMS_OK;
    COMMS_TRY(use_device(h->device));
    CrcArgs a = crc_args(h, d_in, n_frames);
    a.out = static_cast<unsigned*>(d_out);
    return crc_launch<false>(h, a, h->pick(stream));
}

comms_status_t comms_crc_check_run_dev(comms_crc_t* h, const void* d_in, size_t n_frames, void* d_payload, int32_t* d_pass, uint32_t* d_crc,
                                       uint32_t* d_n_failed, void* stream) {
    COMMS_TRY(check_frame_call(h, [&](const comms_crc* c) { return check_call(c, d_payload); }, d_in, n_frames, d_payload, true));
    COMMS_ARG(aligned(d_pass, 4) && aligned(d_crc, 4) && aligned(d_n_failed, 4), "the device pointers must be aligned to 4 bytes");
    if (!n_frames) return COMMS_OK;
    const size_t in_bytes = n_frames * coded_bytes(h);
    COMMS_ARG(!(d_pass && ranges_overlap(d_in, in_bytes, d_pass, n_frames * sizeof(int32_t))) &&
                  !(d_crc && ranges_overlap(d_in, in_bytes, d_crc, n_frames * sizeof(uint32_t))) &&
                  !(d_n_failed && ranges_overlap(d_in, in_bytes, d_n_failed, sizeof(uint32_t))),
              "the input records and an output overlap");
    {
        const void* outs[4] = {d_payload, d_pass, d_crc, d_n_failed};
        const size_t bytes[4] = {n_frames * payload_bytes(h), n_frames * sizeof(int32_t), n_frames * sizeof(uint32_t), sizeof(uint32_t)};
        for (int i = 0; i < 4; ++i)
            for (int k = i + 1; k < 4; ++k)
                COMMS_ARG(!(outs[i] && outs[k] && ranges_overlap(outs[i], bytes[i], outs[k], bytes[k])), "two outputs overlap");
    }
    COMMS_TRY(use_device(h->device));
    CrcArgs a = crc_args(h, d_in, n_frames);
    a.out = static_cast<unsigned*>(d_payload);
    a.pass = d_pass;
    a.crc = d_crc;
    a.n_failed = d_n_failed;
    return crc_launch<true>(h, a, h->pick(stream));
}

comms_status_t comms_crc_attach_run(comms_crc_t* h, const void* in, size_t n_frames, void* out) {
    return run_frame_call(h, attach_call, in, n_frames, out,
                          [&](void* d_in, void* d_out) { return comms_crc_attach_run_dev(h, d_in, n_frames, d_out, COMMS_STREAM_HANDLE); });
}

comms_status_t comms_crc_check_run(comms_crc_t* h, const void* in, size_t n_frames, void* payload, int32_t* pass, uint32_t* crc,
                                   size_t* n_failed) {
    COMMS_TRY(check_frame_call(h, [&](const comms_crc* c) { return check_call(c, payload); }, in, n_frames, payload, false));
    if (n_failed) *n_failed = 0;
    if (!n_frames) return COMMS_OK;
    COMMS_TRY(use_device(h->device));
    // one device block for the outputs: the payload records, the flags, the crcs, the counter
    const size_t pay_b = n_frames * payload_bytes(h), col_b = n_frames * sizeof(uint32_t);
    COMMS_TRY(h->in_scratch.reserve(n_frames * coded_bytes(h)));
    COMMS_TRY(h->out_scratch.reserve(pay_b + 2 * col_b + sizeof(uint32_t)));
    char* d_out = static_cast<char*>(h->out_scratch.p);
    int32_t* d_pass = reinterpret_cast<int32_t*>(d_out + pay_b);
    uint32_t* d_crc = reinterpret_cast<uint32_t*>(d_out + pay_b + col_b);
    uint32_t* d_count = reinterpret_cast<uint32_t*>(d_out + pay_b + 2 * col_b);
    uint32_t count = 0;
    COMMS_HIP_TRY(hipMemcpyAsync(h->in_scratch.p, in, n_frames * coded_bytes(h), hipMemcpyHostToDevice, h->stream));
    if (n_failed) COMMS_HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(uint32_t), h->stream));
    COMMS_TRY(comms_crc_check_run_dev(h, h->in_scratch.p, n_frames, payload ? d_out : nullptr, pass ? d_pass : nullptr, crc ? d_crc : nullptr,
                                      n_failed ? d_count : nullptr, COMMS_STREAM_HANDLE));
    if (payload) COMMS_HIP_TRY(hipMemcpyAsync(payload, d_out, pay_b, hipMemcpyDeviceToHost, h->stream));
    if (pass) COMMS_HIP_TRY(hipMemcpyAsync(pass, d_pass, col_b, hipMemcpyDeviceToHost, h->stream));
    if (crc) COMMS_HIP_TRY(hipMemcpyAsync(crc, d_crc, col_b, hipMemcpyDeviceToHost, h->stream));
    if (n_failed) COMMS_HIP_TRY(hipMemcpyAsync(&count, d_count, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    COMMS_HIP_TRY(hipStreamSynchronize(h->stream));
    if (n_failed) *n_failed = count;
    return COMMS_OK;
}

comms_status_t comms_crc_get_kernel(const comms_crc_t* h, int32_t direction, size_t n_frames, char* name, size_t name_len) {
    COMMS_ARG(h && name && name_len, "NULL argument");
    COMMS_ARG(direction == COMMS_CRC_ATTACH || direction == COMMS_CRC_CHECK, "direction must be COMMS_CRC_ATTACH or COMMS_CRC_CHECK (got %d)",
              direction);
    std::snprintf(name, name_len, "%s wg=%d group=%u rounds=%u width=%u words=%zu frames=%zu grid=%zu max_grid=%u lds=0",
                  direction == COMMS_CRC_ATTACH ? "crc_attach_kernel" : "crc_check_kernel", CRC_WG, h->plan.group, h->plan.rounds, h->plan.W,
                  n_frames * h->plan.cw, n_frames, crc_grid(h, n_frames), h->max_grid);
    return COMMS_OK;
}

comms_status_t comms_crc_set_timer(comms_crc_t* h, comms_timer_t* t) { return set_handle_timer(h, t); }

comms_status_t comms_crc_destroy(comms_crc_t* h) { return destroy_handle(h); }

}  // extern "C"
