// ldpc.hip -- quasi-cyclic LDPC coding: the dual-diagonal encoder (ldpc_encode_kernel) and the layered normalised min-sum
// decoder (ldpc_decode_kernel) of one base matrix, every frame of a call by ONE launch each.
//
// The reference has no such blocks; the contract is include/comms_hip.h's ("LDPC code", "LDPC encoder", "LDPC decoder").  In
// short: entry b >= 0 of block (i, j) makes check z of block row i touch variable j Z + (z + b) mod Z; the decoder walks the
// block rows in order, per check  Q_e = P_v - R_e,  m1 / idx / m2 over |clamp(Q_e, +-127)|,  par = XOR (Q_e < 0),
// |R_e'| = (a * (e == idx ? m2 : m1)) >> 4 with the sign par ^ (Q_e < 0),  P_v = Q_e + R_e',  and stops a frame after the
// first iteration whose hard decisions satisfy every check.  Everything is integer once the LLRs are quantised, so the bits
// and statuses are those of tests/ldpc_ref.py exactly.
//
// Both kernels: ONE WAVE PER FRAME, lanes over the z of the current block row (Z <= 64: one partial or full pass, Z > 64:
// two; lanes beyond Z shadow the last check and store nothing), frames_per_wg waves per workgroup that meet once, at the barrier behind the copy of the edge table into LDS.  The
// grids are sized by the work, ceil(n_frames / frames_per_wg) workgroups, not persistent loops under the library's grid cap:
// a frame's state is tens of KiB of LDS that a wave sets up per frame anyway, so a resident wave that loops over frames
// saves only its dispatch, while a grid of the work lets the dispatcher refill a CU the moment a workgroup of early-exit
// frames ends -- frames of one call run from 1 to max_iters iterations.
//   * the edge table: per block row LD_ROW words (column j Z | shift << 16, LD_NONE behind the last edge).  A layer's words
//     are read into lanes 0 ... 31 by one LDS read, and edge e is taken by v_readlane: the column and the shift are scalars.
//   * ldpc_decode_kernel: P as int16 (2 N bytes) and per check ONE 8-byte record {m1', m2', idx, sign mask of <= 32 edges}
//     (8 M bytes) from which R_e is recomputed exactly: |R_e| = e == idx ? m2' : m1' (already scaled), negative iff bit e.
//     A check makes two passes over its edges: the first finds m1, m2, idx and the signs from P_v - R_e, the second reads P_v
//     again (four edges' reads in flight before their stores) and writes P_v - R_e + R_e'.  The stopping test reads every
//     P_v once more per iteration, a lane ORs (never sums) the parities of its checks of the two passes, and it leaves at the
//     first block row with an unsatisfied check.  No device workspace: a
//     handle is not tied to one stream.
//   * ldpc_encode_kernel: the coded bits of a frame as N bytes of LDS.  lambda_i[z] goes to where p_{i+1}[z] will stand, the
//     sum over i to p_0[(z + t) mod Z]; then each lane runs down its own z: p_{i+1} = lambda_i ^ p_i (^ the sum in row r).
//   * output words: a 64-bit ballot per 64 bits, kept by lane (chunk mod 64) and stored 64 chunks at a time.
// Wave-private LDS needs no barrier (a wave's LDS operations complete in order); wave_sync() keeps the compiler from moving
// one lane's read over another lane's write.
#include <cmath>
#include <vector>

#include "common.hpp"

namespace comms {

constexpr int LD_MAX_MB = 32, LD_MAX_NB = 64, LD_MAX_Z = 128;
constexpr int LD_ROW = 32;                         // edges of a block row at most: the sign mask's width, and the table's row stride
constexpr int LD_WAVES = 4;                        // frames (waves) per workgroup at most
constexpr size_t LD_WG_LDS = 64 * 1024;            // a decoder workgroup's LDS stays under this unless one frame alone exceeds it
constexpr unsigned LD_NONE = 0xFFFFFFFFu;
constexpr size_t LD_MAX_GRID = 0x7FFFFFFF;

struct LdpcCode {
    int mb = 0, nb = 0, Z = 0;
    unsigned N = 0, M = 0, T = 0, edges = 0;
    unsigned r = 0, s = 0, t = 0;                  // the encoder's column kb: s in rows 0 and mb-1, t in row r
    std::vector<unsigned> table;                   // mb * LD_ROW words
};

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// The variable that edge word `en` gives check z
__device__ __forceinline__ unsigned ld_var(unsigned en, unsigned z, unsigned Z) {
    const unsigned t = z + (en >> 16);
    return (en & 0xFFFFu) + (t >= Z ? t - Z : t);
}

// The frame's edge table from device memory into the front of the workgroup's LDS; the only barrier of either kernel
__device__ __forceinline__ void ld_table(unsigned* tab, const unsigned* table, unsigned mb) {
    for (unsigned k = threadIdx.x; k < mb * LD_ROW; k += blockDim.x) tab[k] = table[k];
    __syncthreads();
}

// Bits 0 ... n_bits-1 given by bit(v), and zeros up to 32 out_words, as the words of one record
template <class B>
__device__ __forceinline__ void ld_pack(unsigned lane, unsigned n_bits, unsigned out_words, unsigned* out, B&& bit) {
    const unsigned chunks = (out_words + 1u) / 2u;
    unsigned long long keep = 0;
    for (unsigned c = 0; c < chunks; ++c) {
        const unsigned v = 64u * c + lane;
        const unsigned long long m = __ballot(v < n_bits && bit(v));
        keep = lane == (c & 63u) ? m : keep;
        if ((c & 63u) == 63u || c + 1u == chunks) {
            const unsigned w = 2u * ((c & ~63u) + lane);
            if (w < out_words) out[w] = static_cast<unsigned>(keep);
            if (w + 1u < out_words) out[w + 1u] = static_cast<unsigned>(keep >> 32);
        }
    }
}

struct LeArgs {
    const unsigned* in;
    unsigned* out;
    const unsigned* table;
    size_t n_frames;
    unsigned mb, Z, N, T, in_words, out_words, r, s, t, frame_lds;
};

__global__ __launch_bounds__(64 * LD_WAVES) void ldpc_encode_kernel(const LeArgs a) {
    extern __shared__ __align__(16) unsigned le_lds[];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    ld_table(le_lds, a.table, a.mb);
    const size_t f = static_cast<size_t>(blockIdx.x) * (blockDim.x >> 6) + wave;
    if (f >= a.n_frames) return;                                  // wave-uniform, behind the barrier
    unsigned char* const c = reinterpret_cast<unsigned char*>(le_lds + a.mb * LD_ROW) + wave * a.frame_lds;   // the N coded bits
    const unsigned* in = a.in + f * a.in_words;
    const unsigned Z = a.Z, T = a.T;
    for (unsigned v = lane; v < T; v += 64u) c[v] = static_cast<unsigned char>((in[v >> 5] >> (v & 31u)) & 1u);   // bits from T on do not count
    wave_sync();
    unsigned sum[2] = {0u, 0u};
    for (unsigned i = 0; i < a.mb; ++i) {
        const unsigned ent = le_lds[i * LD_ROW + (lane & 31u)];
        const unsigned deg = static_cast<unsigned>(__popcll(__ballot(lane < 32u && ent != LD_NONE)));
#pragma unroll
        for (unsigned pz = 0; pz < 2; ++pz) {
            const bool live = lane + 64u * pz < Z;
            const unsigned z = live ? lane + 64u * pz : Z - 1u;   // lanes beyond Z shadow the last z and store nothing: the
            unsigned lam = 0;                                     // v_readlane of `ent` runs with all lanes active
            for (unsigned e = 0; e < deg; ++e) {
                const unsigned en = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(ent), static_cast<int>(e)));
                if ((en & 0xFFFFu) < T) lam ^= c[ld_var(en, z, Z)];          // the information columns
            }
            sum[pz] ^= lam;
            if (live && i + 1u < a.mb) c[T + (i + 1u) * Z + z] = static_cast<unsigned char>(lam);
        }
    }
#pragma unroll
    for (unsigned pz = 0; pz < 2; ++pz) {
        const unsigned z = lane + 64u * pz;
        if (z < Z) c[T + ld_var(a.t << 16, z, Z)] = static_cast<unsigned char>(sum[pz]);   // p_0[(z + t) mod Z]
    }
    wave_sync();
#pragma unroll
    for (unsigned pz = 0; pz < 2; ++pz) {
        const unsigned z = lane + 64u * pz;
        if (z < Z) {
            unsigned p = c[T + Z + z] ^ c[T + ld_var(a.s << 16, z, Z)];               // p_1 = lambda_0 ^ p_0[(z + s) mod Z]
            c[T + Z + z] = static_cast<unsigned char>(p);
            for (unsigned i = 1; i + 1u < a.mb; ++i) {
                p ^= c[T + (i + 1u) * Z + z] ^ (i == a.r ? sum[pz] : 0u);
                c[T + (i + 1u) * Z + z] = static_cast<unsigned char>(p);
            }
        }
    }
    wave_sync();
    ld_pack(lane, a.N, a.out_words, a.out + f * a.out_words, [&](unsigned v) { return c[v] != 0; });
}

struct LdArgs {
    const float* llr;
    unsigned* bits;
    int* status;                   // may be null
    const unsigned* table;
    size_t n_frames, record_llrs;
    unsigned mb, Z, N, M, T, out_words, max_iters, norm16, frame_lds, p_bytes;
    float qscale;
};

__global__ __launch_bounds__(64 * LD_WAVES) void ldpc_decode_kernel(const LdArgs a) {
    extern __shared__ __align__(16) unsigned ld_lds[];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    ld_table(ld_lds, a.table, a.mb);
    const size_t f = static_cast<size_t>(blockIdx.x) * (blockDim.x >> 6) + wave;
    if (f >= a.n_frames) return;                                  // wave-uniform, behind the barrier
    char* const mine = reinterpret_cast<char*>(ld_lds + a.mb * LD_ROW) + wave * a.frame_lds;
    short* const P = reinterpret_cast<short*>(mine);
    uint2* const rec = reinterpret_cast<uint2*>(mine + a.p_bytes);
    const unsigned Z = a.Z;
    const float* L = a.llr + f * a.record_llrs;
#pragma unroll 4
    for (unsigned v = lane; v < a.N; v += 64u) P[v] = static_cast<short>(quantise_llr(L[v], a.qscale));
    for (unsigned k = lane; k < a.M; k += 64u) rec[k] = make_uint2(0u, 0u);          // every R_e = 0
    wave_sync();
    int status = -static_cast<int>(a.max_iters);
    for (unsigned it = 1; it <= a.max_iters; ++it) {
        for (unsigned i = 0; i < a.mb; ++i) {
            const unsigned ent = ld_lds[i * LD_ROW + (lane & 31u)];
            const unsigned deg = static_cast<unsigned>(__popcll(__ballot(lane < 32u && ent != LD_NONE)));
            const unsigned all = deg >= 32u ? 0xFFFFFFFFu : (1u << deg) - 1u;
            for (unsigned z0 = 0; z0 < Z; z0 += 64u) {   // a uniform loop: every v_readlane of `ent` runs with all lanes active
                const bool live = z0 + lane < Z;
                const unsigned z = live ? z0 + lane : Z - 1u;                        // lanes beyond Z shadow the last check and store nothing
                const unsigned k = i * Z + z;
                const uint2 old = rec[k];
                const int o1 = static_cast<int>(old.x & 0xFFu), o2 = static_cast<int>((old.x >> 8) & 0xFFu);
                const unsigned oidx = (old.x >> 16) & 0xFFu, oneg = old.y;
                auto edge = [&](unsigned e) { return static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(ent), static_cast<int>(e))); };
                auto r_old = [&](unsigned e) {
                    const int mag = e == oidx ? o2 : o1;
                    return (oneg >> e) & 1u ? -mag : mag;
                };
                int m1 = 255, m2 = 255;
                unsigned idx = 0, neg = 0;
                for (unsigned e0 = 0; e0 < deg; e0 += 4u) {                          // four reads in flight
                    int p[4] = {0, 0, 0, 0};
#pragma unroll
                    for (unsigned j = 0; j < 4; ++j)
                        if (e0 + j < deg) p[j] = P[ld_var(edge(e0 + j), z, Z)];
#pragma unroll
                    for (unsigned j = 0; j < 4; ++j)
                        if (e0 + j < deg) {
                            const unsigned e = e0 + j;
                            const int q = p[j] - r_old(e);
                            const int aq = q < 0 ? -q : q;
                            const int ac = aq > 127 ? 127 : aq;
                            neg |= static_cast<unsigned>(q < 0) << e;
                            const bool first = ac < m1;                              // strictly: idx is the FIRST edge at the minimum
                            m2 = first ? m1 : ac < m2 ? ac : m2;
                            idx = first ? e : idx;
                            m1 = first ? ac : m1;
                        }
                }
                const unsigned nneg = __popc(neg) & 1u ? neg ^ all : neg;            // negative iff par ^ (Q_e < 0)
                const int n1 = (static_cast<int>(a.norm16) * m1) >> 4, n2 = (static_cast<int>(a.norm16) * m2) >> 4;
                if (live) rec[k] = make_uint2(static_cast<unsigned>(n1) | static_cast<unsigned>(n2) << 8 | idx << 16, nneg);
                for (unsigned e0 = 0; e0 < deg; e0 += 4u) {                          // four reads in flight, then their stores
                    unsigned v[4] = {0u, 0u, 0u, 0u};
                    int p[4] = {0, 0, 0, 0};
#pragma unroll
                    for (unsigned j = 0; j < 4; ++j)
                        if (e0 + j < deg) {
                            v[j] = ld_var(edge(e0 + j), z, Z);
                            p[j] = P[v[j]];
                        }
#pragma unroll
                    for (unsigned j = 0; j < 4; ++j)
                        if (e0 + j < deg) {
                            const unsigned e = e0 + j;
                            const int mag = e == idx ? n2 : n1;
                            if (live) P[v[j]] = static_cast<short>(p[j] - r_old(e) + ((nneg >> e) & 1u ? -mag : mag));
                        }
                }
            }
            wave_sync();                                                            // the next block row reads what other lanes wrote
        }
        // x_v = (P_v < 0): does every check hold?
        bool ok = true;
        for (unsigned i = 0; i < a.mb && ok; ++i) {
            const unsigned ent = ld_lds[i * LD_ROW + (lane & 31u)];
            const unsigned deg = static_cast<unsigned>(__popcll(__ballot(lane < 32u && ent != LD_NONE)));
            bool bad = false;                                                       // any of the lane's checks, never a sum over them
            for (unsigned z0 = 0; z0 < Z; z0 += 64u) {
                const bool live = z0 + lane < Z;
                const unsigned z = live ? z0 + lane : Z - 1u;
                unsigned odd = 0;
                for (unsigned e0 = 0; e0 < deg; e0 += 4u) {
#pragma unroll
                    for (unsigned j = 0; j < 4; ++j)
                        if (e0 + j < deg) {
                            const unsigned en = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(ent), static_cast<int>(e0 + j)));
                            odd ^= static_cast<unsigned>(P[ld_var(en, z, Z)] < 0);
                        }
                }
                bad = bad || (live && odd != 0u);
            }
            ok = __ballot(bad) == 0ull;
        }
        if (ok) {
            status = static_cast<int>(it);
            break;
        }
    }
    if (a.status != nullptr && lane == 0) a.status[f] = status;
    ld_pack(lane, a.T, a.out_words, a.bits + f * a.out_words, [&](unsigned v) { return P[v] < 0; });
}

// The code of a create call, or COMMS_ERR_ARG: host arithmetic only
inline comms_status_t ldpc_code(int32_t mb, int32_t nb, int32_t Z, const int16_t* base, bool encoder, LdpcCode* out) {
    COMMS_ARG(mb >= 1 && mb <= LD_MAX_MB, "mb must be 1 ... %d block rows (got %d)", LD_MAX_MB, mb);
    COMMS_ARG(nb > mb && nb <= LD_MAX_NB, "nb must be mb < nb <= %d block columns (got %d with mb = %d)", LD_MAX_NB, nb, mb);
    COMMS_ARG(Z >= 2 && Z <= LD_MAX_Z, "Z must be 2 ... %d (got %d)", LD_MAX_Z, Z);
    COMMS_ARG(base != nullptr, "base is NULL");
    LdpcCode c;
    c.mb = mb;
    c.nb = nb;
    c.Z = Z;
    c.N = static_cast<unsigned>(nb * Z);
    c.M = static_cast<unsigned>(mb * Z);
    c.T = c.N - c.M;
    c.table.assign(static_cast<size_t>(mb) * LD_ROW, LD_NONE);
    for (int i = 0; i < mb; ++i) {
        int deg = 0;
        for (int j = 0; j < nb; ++j) {
            const int b = base[i * nb + j];
            COMMS_ARG(b >= -1 && b < Z, "base[%d][%d] must be -1 ... Z-1 = %d (got %d)", i, j, Z - 1, b);
            if (b < 0) continue;
            COMMS_ARG(deg < LD_ROW, "block row %d of base has more than %d entries >= 0", i, LD_ROW);
            c.table[static_cast<size_t>(i) * LD_ROW + deg++] = static_cast<unsigned>(j * Z) | static_cast<unsigned>(b) << 16;
        }
        COMMS_ARG(deg >= 2, "block row %d of base must have at least 2 entries >= 0 (got %d)", i, deg);
        c.edges += static_cast<unsigned>(deg);
    }
    if (encoder) {
        const int kb = nb - mb;
        auto at = [&](int i, int j) { return static_cast<int>(base[i * nb + j]); };
        COMMS_ARG(mb >= 3, "the encoder needs mb >= 3 block rows (got %d)", mb);
        int n_kb = 0, r = 0;
        for (int i = 0; i < mb; ++i)
            if (at(i, kb) >= 0) {
                ++n_kb;
                if (i > 0 && i < mb - 1) r = i;
            }
        COMMS_ARG(n_kb == 3 && at(0, kb) >= 0 && at(mb - 1, kb) >= 0 && r > 0,
                  "base is not of the encoder's form: column kb = %d must have exactly three entries, in rows 0, r and mb-1", kb);
        COMMS_ARG(at(0, kb) == at(mb - 1, kb), "base is not of the encoder's form: base[0][kb] = %d and base[mb-1][kb] = %d must be equal", at(0, kb),
                  at(mb - 1, kb));
        for (int d = 0; d + 1 < mb; ++d)
            for (int i = 0; i < mb; ++i) {
                const int want = i == d || i == d + 1 ? 0 : -1;
                COMMS_ARG(at(i, kb + 1 + d) == want, "base is not of the encoder's form: base[%d][%d] must be %d on the double diagonal (got %d)", i,
                          kb + 1 + d, want, at(i, kb + 1 + d));
            }
        c.r = static_cast<unsigned>(r);
        c.s = static_cast<unsigned>(at(0, kb));
        c.t = static_cast<unsigned>(at(r, kb));
    }
    *out = std::move(c);
    return COMMS_OK;
}

}  // namespace comms

using namespace comms;

struct comms_ldpcenc : Handle {
    LdpcCode code;
    DevBuf<unsigned> table;
    size_t frame_lds = 0;       // bytes of LDS per frame
};
struct comms_ldpcdec : Handle {
    LdpcCode code;
    DevBuf<unsigned> table;
    size_t record_llrs = 0;
    float qscale = 1.0f;
    int max_iters = 0, norm16 = 0;
    int frames_per_wg = 1;
    size_t p_bytes = 0, frame_lds = 0;
};
static_assert(!std::is_copy_constructible_v<comms_ldpcdec> && !std::is_copy_constructible_v<comms_ldpcenc>, "a handle is never copied");

namespace {

size_t table_bytes(const LdpcCode& c) { return static_cast<size_t>(c.mb) * LD_ROW * sizeof(unsigned); }
size_t grid_of(size_t n_frames, int frames_per_wg) { return (n_frames + frames_per_wg - 1) / frames_per_wg; }

size_t enc_lds(const comms_ldpcenc* h) { return table_bytes(h->code) + LD_WAVES * h->frame_lds; }
FrameCall enc_call(const comms_ldpcenc* h) { return {bit_record_bytes(h->code.T), bit_record_bytes(h->code.N), 4, 4, LD_MAX_GRID * LD_WAVES}; }

size_t dec_lds(const comms_ldpcdec* h) { return table_bytes(h->code) + h->frames_per_wg * h->frame_lds; }
// the LLR records and the bit records; the statuses are the decoder's own
FrameCall dec_call(const comms_ldpcdec* h) {
    return {h->record_llrs * sizeof(float), bit_record_bytes(h->code.T), 4, 4, LD_MAX_GRID * static_cast<size_t>(h->frames_per_wg)};
}

}  // namespace

extern "C" {

// ---- encoder
comms_status_t comms_ldpcenc_create(int32_t mb, int32_t nb, int32_t Z, const int16_t* base, int32_t device, comms_ldpcenc_t** out) {
    COMMS_ARG(out != nullptr, "out is NULL");
    *out = nullptr;
    LdpcCode c;
    COMMS_TRY(ldpc_code(mb, nb, Z, base, true, &c));
    HandlePtr<comms_ldpcenc> h;
    COMMS_TRY(make_handle(device, &h));
    COMMS_HIP_TRY(h->table.upload(c.table.data(), c.table.size()));
    h->frame_lds = (c.N + 3u) / 4u * 4u;
    h->code = std::move(c);
    *out = h.release();
    return COMMS_OK;
}

size_t comms_ldpcenc_in_frame_bytes(const comms_ldpcenc_t* h) { return h ? bit_record_bytes(h->code.T) : 0; }
size_t comms_ldpcenc_out_frame_bytes(const comms_ldpcenc_t* h) { return h ? bit_record_bytes(h->code.N) : 0; }

comms_status_t comms_ldpcenc_run_dev(comms_ldpcenc_t* h, const void* d_in, size_t n_frames, void* d_out, void* stream) {
    COMMS_TRY(check_frame_call(h, enc_call, d_in, n_frames, d_out, true));
    if (!n_frames) return COMMS_OK;
    COMMS_TRY(use_device(h->device));
    LeArgs a{};
    a.in = static_cast<const unsigned*>(d_in);
    a.out = static_cast<unsigned*>(d_out);
    a.table = h->table.get();
    a.n_frames = n_frames;
    a.mb = static_cast<unsigned>(h->code.mb);
    a.Z = static_cast<unsigned>(h->code.Z);
    a.N = h->code.N;
    a.T = h->code.T;
    a.in_words = static_cast<unsigned>(bit_record_bytes(h->code.T) / 4);
    a.out_words = static_cast<unsigned>(bit_record_bytes(h->code.N) / 4);
    a.r = h->code.r;
    a.s = h->code.s;
    a.t = h->code.t;
    a.frame_lds = static_cast<unsigned>(h->frame_lds);
    const dim3 grid(static_cast<unsigned>(grid_of(n_frames, LD_WAVES))), wg(64 * LD_WAVES);
    return launch_kernel<ldpc_encode_kernel>("ldpc_encode_kernel", grid, wg, enc_lds(h), h->pick(stream), h->take_events(), a);
}

comms_status_t comms_ldpcenc_run(comms_ldpcenc_t* h, const void* in, size_t n_frames, void* out) {
    return run_frame_call(h, enc_call, in, n_frames, out,
                          [&](void* d_in, void* d_out) { return comms_ldpcenc_run_dev(h, d_in, n_frames, d_out, COMMS_STREAM_HANDLE); });
}

comms_status_t comms_ldpcenc_get_kernel(const comms_ldpcenc_t* h, size_t n_frames, char* name, size_t name_len) {
    COMMS_ARG(h && name && name_len, "NULL argument");
    std::snprintf(name, name_len, "ldpc_encode_kernel wg=%d frames_per_wg=%d Z=%d grid=%zu lds=%zu", 64 * LD_WAVES, LD_WAVES, h->code.Z,
                  grid_of(n_frames, LD_WAVES), enc_lds(h));
    return COMMS_OK;
}

comms_status_t comms_ldpcenc_set_timer(comms_ldpcenc_t* h, comms_timer_t* t) { return set_handle_timer(h, t); }

comms_status_t comms_ldpcenc_destroy(comms_ldpcenc_t* h) { return destroy_handle(h); }

// ---- decoder
comms_status_t comms_ldpcdec_create(int32_t mb, int32_t nb, int32_t Z, const int16_t* base, int32_t max_iters, int32_t norm16,
                                    size_t record_llrs, int32_t device, comms_ldpcdec_t** out) {
    COMMS_ARG(out != nullptr, "out is NULL");
    *out = nullptr;
    LdpcCode c;
    COMMS_TRY(ldpc_code(mb, nb, Z, base, false, &c));
    COMMS_ARG(max_iters >= 1 && max_iters <= 255, "max_iters must be 1 ... 255 (got %d)", max_iters);
    COMMS_ARG(norm16 >= 1 && norm16 <= 16, "norm16 must be 1 ... 16 sixteenths (got %d)", norm16);
    COMMS_ARG(record_llrs == 0 || record_llrs >= c.N, "record_llrs must be 0 or at least N = %u (got %zu)", c.N, record_llrs);
    COMMS_ARG(record_llrs <= (size_t(1) << 32), "record_llrs must be at most 2^32 (got %zu)", record_llrs);
    HandlePtr<comms_ldpcdec> h;
    COMMS_TRY(make_handle(device, &h));
    COMMS_HIP_TRY(h->table.upload(c.table.data(), c.table.size()));
    h->record_llrs = record_llrs ? record_llrs : c.N;
    h->max_iters = max_iters;
    h->norm16 = norm16;
    h->p_bytes = (2 * static_cast<size_t>(c.N) + 7) / 8 * 8;
    h->frame_lds = h->p_bytes + 8 * static_cast<size_t>(c.M);
    // as many frames as fit LD_WG_LDS beside the table, LD_WAVES at most: small workgroups leave the CU's LDS (160 KiB) to be
    // filled by whole workgroups, and a workgroup ends when its slowest frame does
    const size_t fit = (LD_WG_LDS - table_bytes(c)) / h->frame_lds;
    h->frames_per_wg = static_cast<int>(fit < 1 ? 1 : fit > LD_WAVES ? LD_WAVES : fit);
    h->code = std::move(c);
    *out = h.release();
    return COMMS_OK;
}

comms_status_t comms_ldpcdec_set_quant_scale(comms_ldpcdec_t* h, float qscale) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG(std::isfinite(qscale), "qscale must be finite");
    h->qscale = qscale;
    return COMMS_OK;
}

size_t comms_ldpcdec_in_frame_bytes(const comms_ldpcdec_t* h) { return h ? h->record_llrs * sizeof(float) : 0; }
size_t comms_ldpcdec_out_frame_bytes(const comms_ldpcdec_t* h) { return h ? bit_record_bytes(h->code.T) : 0; }

comms_status_t comms_ldpcdec_run_dev(comms_ldpcdec_t* h, const float* d_llr, size_t n_frames, void* d_bits, int32_t* d_status, void* stream) {
    COMMS_TRY(check_frame_call(h, dec_call, d_llr, n_frames, d_bits, true));
    COMMS_ARG(aligned(d_status, 4), "d_status must be aligned to 4 bytes");
    COMMS_ARG(!d_status || !n_frames ||
                  (!ranges_overlap(d_status, n_frames * sizeof(int32_t), d_llr, n_frames * dec_call(h).in_bytes) &&
                   !ranges_overlap(d_status, n_frames * sizeof(int32_t), d_bits, n_frames * dec_call(h).out_bytes)),
              "d_status overlaps the LLR records or the bit records");
    if (!n_frames) return COMMS_OK;
    COMMS_TRY(use_device(h->device));
    LdArgs a{};
    a.llr = d_llr;
    a.bits = static_cast<unsigned*>(d_bits);
    a.status = d_status;
    a.table = h->table.get();
    a.n_frames = n_frames;
    a.record_llrs = h->record_llrs;
    a.mb = static_cast<unsigned>(h->code.mb);
    a.Z = static_cast<unsigned>(h->code.Z);
    a.N = h->code.N;
    a.M = h->code.M;
    a.T = h->code.T;
    a.out_words = static_cast<unsigned>(bit_record_bytes(h->code.T) / 4);
    a.max_iters = static_cast<unsigned>(h->max_iters);
    a.norm16 = static_cast<unsigned>(h->norm16);
    a.frame_lds = static_cast<unsigned>(h->frame_lds);
    a.p_bytes = static_cast<unsigned>(h->p_bytes);
    a.qscale = h->qscale;
    const dim3 grid(static_cast<unsigned>(grid_of(n_frames, h->frames_per_wg))), wg(64u * static_cast<unsigned>(h->frames_per_wg));
    return launch_kernel<ldpc_decode_kernel>("ldpc_decode_kernel", grid, wg, dec_lds(h), h->pick(stream), h->take_events(), a);
}

comms_status_t comms_ldpcdec_run(comms_ldpcdec_t* h, const float* llr, size_t n_frames, void* bits, int32_t* status) {
    COMMS_TRY(check_frame_call(h, dec_call, llr, n_frames, bits, false));
    const size_t in_b = dec_call(h).in_bytes, out_b = dec_call(h).out_bytes;
    if (!n_frames) return COMMS_OK;
    COMMS_TRY(use_device(h->device));
    // the records, then the statuses, in one device block
    const size_t bits_bytes = n_frames * out_b;
    COMMS_TRY(h->in_scratch.reserve(n_frames * in_b));
    COMMS_TRY(h->out_scratch.reserve(bits_bytes + n_frames * sizeof(int32_t)));
    char* d_out = static_cast<char*>(h->out_scratch.p);
    int32_t* d_status = status ? reinterpret_cast<int32_t*>(d_out + bits_bytes) : nullptr;
    COMMS_HIP_TRY(hipMemcpyAsync(h->in_scratch.p, llr, n_frames * in_b, hipMemcpyHostToDevice, h->stream));
    COMMS_TRY(comms_ldpcdec_run_dev(h, static_cast<const float*>(h->in_scratch.p), n_frames, d_out, d_status, COMMS_STREAM_HANDLE));
    COMMS_HIP_TRY(hipMemcpyAsync(bits, d_out, bits_bytes, hipMemcpyDeviceToHost, h->stream));
    if (status) COMMS_HIP_TRY(hipMemcpyAsync(status, d_status, n_frames * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    COMMS_HIP_TRY(hipStreamSynchronize(h->stream));
    return COMMS_OK;
}

comms_status_t comms_ldpcdec_get_kernel(const comms_ldpcdec_t* h, size_t n_frames, char* name, size_t name_len) {
    COMMS_ARG(h && name && name_len, "NULL argument");
    std::snprintf(name, name_len, "ldpc_decode_kernel wg=%d waves=%d frames_per_wg=%d mb=%d nb=%d Z=%d edges=%u max_iters=%d grid=%zu lds=%zu",
                  64 * h->frames_per_wg, h->frames_per_wg, h->frames_per_wg, h->code.mb, h->code.nb, h->code.Z, h->code.edges, h->max_iters,
                  grid_of(n_frames, h->frames_per_wg), dec_lds(h));
    return COMMS_OK;
}

comms_status_t comms_ldpcdec_set_timer(comms_ldpcdec_t* h, comms_timer_t* t) { return set_handle_timer(h, t); }

comms_status_t comms_ldpcdec_destroy(comms_ldpcdec_t* h) { return destroy_handle(h); }

}  // extern "C"
