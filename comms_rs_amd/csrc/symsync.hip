// symsync.hip -- symbol synchroniser: fractional-delay matched filter, symbol-rate sampler, rotation and hard decision
// over a Complex<f32> stream in one launch.
//
//   UpsampleNode(L) -> BatchFirNode(Complex(h, 0)) -> [skip mu samples] -> DecimateNode(L S) -> MixerNode(dphase, phase)
//   -> decision     (src/util/resample_node.rs:53-65,120-131; src/filter/fir.rs:87-102; src/mixer.rs:73-84)
// is how the reference would take its symbol-rate sample between two input samples: the matched filter at L times the
// rate, all but one result in L S dropped, and a skip that is no node at all.  Only the kept outputs are computed here,
// each from the one polyphase row of h its timing phase selects:
//   y[k]   = sum_{j >= 0, p + L j < N} h[p + L j] x[k S + q - j],     p = mu mod L,  q = mu div L,  0 <= mu < S L
//   out[k] = Mixer::mix(y[k]) at phase + k dphase (skipped while both are zero), or its decision (COMMS_SYM_BITS)
// with x[-1], x[-2], ... the last input samples of earlier calls: the node's state is Q = (N - 1) div L RAW input samples,
// whatever mu was or becomes.
//
// symsync_kernel (L <= 256, S <= 256, ceil(N / L) <= 1024), 8 bytes of HBM read per input sample and 8 / S written:
//   * the taps are stored phase-major as in resample.hip, tab[p][j] = h[p + L j], rows padded with zeros to blocks of four.
//     Within a call every output is on the SAME row, so its taps are uniform across the wave: a block of four comes by one
//     scalar load and the taps are SGPR operands of the multiply-adds (sgpr_mac.hpp), as in rfir_decim_kernel -- not the
//     per-lane LDS reads of resample_kernel, whose neighbouring lanes are on different phases.
//   * workgroups are persistent and walk tiles of TO consecutive outputs, tile t, t + gridDim.x, ...  A tile stages its
//     S (TO + HB) input samples (HB = ceil((4 NB - 1) / S) outputs' worth in front, NB blocks of four taps) with whole-row
//     buffer loads -- the stream's end reads as zero -- into S PHASE ARRAYS, sample s at [s mod S][s div S], as
//     rfir_decim_kernel does.  The halo is a multiple of S, so tap j = S m - r meets phase array r at element
//     (output + HB - m) for EVERY output: the array and the element offset of a tap are scalars, and the lanes of a read
//     are on consecutive elements (no bank conflicts).  The tiles at the front read the handle's history buffer.
//   * lane t holds outputs jb + t, jb + t + WG, ... (U of them in flight): consecutive lanes hold consecutive outputs, so
//     the Complex<f32> stores are whole lines as they are.  In the bits format the 32 / k lanes of a word gather their
//     decisions with the chain's cross-lane OR (bits_gather) and one of them writes the word, once, with a plain store.
//   * the summation order of an output -- j ascending from an accumulator of +0, one FMA per tap, the zero taps that pad the
//     row included -- depends on nothing but the taps, L and p; the rotor of an output is evaluated in closed form from its
//     own phase (turns0 + k frac, the mixer's fixed point): an output has the same bits wherever a call or a tile boundary
//     falls.
//   * workgroup 0 writes the new history to the other half of a ping-pong pair (History, common.hpp).
// One LDS read (ds_read_b64) per tap and output, i.e. per two FMAs: no window is shared between a lane's outputs yet.
//
// Taps are real and applied as Complex(h, 0): the complex product's cross terms h * im - 0 * re are not formed, so signed
// zeros and non-finite samples may differ from the literal product.  The zero taps that pad a row multiply real samples: a
// NaN or Inf sample may reach outputs up to 4 L - 1 upsampled samples beyond its N taps.
#include <vector>

#include "common.hpp"
#include "fir_handle.hpp"
#include "sgpr_mac.hpp"
#include "stream_call.hpp"

namespace comms {

struct SsArgs {
    const float2* in;       // n samples
    const float2* hist;     // last Q samples before this call, time order
    float2* new_hist;
    void* out;              // n_out Complex<f32>, or ceil(n_out k / 8) bytes of packed decisions
    const float* row;       // the call's row of the tap table: 4 NB floats, row[j] = h[p + L j] (zero beyond the filter)
    size_t n, n_out, n_bytes, tiles;
    int Q, S, NB, HB;
    int q;                  // mu div L: whole input samples of the timing offset
    int TO;                 // outputs per tile
    int stride;             // float2 between phase arrays (>= TO + HB)
    int dp, de;             // blockDim.x mod S, blockDim.x div S: a lane's step from one staged row to its next
    int rotate;             // 0: out = y
    uint64_t turns0, frac;  // mixer phase of output 0 and per-output increment (turns)
    SymTable sym;           // FMT 1, 2
};

// U: outputs a lane has in flight (TO is a multiple of U blockDim.x); FMT: 0 Complex<f32>, k = 1, 2 decided bits per symbol
template <int U, int FMT>
__global__ __launch_bounds__(256) void symsync_kernel(const SsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float2 ss_smem[];
    const int tid = threadIdx.x, WG = blockDim.x;
    const int S = a.S, NB = a.NB, HB = a.HB, TO = a.TO;
    float2* xs = ss_smem;  // [S][stride]
    const int count = S * (TO + HB);
    const int p0 = tid % S, e0 = tid / S;
    typedef const __attribute__((address_space(4))) v2f* const_v2f_ptr;  // constant address space: scalar loads
    const const_v2f_ptr row = (const_v2f_ptr)a.row;

    for (size_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const size_t jb = tile * static_cast<size_t>(TO);  // first output of the tile
        // stream index of the tile's first staged sample: output k, tap j meets staged sample S (k + HB) - j
        const long long g0 = (static_cast<long long>(jb) - HB) * S + a.q;
        __syncthreads();  // the previous tile's samples have been read
        // ---- stage: sample s of the tile -> xs[s mod S][s div S]
        int p = p0, e = e0;
        auto step = [&]() {
            p += a.dp;
            e += a.de;
            if (p >= S) {
                p -= S;
                ++e;
            }
        };
        if (g0 >= 0) {
            // rows of WG samples, four requested before the first is written; past the stream's end a buffer load returns zero
            const size_t left = a.n - static_cast<size_t>(g0);  // g0 <= (n_out - 1 - HB) S + q < n
            const size_t have = left < static_cast<size_t>(count) ? left : static_cast<size_t>(count);
            const __amdgpu_buffer_rsrc_t rs = make_rsrc(a.in + g0, have * 8);
            for (int base = 0; base < count; base += 4 * WG) {
                float2 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = BufRows<const float2*>::get_from(rs, tid * 8, (base + u * WG) * 8);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (base + u * WG + tid < count) xs[p * a.stride + e] = v[u];
                    step();
                }
            }
        } else {  // the tiles that reach back into the history (or in front of it: zeros)
            for (int s = tid; s < count; s += WG) {
                xs[p * a.stride + e] = stream_at(a.in, a.hist, a.Q, g0 + s, a.n);
                step();
            }
        }
        __syncthreads();

        // ---- filter: j ascending; tap j = S m - r of output t meets xs[r][t + HB - m]
        for (int t0 = 0; t0 < TO; t0 += U * WG) {
            cf acc[U];
            const float2* xp[U];
            bool live[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int t = t0 + u * WG + tid;
                acc[u] = cf{0.f, 0.f};
                live[u] = t < TO;  // (a tile smaller than the workgroup)
                xp[u] = xs + (live[u] ? t : 0);
            }
            int r = 0, off = HB;  // of tap 0: phase array 0, element t + HB
            for (int b = 0; b < NB; ++b) {
                const v2f w01 = row[2 * b], w23 = row[2 * b + 1];
                // the block's reads first (a tap's array and element are scalars), then its multiply-adds
                cf x[4][U];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const float2 v = xp[u][off];
                        x[i][u] = cf{v.x, v.y};
                    }
                    // the next tap: one sample earlier -- the phase array below, or the last one, an element earlier
                    off -= a.stride;
                    if (--r < 0) {
                        r += S;
                        off += S * a.stride - 1;
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        if (i & 1) mac_s_hi(acc[u], x[i][u], i < 2 ? w01 : w23);
                        else mac_s_lo(acc[u], x[i][u], i < 2 ? w01 : w23);
                    }
                }
            }

            // ---- store: rotate (the mixer's arithmetic), then the sample itself or its decision
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const size_t j = jb + static_cast<size_t>(t0 + u * WG + tid);
                const bool ok = live[u] && j < a.n_out;
                float2 y = make_float2(acc[u].x, acc[u].y);
                if (a.rotate) {
                    double c, s;
                    mix_rotor_at(a.turns0 + static_cast<uint64_t>(j) * a.frac, c, s);
                    y = mix_one(y, c, s);
                }
                if (FMT == 0) {
                    if (ok) static_cast<float2*>(a.out)[j] = y;
                } else {
                    // the 32 / k lanes of a word hold consecutive outputs, the first a multiple of 32 / k (TO and WG are
                    // multiples of 32): outputs past the end decide to 0, the tail bits of the last byte
                    constexpr int K = FMT == 0 ? 1 : FMT, G = 32 / K;
                    const int l = tid & 63;
                    unsigned bits = ok ? sym_decide<K>(y, a.sym.c) : 0u;
                    bits = bits_gather<G>(bits << (K * (l % G)));
                    if (l % G == 0 && ok) bits_store_word(static_cast<uint8_t*>(a.out), j * K / 8, a.n_bytes, bits);
                }
            }
        }
    }

    hist_advance(a.hist, a.in, a.n, a.new_hist, a.Q);
}

}  // namespace comms

using namespace comms;

struct comms_symsync : Handle {
    size_t n_taps = 0;
    size_t L = 1, S = 1;            // >= 1 (0 is taken as 1)
    size_t Q = 0;                   // state: (n_taps - 1) / L input samples
    uint32_t mu = 0;                // timing offset in steps of 1 / L input samples, 0 <= mu < S L
    double dphase = 0.0;            // as given (wrapped like Mixer::new)
    uint64_t turns = 0, frac = 0;   // the mixer's phase arithmetic: phase of the next output and increment, in turns
    int out_bits = 0;               // 0: Complex<f32>; 1, 2: decided bits per symbol
    SymTable out_sym{};
    int RS = 4, NB = 1, HB = 0, TO = 0, WG = 256, U = 1, stride = 0;
    size_t lds = 0;
    unsigned max_grid = 1;
    DevBuf<float> d_tab;            // [L][RS]
    History hist;                   // last Q samples
};
static_assert(!std::is_copy_constructible_v<comms_symsync>, "a handle is never copied");

namespace {

constexpr size_t SS_MAX_PHASES = 256, SS_MAX_SPS = 256, SS_MAX_ROW = 1024;
constexpr size_t SS_LDS_FOUR = 40 * 1024;  // four workgroups per CU, resample.hip's tier (not measured for this kernel)
constexpr size_t SS_LDS_MAX = 64 * 1024;   // what the project's kernels request per workgroup ...
constexpr size_t SS_LDS_WIDE = 96 * 1024;  // ... but a word of bits needs 32 outputs in a tile, and 32 S samples of S = 256 do not fit there
constexpr int SS_MIN_TILE = 32;

// Tile size: the largest of 1024 ... 32 outputs whose phase arrays fit -- within 40 KiB if a tile of at least 256 does,
// otherwise within 64 KiB, and 96 KiB for the widest symbols.  Within the limits of comms_symsync_create a tile of 32 always
// fits: S (32 + HB) <= 32 S + 1023 + S <= 9471 samples = 74 KiB
bool plan_tile(comms_symsync* h) {
    const int S = static_cast<int>(h->S);
    for (size_t limit : {SS_LDS_FOUR, SS_LDS_MAX, SS_LDS_WIDE})
        for (int TO = 1024; TO >= (limit == SS_LDS_FOUR ? 256 : SS_MIN_TILE); TO /= 2) {
            if ((static_cast<size_t>(TO) + h->HB) * S * 8 > limit) continue;
            int stride = plan_stride(S, TO + h->HB, 16);
            if (static_cast<size_t>(S) * stride * 8 > limit) stride = TO + h->HB;  // the padding does not fit: unpadded does
            const size_t lds = static_cast<size_t>(S) * stride * 8;
            h->TO = TO;
            h->stride = stride;
            h->lds = lds;
            return true;
        }
    return false;
}

template <int U, int FMT>
comms_status_t launch_symsync(const SsArgs& a, unsigned blocks, int wg, size_t lds, hipStream_t s) {
    return launch_kernel<symsync_kernel<U, FMT>>("symsync_kernel", dim3(blocks), dim3(wg), lds, s, {}, a);
}

template <int U>
comms_status_t launch_symsync_fmt(int fmt, const SsArgs& a, unsigned blocks, int wg, size_t lds, hipStream_t s) {
    switch (fmt) {
        case 1: return launch_symsync<U, 1>(a, blocks, wg, lds, s);
        case 2: return launch_symsync<U, 2>(a, blocks, wg, lds, s);
        default: return launch_symsync<U, 0>(a, blocks, wg, lds, s);
    }
}

// tiles of a call that writes n_out symbols, and the grid that walks them
size_t symsync_tiles(const comms_symsync* h, size_t n_out) { return (n_out + h->TO - 1) / h->TO; }
size_t symsync_grid(const comms_symsync* h, size_t n_out) { return tile_grid(symsync_tiles(h, n_out), h->max_grid); }

size_t symsync_out_bytes(const comms_symsync* h, size_t n_out) {
    return h->out_bits ? (n_out * h->out_bits + 7) / 8 : n_out * sizeof(comms_c32);
}

}  // namespace

extern "C" {

comms_status_t comms_symsync_out_len(size_t n, size_t sps, size_t* out_len) {
    COMMS_ARG(out_len != nullptr, "out_len is NULL");
    *out_len = n / (sps < 1 ? 1 : sps);
    return COMMS_OK;
}

comms_status_t comms_symsync_state_len(size_t n_taps, size_t phases, size_t* out_len) {
    COMMS_ARG(out_len != nullptr, "out_len is NULL");
    COMMS_ARG(n_taps > 0, "taps must hold at least one tap");
    *out_len = (n_taps - 1) / (phases < 1 ? 1 : phases);
    return COMMS_OK;
}

comms_status_t comms_symsync_create(const float* taps, size_t n_taps, size_t phases, size_t sps, int32_t device,
                                    comms_symsync_t** out) {
    COMMS_ARG(out != nullptr, "out is NULL");
    *out = nullptr;
    COMMS_ARG(taps != nullptr && n_taps > 0, "taps must hold at least one tap");
    const size_t L = phases < 1 ? 1 : phases, S = sps < 1 ? 1 : sps;
    COMMS_ARG(L <= SS_MAX_PHASES, "at most %zu phases (got %zu)", SS_MAX_PHASES, L);
    COMMS_ARG(S <= SS_MAX_SPS, "at most %zu samples per symbol (got %zu)", SS_MAX_SPS, S);
    COMMS_ARG(n_taps <= SS_MAX_ROW * L, "at most %zu taps per phase (%zu taps over %zu phases)", SS_MAX_ROW, n_taps, L);
    HandlePtr<comms_symsync> h;
    COMMS_TRY(make_handle(device, &h));
    h->n_taps = n_taps;
    h->L = L;
    h->S = S;
    h->Q = (n_taps - 1) / L;
    h->NB = static_cast<int>((h->Q + 1 + 3) / 4);
    h->RS = 4 * h->NB;
    h->HB = static_cast<int>((4 * h->NB - 1 + S - 1) / S);
    if (!plan_tile(h.get()))
        return fail(COMMS_ERR_DEVICE, "symsync: no tile fits (%zu phases, %zu samples per symbol, %zu taps)", L, S, n_taps);
    h->WG = tile_workgroup(h->TO);
    h->U = h->TO >= 4 * h->WG ? 4 : h->TO >= 2 * h->WG ? 2 : 1;
    h->max_grid = resident_workgroups(h->lds);
    COMMS_HIP_TRY(h->d_tab.upload(polyphase_rows(taps, n_taps, L, static_cast<size_t>(h->RS))));
    COMMS_HIP_TRY(h->hist.alloc(h->Q, sizeof(comms_c32)));
    *out = h.release();
    return COMMS_OK;
}

comms_status_t comms_symsync_set_timing(comms_symsync_t* h, double tau) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG(std::isfinite(tau), "tau must be finite");
    const double steps = tau * static_cast<double>(h->L);
    COMMS_ARG(std::fabs(steps) < 0x1.0p62, "tau is out of range");
    const long long period = static_cast<long long>(h->S * h->L);
    long long m = std::llround(steps) % period;
    if (m < 0) m += period;
    h->mu = static_cast<uint32_t>(m);
    return COMMS_OK;
}

comms_status_t comms_symsync_get_timing(const comms_symsync_t* h, uint32_t* out_mu) {
    COMMS_ARG(h && out_mu, "NULL argument");
    *out_mu = h->mu;
    return COMMS_OK;
}

comms_status_t comms_symsync_set_rotation(comms_symsync_t* h, double dphase, double phase) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG(std::isfinite(dphase) && std::isfinite(phase), "dphase and phase must be finite");
    h->dphase = mix_wrap_dphase(dphase);
    h->frac = mix_to_turns(h->dphase);
    h->turns = mix_to_turns(phase);
    return COMMS_OK;
}

// Rotor phase of the next output (radians, as comms_mixer_get_phase).
comms_status_t comms_symsync_get_phase(const comms_symsync_t* h, double* out_phase) {
    COMMS_ARG(h && out_phase, "NULL argument");
    *out_phase = static_cast<double>(h->turns >> 11) * (kMixT * 0x1.0p-53);
    return COMMS_OK;
}

// Stateless: history, phase and timing are the same whichever format a call writes.
comms_status_t comms_symsync_set_output_format(comms_symsync_t* h, int32_t format, int32_t bits_per_sym, const comms_c32* constellation) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG(format == COMMS_SYM_C32 || format == COMMS_SYM_BITS, "the synchroniser writes COMMS_SYM_C32 or COMMS_SYM_BITS (got format %d)", format);
    if (format == COMMS_SYM_C32) {
        h->out_bits = 0;
        return COMMS_OK;
    }
    SymTable t;
    COMMS_TRY(sym_table(bits_per_sym, constellation, &t));
    h->out_sym = t;
    h->out_bits = bits_per_sym;
    return COMMS_OK;
}

comms_status_t comms_symsync_run_dev(comms_symsync_t* h, const comms_c32* d_in, size_t n, void* d_out, void* stream) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG((d_in && d_out) || !n, "NULL device pointer");
    COMMS_ARG(n % h->S == 0, "n (%zu) must be a multiple of the %zu samples per symbol", n, h->S);
    COMMS_ARG(n <= SIZE_MAX / 8, "n overflows");
    const size_t n_out = n / h->S, out_bytes = symsync_out_bytes(h, n_out);
    COMMS_ARG(!n || !ranges_overlap(d_in, n * 8, d_out, out_bytes), "the synchroniser cannot run in place");
    COMMS_ARG((reinterpret_cast<uintptr_t>(d_in) & 7) == 0, "input must be aligned to one sample");
    COMMS_ARG((reinterpret_cast<uintptr_t>(d_out) & (h->out_bits ? 3 : 7)) == 0,
              h->out_bits ? "bits output (COMMS_SYM_BITS) must be 4-byte aligned" : "output must be aligned to one sample");
    COMMS_TRY(use_device(h->device));
    if (!n) return COMMS_OK;
    hipStream_t s = nullptr;
    COMMS_TRY(h->enter(stream, &s));
    const unsigned grid = static_cast<unsigned>(symsync_grid(h, n_out));
    SsArgs a{};
    a.in = reinterpret_cast<const float2*>(d_in);
    a.hist = h->hist.cur<float2>();
    a.new_hist = h->hist.next<float2>();
    a.out = d_out;
    a.row = h->d_tab.get() + static_cast<size_t>(h->mu % h->L) * h->RS;
    a.n = n;
    a.n_out = n_out;
    a.n_bytes = out_bytes;
    a.tiles = symsync_tiles(h, n_out);
    a.Q = static_cast<int>(h->Q);
    a.S = static_cast<int>(h->S);
    a.NB = h->NB;
    a.HB = h->HB;
    a.q = static_cast<int>(h->mu / h->L);
    a.TO = h->TO;
    a.stride = h->stride;
    a.dp = h->WG % a.S;
    a.de = h->WG / a.S;
    a.rotate = (h->turns | h->frac) != 0;
    a.turns0 = h->turns;
    a.frac = h->frac;
    a.sym = h->out_sym;
    h->tic(s);
    comms_status_t st;
    switch (h->U) {
        case 4: st = launch_symsync_fmt<4>(h->out_bits, a, grid, h->WG, h->lds, s); break;
        case 2: st = launch_symsync_fmt<2>(h->out_bits, a, grid, h->WG, h->lds, s); break;
        default: st = launch_symsync_fmt<1>(h->out_bits, a, grid, h->WG, h->lds, s); break;
    }
    h->toc(s);
    COMMS_TRY(st);
    h->hist.flip();
    h->turns += static_cast<uint64_t>(n_out) * h->frac;
    return COMMS_OK;
}

comms_status_t comms_symsync_run(comms_symsync_t* h, const comms_c32* in, size_t n, void* out) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG((in && out) || !n, "NULL host pointer");
    COMMS_ARG(n % h->S == 0, "n (%zu) must be a multiple of the %zu samples per symbol", n, h->S);
    COMMS_ARG(n <= SIZE_MAX / 8, "n overflows");
    COMMS_TRY(use_device(h->device));
    if (!n) return COMMS_OK;
    // a unit = S input samples, one output; bits output: 32 / k of them, one whole 32-bit word of bits, so that every chunk
    // but the last starts on a word of the output
    const size_t out_elem = h->out_bits ? 4 : sizeof(comms_c32);
    const size_t unit = h->out_bits ? h->S * static_cast<size_t>(32 / h->out_bits) : h->S;
    return h->run_host_units(in, n * 8, unit * 8, out, symsync_out_bytes(h, n / h->S), out_elem, [&](void* d_in, void* d_out, size_t ib, size_t) {
        return comms_symsync_run_dev(h, static_cast<const comms_c32*>(d_in), ib / 8, d_out, COMMS_STREAM_HANDLE);
    });
}

comms_status_t comms_symsync_get_state(comms_symsync_t* h, comms_c32* state, size_t n_state) {
    return get_history_state(h, state, n_state, "samples");
}

comms_status_t comms_symsync_set_state(comms_symsync_t* h, const comms_c32* state, size_t n_state) {
    return set_history_state(h, state, n_state, "samples");
}

comms_status_t comms_symsync_get_kernel(const comms_symsync_t* h, size_t n, char* name, size_t name_len) {
    COMMS_ARG(h && name && name_len, "NULL argument");
    std::snprintf(name, name_len, "symsync_kernel<%d, %s> tile=%d wg=%d lds=%zu tiles=%zu grid=%zu max_grid=%u", h->U,
                  h->out_bits == 0 ? "c32" : h->out_bits == 1 ? "bits1" : "bits2", h->TO, h->WG, h->lds, symsync_tiles(h, n / h->S),
                  symsync_grid(h, n / h->S), h->max_grid);
    return COMMS_OK;
}

comms_status_t comms_symsync_set_timer(comms_symsync_t* h, comms_timer_t* t) { return set_handle_timer(h, t); }

comms_status_t comms_symsync_destroy(comms_symsync_t* h) { return destroy_handle(h); }

}  // extern "C"
