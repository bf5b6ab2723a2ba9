// channelizer.hip -- polyphase channelizer: M tuner chains (mixer, FIR, decimator) over one Complex<f32> stream in one launch.
//
//   for k in 0 .. M-1:  MixerNode::new(0, -2 pi k / M) -> BatchFirNode(Complex(taps, 0)) -> DecimateNode(D)
//   (src/mixer.rs:43-84; src/filter/fir.rs:87-102; src/util/resample_node.rs:53-65)
// The M chains in series read the stream M times and spend N multiply-adds per kept output of every channel.  With
// w = e^{-2 pi i / M}, t the stream index of a kept sample, r = t mod M and n = p + M q the chains collapse to
//   v_p(t)   = sum_{q >= 0, p + M q < N} h[p + M q] x[t - p - M q]            p = 0 .. M-1   (N real x complex MACs per frame)
//   out_k[j] = sum_{p < M} e^{+2 pi i k p / M} v_{(p + r) mod M}(t)            t = c + j D, c = stream index of the call's sample 0
// an unnormalised inverse M-point DFT of the branch outputs, circularly shifted by r.  The oscillator phase is the integer
// (k t) mod M: exact, never accumulated.
//
// channelizer_kernel (M a power of two 2 ... 1024, N <= 16 M, D <= 4 M), 8 bytes in and 8 M / D bytes out per input sample:
//   * a tile is F consecutive frames (one output of every channel each), F M <= 2048.  Workgroups are persistent and take
//     CONSECUTIVE tiles (workgroup b: tiles b T ... b T + T - 1): the channel-major rows of neighbouring tiles and the
//     N - D samples two neighbouring tiles share then meet in the same cache.
//   * STAGED: the (F - 1) D + Q M samples a tile reaches (Q = ceil(N / M)) are copied to LDS once; the tiles at the front
//     read the handle's history buffer.  A span that does not fit beside the frame buffer even for one frame (M = 1024 from nine
//     taps per branch, M = 512 from fifteen) is read from global memory through the caches instead, with the same arithmetic.
//   * the taps are used in their natural order, zero-padded to Q M: lane p of a frame reads h[p + M q], consecutive lanes
//     consecutive floats (LDS up to 16 KiB, the vector cache above), and x[t - p - M q], consecutive lanes consecutive
//     samples downwards: no bank conflicts either side.  q ascends from an accumulator of +0, one FMA per component.
//   * v_p is placed at index (p - r) mod M of its frame: the shift by r is an index rotation, not a multiplication.
//   * the inverse DFT of all frames of the tile: Stockham radix-4 layers (fft_radix.hpp's packed butterflies, DIR = +1)
//     between two LDS buffers, a radix-2 layer last where log2 M is odd, twiddles from a table of the M-th roots.
//     Frames are M + 1 samples apart in LDS, so the channel-major store, which walks a channel across the frames, is
//     conflict-free; every channel row receives the tile's F outputs as one contiguous piece.
//   * an output's bits depend on the taps, M, D, t mod M and the samples only -- not on its place in a tile, a call or the
//     grid, nor on the layout or on where the samples were read from.
//   * workgroup 0 writes the new history (last N - 1 samples) to the other half of a ping-pong pair.
// Everything else -- M not a power of two, M = 1, longer filters, larger rates -- runs M launches of the chain node
// (comms_chain_*, mixer in front, dphase = -2 pi k / M, phase set from t) on scratch of the handle: a first pass writes
// history + call, padded with zeros to whole groups of D either side, so that the chains need no state of their own and a
// ragged call costs nothing extra; a last pass moves the kept outputs into the layout.
//
// Taps are real and applied as Complex(h, 0) without the cross terms; the zero taps that pad a branch and the transform
// spread a NaN or Inf sample over all M channels of the frames it reaches.
#include <algorithm>
#include <string>
#include <vector>

#include "common.hpp"
#include "fft_radix.hpp"
#include "stream_call.hpp"

namespace comms {

struct ChzArgs {
    const float2* in;      // n samples
    const float2* hist;    // last H samples before this call, time order
    float2* new_hist;
    float2* out;           // frames * M outputs
    const float* taps;     // Q * M floats: h[0 .. N), then zeros
    const float2* tw;      // tw[m] = e^{+2 pi i m / M}
    size_t n, frames, tiles, tiles_per_wg;
    int H;                 // N - 1
    int M, lgM, D, Q, F;
    int S;                 // samples staged per tile: (F - 1) D + Q M
    unsigned r0;           // t mod M of the call's sample 0
    int frame_major;
};

__device__ __forceinline__ float2 chz_mac(float2 acc, float w, float2 x) {
    acc.x = __builtin_fmaf(w, x.x, acc.x);
    acc.y = __builtin_fmaf(w, x.y, acc.y);
    return acc;
}

// One Stockham layer of radix R over the nf frames of a tile: src -> dst, Ns = product of the radices so far
template <int R>
__device__ __forceinline__ void chz_layer(const float2* src, float2* dst, const float2* tw, int nf, int M, int lgM, int MS, int Ns) {
    constexpr int lgR = R == 4 ? 2 : 1;
    const int per = M >> lgR, items = nf << (lgM - lgR);
    const int tstep = M / (Ns * R);
    for (int it = threadIdx.x; it < items; it += blockDim.x) {
        const int f = it >> (lgM - lgR), j = it & (per - 1);
        const int k = j & (Ns - 1);
        const float2* s = src + f * MS + j;
        float2* d = dst + f * MS + ((j - k) << lgR) + k;
        if constexpr (R == 4) {
            cf a = to_cf(s[0]), b = to_cf(s[per]), c = to_cf(s[2 * per]), e = to_cf(s[3 * per]);
            if (Ns > 1) {
                const int i1 = k * tstep;
                b = cmulf(b, to_cf(tw[i1]));
                c = cmulf(c, to_cf(tw[2 * i1]));
                e = cmulf(e, to_cf(tw[3 * i1]));
            }
            radix4<1>(a, b, c, e);
            d[0] = to_f2(a);
            d[Ns] = to_f2(b);
            d[2 * Ns] = to_f2(c);
            d[3 * Ns] = to_f2(e);
        } else {
            cf a = to_cf(s[0]), b = to_cf(s[per]);
            if (Ns > 1) b = cmulf(b, to_cf(tw[k * tstep]));
            d[0] = to_f2(cadd(a, b));
            d[Ns] = to_f2(csub(a, b));
        }
    }
}

template <bool STAGED, bool TAB_LDS>
__global__ __launch_bounds__(256) void channelizer_kernel(const ChzArgs a) {
    extern __shared__ __attribute__((aligned(16))) float chz_smem[];
    const int tid = threadIdx.x, WG = blockDim.x;
    const int M = a.M, lgM = a.lgM, D = a.D, Q = a.Q, F = a.F, MS = M + 1;
    const int QM = Q * M;
    const int tab_floats = TAB_LDS ? QM : 0;  // even: M >= 2
    float2* fa = reinterpret_cast<float2*>(chz_smem + tab_floats);  // F frames of MS samples
    float2* fb = fa + F * MS;                                       // the second frame buffer; the staged samples until the transform
    float2* xs = fb;
    const float* tab = a.taps;
    if (TAB_LDS) {
        for (int i = tid; i < tab_floats; i += WG) chz_smem[i] = a.taps[i];
        tab = chz_smem;
    }
    const float2 zero = make_float2(0.f, 0.f);
    const size_t t_begin = static_cast<size_t>(blockIdx.x) * a.tiles_per_wg;
    const size_t t_end = t_begin + a.tiles_per_wg < a.tiles ? t_begin + a.tiles_per_wg : a.tiles;

    for (size_t tile = t_begin; tile < t_end; ++tile) {
        const size_t j0 = tile * static_cast<size_t>(F);
        const int nf = a.frames - j0 < static_cast<size_t>(F) ? static_cast<int>(a.frames - j0) : F;
        // sample t - p - M q of frame f sits (QM - 1) + f D - p - M q beyond the tile's first sample, call index glo
        const long long glo = static_cast<long long>(j0) * D - (QM - 1);
        __syncthreads();  // the table is in place; the previous tile's frames have been stored
        if (STAGED) {
            for (int s = tid; s < a.S; s += WG) {
                const long long g = glo + s;
                float2 v = zero;
                if (g >= 0) {
                    if (static_cast<size_t>(g) < a.n) v = a.in[g];
                } else if (g >= -static_cast<long long>(a.H)) {
                    v = a.hist[a.H + g];
                }
                xs[s] = v;
            }
            __syncthreads();
        }

        // ---- branch filters: item (f, p), consecutive lanes consecutive p
        const int items = nf << lgM;
        for (int it = tid; it < items; it += WG) {
            const int p = it & (M - 1), f = it >> lgM;
            float2 acc = zero;
            const float* tp = tab + p;
            if (STAGED) {
                const float2* xp = xs + (QM - 1) + f * D - p;
#pragma unroll 4
                for (int q = 0; q < Q; ++q) acc = chz_mac(acc, tp[q * M], xp[-q * M]);
            } else {
                const long long g = static_cast<long long>(j0 + f) * D - p;  // < n: the frame's newest sample is one of the call's
                if (glo >= 0) {
                    const float2* xp = a.in + g;
#pragma unroll 4
                    for (int q = 0; q < Q; ++q) acc = chz_mac(acc, tp[q * M], xp[-static_cast<long long>(q) * M]);
                } else {
                    for (int q = 0; q < Q; ++q) {
                        const long long gq = g - static_cast<long long>(q) * M;
                        float2 x = zero;
                        if (gq >= 0) x = a.in[gq];
                        else if (gq >= -static_cast<long long>(a.H)) x = a.hist[a.H + gq];
                        acc = chz_mac(acc, tp[q * M], x);
                    }
                }
            }
            const unsigned r = (a.r0 + static_cast<unsigned>((j0 + f) * static_cast<size_t>(D))) & (M - 1);
            fa[f * MS + ((p - r) & (M - 1))] = acc;
        }
        __syncthreads();

        // ---- inverse DFT of every frame, natural order in and out
        const float2* res = fa;
        {
            float2* src = fa;
            float2* dst = fb;
            int Ns = 1;
            for (; Ns * 4 <= M; Ns *= 4) {
                chz_layer<4>(src, dst, a.tw, nf, M, lgM, MS, Ns);
                __syncthreads();
                float2* t = src;
                src = dst;
                dst = t;
            }
            if (Ns < M) {
                chz_layer<2>(src, dst, a.tw, nf, M, lgM, MS, Ns);
                __syncthreads();
                src = dst;
            }
            res = src;
        }

        // ---- store
        if (a.frame_major) {
            float2* o = a.out + j0 * M;
            for (int it = tid; it < items; it += WG) o[it] = res[(it >> lgM) * MS + (it & (M - 1))];
        } else {
            // F is a power of two: item (k, f), consecutive lanes consecutive frames of one channel
            const int lgF = 31 - __builtin_clz(F);
            for (int it = tid; it < (M << lgF); it += WG) {
                const int f = it & (F - 1), k = it >> lgF;
                if (f < nf) a.out[static_cast<size_t>(k) * a.frames + j0 + f] = res[f * MS + k];
            }
        }
    }

    // ---- new_hist = last H samples of concat(old_hist, in)
    if (blockIdx.x == 0) {
        for (int j = tid; j < a.H; j += WG) {
            const size_t q = a.n + static_cast<size_t>(j);
            a.new_hist[j] = q < static_cast<size_t>(a.H) ? a.hist[q] : a.in[q - a.H];
        }
    }
}

// The series, first pass: ext = zeros(P - H) | history | call | zeros to a whole group of D; and the new history
__global__ __launch_bounds__(256) void chz_prep_kernel(const float2* in, const float2* hist, float2* new_hist, float2* ext, size_t n, size_t total,
                                                       size_t P, int H) {
    const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    const size_t t0 = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    for (size_t i = t0; i < total; i += stride) {
        float2 v = make_float2(0.f, 0.f);
        if (i >= P) {
            if (i - P < n) v = in[i - P];
        } else if (P - i <= static_cast<size_t>(H)) {
            v = hist[H - (P - i)];
        }
        ext[i] = v;
    }
    for (size_t j = t0; j < static_cast<size_t>(H); j += stride) {
        const size_t q = n + j;
        new_hist[j] = q < static_cast<size_t>(H) ? hist[q] : in[q - H];
    }
}

// The series, last pass: tmp[k][skip + j] -> the layout
__global__ __launch_bounds__(256) void chz_scatter_kernel(const float2* tmp, float2* out, size_t frames, size_t M, size_t row, size_t skip, int frame_major) {
    const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    const size_t total = frames * M;
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < total; i += stride) {
        if (frame_major) {
            const size_t j = i / M, k = i % M;
            out[i] = tmp[k * row + skip + j];
        } else {
            const size_t k = i / frames, j = i % frames;
            out[i] = tmp[k * row + skip + j];
        }
    }
}

}  // namespace comms

using namespace comms;

struct comms_channelizer : Handle {
    size_t n_taps = 0, M = 1, D = 1;
    size_t H = 0;            // state: n_taps - 1 input samples
    uint64_t r = 0;          // t mod M of the next input sample
    int layout = COMMS_CHANNELIZER_CHANNEL_MAJOR;
    bool series = false;     // outside the kernel's range
    // channelizer_kernel
    int lgM = 0, Q = 1, F = 1, S = 0;
    bool staged = true, tab_lds = true;
    size_t lds = 0;
    unsigned max_grid = 1;
    DevBuf<float> d_tab;
    DevBuf<float2> d_tw;
    History hist;            // last H samples
    // the series: one chain per channel (made on first use), the padded stream and the chains' outputs
    std::vector<float> taps;
    std::vector<InnerHandle<comms_chain_t, comms_chain_destroy>> chains;
    Scratch ext, tmp;
};
static_assert(!std::is_copy_constructible_v<comms_channelizer>, "a handle is never copied");

namespace {

constexpr size_t CHZ_MAX_M = 1024;        // one launch: M a power of two 2 ... 1024
constexpr size_t CHZ_TAPS_PER_M = 16;     //             N <= 16 M
constexpr size_t CHZ_RATE_PER_M = 4;      //             D <= 4 M
// The series: one chain handle per channel.  Every chain handle (and the FIR handle inside it) takes a stream of its own from
// the device's pool although the chains only ever run on the channelizer's stream: a series of M channels holds about 2 M
// pooled streams until it is destroyed, when they go back to the pool (comms_stream_pool_trim frees them).  The cap keeps
// that at about two thousand.
constexpr size_t CHZ_MAX_SERIES_M = 1024;
constexpr size_t CHZ_TILE = 2048;         // F M
constexpr size_t CHZ_LDS_MAX = 64 * 1024; // what the project's kernels request per workgroup
constexpr size_t CHZ_TAB_LDS = 16 * 1024;

bool in_kernel_range(size_t M, size_t N, size_t D) {
    return M >= 2 && M <= CHZ_MAX_M && (M & (M - 1)) == 0 && N <= CHZ_TAPS_PER_M * M && D <= CHZ_RATE_PER_M * M;
}

// F = 2048 / M frames per tile, halved while the tile's samples do not fit in LDS beside table and frame buffer; if not even
// one frame's do, the samples stay in global memory and the tile keeps 2048 / M frames
void plan_tile(comms_channelizer* h) {
    const size_t M = h->M, D = h->D, QM = static_cast<size_t>(h->Q) * M, MS = M + 1;
    const size_t tab = QM * 4 <= CHZ_TAB_LDS ? QM * 4 : 0;
    h->tab_lds = tab != 0;
    const size_t F0 = CHZ_TILE / M;
    for (size_t F = F0; F >= 1; F /= 2) {
        const size_t S = (F - 1) * D + QM;
        const size_t lds = tab + (F * MS + std::max(F * MS, S)) * 8;
        if (lds > CHZ_LDS_MAX) continue;
        h->staged = true;
        h->F = static_cast<int>(F);
        h->S = static_cast<int>(S);
        h->lds = lds;
        return;
    }
    h->staged = false;
    h->F = static_cast<int>(F0);
    h->S = 0;
    h->lds = tab + 2 * F0 * MS * 8;
}

template <bool STAGED, bool TAB_LDS>
comms_status_t launch_channelizer(const ChzArgs& a, unsigned blocks, size_t lds, hipStream_t s) {
    return launch_kernel<channelizer_kernel<STAGED, TAB_LDS>>("channelizer_kernel", dim3(blocks), dim3(256), lds, s, {}, a);
}

size_t chz_frames(size_t n, size_t D) { return n / D + (n % D ? 1 : 0); }

bool forced_series() { return diag_knob("COMMS_CHANNELIZER_SERIES", 0) != 0; }

comms_status_t ensure_chains(comms_channelizer* h) {
    if (!h->chains.empty()) return COMMS_OK;
    std::vector<comms_c32> ct(h->n_taps);
    for (size_t i = 0; i < h->n_taps; ++i) ct[i] = comms_c32{h->taps[i], 0.0f};
    std::vector<InnerHandle<comms_chain_t, comms_chain_destroy>> made(h->M);  // all M of them, or none
    for (size_t k = 0; k < h->M; ++k) {
        const double dphase = -kMixT * (static_cast<double>(k) / static_cast<double>(h->M));
        comms_chain_t* c = nullptr;
        COMMS_TRY(comms_chain_create_ex(dphase, 0.0, ct.data(), h->n_taps, h->D, 0, h->device, &c));
        made[k].reset(c);
    }
    h->chains.swap(made);
    if (h->timer) COMMS_TRY(comms_chain_set_timer(h->chains[0].get(), h->timer));
    return COMMS_OK;
}

// M launches of the chain node on history + call; the chains keep no state that matters: every call brings its own history
// in front, in whole groups of D whose outputs are dropped, and sets each oscillator from t
comms_status_t run_series(comms_channelizer* h, const float2* d_in, size_t n, float2* d_out, size_t frames, hipStream_t s) {
    COMMS_TRY(ensure_chains(h));
    const size_t D = h->D, M = h->M, H = h->H;
    const size_t P = (H + D - 1) / D * D, skip = P / D;
    const size_t total = P + frames * D, row = skip + frames;
    COMMS_ARG(row <= SIZE_MAX / 8 / M, "the series' scratch overflows");
    COMMS_TRY(h->ext.reserve(total * 8));
    COMMS_TRY(h->tmp.reserve(row * M * 8));
    float2* ext = static_cast<float2*>(h->ext.p);
    float2* tmp = static_cast<float2*>(h->tmp.p);
    const unsigned blocks = static_cast<unsigned>(std::min<size_t>((total + 255) / 256, static_cast<size_t>(kNumCU) * 8));
    chz_prep_kernel<<<dim3(blocks), dim3(256), 0, s>>>(d_in, h->hist.cur<float2>(), h->hist.next<float2>(), ext, n, total, P, static_cast<int>(H));
    COMMS_TRY(launch_ok("chz_prep_kernel"));
    const uint64_t t0 = (h->r + M - P % M) % M;  // (t - P) mod M: the stream index of ext[0]
    for (size_t k = 0; k < M; ++k) {
        const uint64_t turn = ((M - k) % M) * t0 % M;  // -(k t0) mod M
        COMMS_TRY(comms_chain_set_phase(h->chains[k].get(), kMixT * (static_cast<double>(turn) / static_cast<double>(M))));
        COMMS_TRY(comms_chain_run_dev(h->chains[k].get(), reinterpret_cast<const comms_c32*>(ext), total, tmp + k * row, s));
    }
    const size_t outs = frames * M;
    const unsigned sblocks = static_cast<unsigned>(std::min<size_t>((outs + 255) / 256, static_cast<size_t>(kNumCU) * 8));
    chz_scatter_kernel<<<dim3(sblocks), dim3(256), 0, s>>>(tmp, d_out, frames, M, row, skip, h->layout == COMMS_CHANNELIZER_FRAME_MAJOR);
    return launch_ok("chz_scatter_kernel");
}

unsigned chz_grid(const comms_channelizer* h, size_t frames, size_t* tiles_out, size_t* per_out) {
    const size_t tiles = (frames + h->F - 1) / h->F;
    const size_t per = (tiles + h->max_grid - 1) / h->max_grid;
    const size_t per1 = per < 1 ? 1 : per;
    *tiles_out = tiles;
    *per_out = per1;
    return static_cast<unsigned>((tiles + per1 - 1) / per1);
}

}  // namespace

extern "C" {

comms_status_t comms_channelizer_out_len(size_t n, size_t down, size_t* frames) {
    COMMS_ARG(frames != nullptr, "frames is NULL");
    *frames = chz_frames(n, down < 1 ? 1 : down);
    return COMMS_OK;
}

comms_status_t comms_channelizer_state_len(size_t n_taps, size_t* out_len) {
    COMMS_ARG(out_len != nullptr, "out_len is NULL");
    COMMS_ARG(n_taps > 0, "taps must hold at least one tap");
    *out_len = n_taps - 1;
    return COMMS_OK;
}

comms_status_t comms_channelizer_create(const float* taps, size_t n_taps, size_t channels, size_t down, int32_t layout, int32_t device,
                                        comms_channelizer_t** out) {
    COMMS_ARG(out != nullptr, "out is NULL");
    *out = nullptr;
    COMMS_ARG(taps != nullptr && n_taps > 0, "taps must hold at least one tap (the reference panics on an empty state)");
    COMMS_ARG(channels >= 1, "a channelizer has at least one channel");
    COMMS_ARG(layout == COMMS_CHANNELIZER_CHANNEL_MAJOR || layout == COMMS_CHANNELIZER_FRAME_MAJOR,
              "layout must be COMMS_CHANNELIZER_CHANNEL_MAJOR (0) or COMMS_CHANNELIZER_FRAME_MAJOR (1), got %d", layout);
    COMMS_ARG(down <= 0x7fffffffu, "rate %zu is out of range", down);
    COMMS_ARG(n_taps <= (1u << 20), "too many taps (%zu)", n_taps);
    const size_t D = down < 1 ? 1 : down;
    const bool series = !in_kernel_range(channels, n_taps, D);
    COMMS_ARG(!series || channels <= CHZ_MAX_SERIES_M, "%zu channels: outside the kernel's range the node runs one chain per channel, at most %zu",
              channels, CHZ_MAX_SERIES_M);
    HandlePtr<comms_channelizer> h;
    COMMS_TRY(make_handle(device, &h));
    h->n_taps = n_taps;
    h->M = channels;
    h->D = D;
    h->H = n_taps - 1;
    h->layout = layout;
    h->series = series;
    h->taps.assign(taps, taps + n_taps);
    COMMS_HIP_TRY(h->hist.alloc(h->H, sizeof(float2)));
    if (!series) {
        const size_t M = channels;
        while ((static_cast<size_t>(1) << h->lgM) < M) ++h->lgM;
        h->Q = static_cast<int>((n_taps + M - 1) / M);
        plan_tile(h.get());
        h->max_grid = resident_workgroups(h->lds);
        const int cap = diag_knob("COMMS_CHANNELIZER_GRID", 0);  // sweeps: fewer workgroups
        if (cap > 0 && static_cast<unsigned>(cap) < h->max_grid) h->max_grid = static_cast<unsigned>(cap);
        std::vector<float> tab(static_cast<size_t>(h->Q) * M, 0.0f);
        std::copy(taps, taps + n_taps, tab.begin());
        std::vector<float2> tw(M);
        for (size_t m = 0; m < M; ++m) {
            const double ang = 2.0 * 3.14159265358979323846264338327950288 * static_cast<double>(m) / static_cast<double>(M);
            tw[m] = make_float2(static_cast<float>(cos(ang)), static_cast<float>(sin(ang)));
        }
        COMMS_HIP_TRY(h->d_tab.upload(tab));
        COMMS_HIP_TRY(h->d_tw.upload(tw));
    }
    if (series) COMMS_TRY(ensure_chains(h.get()));
    *out = h.release();
    return COMMS_OK;
}

comms_status_t comms_channelizer_run_dev(comms_channelizer_t* h, const comms_c32* d_in, size_t n, comms_c32* d_out, void* stream) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG((d_in && d_out) || !n, "NULL device pointer");
    COMMS_TRY(use_device(h->device));
    if (!n) return COMMS_OK;
    const size_t frames = chz_frames(n, h->D);
    COMMS_ARG(n <= SIZE_MAX / 16 && frames <= SIZE_MAX / 16 / h->M, "frames * channels overflows");
    const size_t outs = frames * h->M;
    COMMS_ARG(!ranges_overlap(d_in, n * 8, d_out, outs * 8), "the channelizer cannot run in place");
    COMMS_ARG(((reinterpret_cast<uintptr_t>(d_in) | reinterpret_cast<uintptr_t>(d_out)) & 7) == 0, "pointers must be aligned to one sample");
    hipStream_t s = nullptr;
    COMMS_TRY(h->enter(stream, &s));
    const float2* in = reinterpret_cast<const float2*>(d_in);
    float2* out = reinterpret_cast<float2*>(d_out);
    if (h->series || forced_series()) {
        COMMS_TRY(run_series(h, in, n, out, frames, s));
    } else {
        ChzArgs a{};
        a.in = in;
        a.hist = h->hist.cur<float2>();
        a.new_hist = h->hist.next<float2>();
        a.out = out;
        a.taps = h->d_tab.get();
        a.tw = h->d_tw.get();
        a.n = n;
        a.frames = frames;
        const unsigned grid = chz_grid(h, frames, &a.tiles, &a.tiles_per_wg);
        a.H = static_cast<int>(h->H);
        a.M = static_cast<int>(h->M);
        a.lgM = h->lgM;
        a.D = static_cast<int>(h->D);
        a.Q = h->Q;
        a.F = h->F;
        a.S = h->S;
        a.r0 = static_cast<unsigned>(h->r);
        a.frame_major = h->layout == COMMS_CHANNELIZER_FRAME_MAJOR;
        h->tic(s);
        comms_status_t st;
        if (h->staged)
            st = h->tab_lds ? launch_channelizer<true, true>(a, grid, h->lds, s) : launch_channelizer<true, false>(a, grid, h->lds, s);
        else
            st = h->tab_lds ? launch_channelizer<false, true>(a, grid, h->lds, s) : launch_channelizer<false, false>(a, grid, h->lds, s);
        h->toc(s);
        COMMS_TRY(st);
    }
    h->hist.flip();
    h->r = (h->r + n % h->M) % h->M;
    return COMMS_OK;
}

comms_status_t comms_channelizer_run(comms_channelizer_t* h, const comms_c32* in, size_t n, comms_c32* out) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG((in && out) || !n, "NULL host pointer");
    COMMS_TRY(use_device(h->device));
    if (!n) return COMMS_OK;
    const size_t frames = chz_frames(n, h->D);
    COMMS_ARG(n <= SIZE_MAX / 16 && frames <= SIZE_MAX / 16 / h->M, "frames * channels overflows");
    // one piece: a chunk of a channel-major call is not contiguous in the output, so the call is not pipelined
    return h->run_host(in, n * 8, out, frames * h->M * 8, [&](void* d_in, void* d_out) {
        return comms_channelizer_run_dev(h, static_cast<const comms_c32*>(d_in), n, static_cast<comms_c32*>(d_out), COMMS_STREAM_HANDLE);
    });
}

comms_status_t comms_channelizer_get_state(comms_channelizer_t* h, comms_c32* state, size_t n_state) {
    return get_history_state(h, state, n_state, "samples");
}

comms_status_t comms_channelizer_set_state(comms_channelizer_t* h, const comms_c32* state, size_t n_state) {
    return set_history_state(h, state, n_state, "samples");
}

comms_status_t comms_channelizer_get_phase(comms_channelizer_t* h, uint64_t* out_phase) {
    COMMS_ARG(h && out_phase, "NULL argument");
    *out_phase = h->r;
    return COMMS_OK;
}

comms_status_t comms_channelizer_set_phase(comms_channelizer_t* h, uint64_t t) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    h->r = t % h->M;
    return COMMS_OK;
}

comms_status_t comms_channelizer_get_kernel(const comms_channelizer_t* h, size_t n, char* name, size_t name_len) {
    COMMS_ARG(h && name && name_len, "NULL argument");
    if (h->series || forced_series()) {
        int32_t kind = -1;  // comms_chain_is_fused of the channels' chains (made on first use where the series is forced)
        if (!h->chains.empty()) COMMS_TRY(comms_chain_is_fused(h->chains[0].get(), &kind));
        std::snprintf(name, name_len, "series: chz_prep_kernel + %zu x comms_chain (kind %d) + chz_scatter_kernel", h->M, kind);
    } else {
        size_t tiles = 0, per = 0;
        const unsigned grid = chz_grid(h, chz_frames(n, h->D), &tiles, &per);
        std::snprintf(name, name_len, "channelizer_kernel<%s, %s> M=%zu frames/tile=%d lds=%zu tiles=%zu grid=%u max_grid=%u",
                      h->staged ? "samples in LDS" : "samples in global memory", h->tab_lds ? "taps in LDS" : "taps in global memory", h->M, h->F,
                      h->lds, tiles, grid, h->max_grid);
    }
    return COMMS_OK;
}

comms_status_t comms_channelizer_set_timer(comms_channelizer_t* h, comms_timer_t* t) {
    COMMS_TRY(set_handle_timer(h, t));
    if (!h->chains.empty()) return comms_chain_set_timer(h->chains[0].get(), t);  // the series: the pair brackets channel 0's FIR launch
    return COMMS_OK;
}

comms_status_t comms_channelizer_destroy(comms_channelizer_t* h) { return destroy_handle(h); }

}  // extern "C"
