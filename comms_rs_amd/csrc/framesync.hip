// framesync.hip -- frame synchroniser: normalised correlation of a Complex<f32> symbol stream with a known word, the peak
// search and the threshold in one launch that writes nothing but its detections.
//
// The reference has no such block (examples/qpsk_zmq.rs stops at symbols); the contract is include/comms_hip.h's:
//   c[k] = sum_j y[k+j] conj(p[j]),  e[k] = sum_j |y[k+j]|^2,  m[k] = |c[k]|^2 / (Ep e[k])   (0 where e[k] == 0)
//   k is a detection iff  k >= origin,  m[k] >= thr,  m[k] > m[k-j] and m[k] >= m[k+j] for j = 1 .. G.
// The existing route to c[k] is BatchFirNode with the conjugated, reversed word as taps: 8 bytes written per position, no
// normalisation, and the peak search left to the host.
//
// framesync_kernel (2 <= P <= 512, G <= 512), 8 bytes of HBM read per symbol, nothing written per symbol:
//   * a call on n symbols decides the n positions k_first .. k_first + n - 1, k_first = T - (P + G) + 1: the last position
//     whose guard window [k - G, k + G] and every window in it end inside the T + n symbols seen so far.  The handle's
//     History holds the H = P + 2 G - 1 raw symbols in front of the call, which is exactly the reach of the first position.
//   * workgroups are persistent and walk tiles of 2048 decided positions, tile t, t + gridDim.x, ...  A tile stages the
//     2048 + 2 G + P - 1 symbols of its positions and of their guard windows (history, input, or zero in front of the history
//     and past the input) into a padded LDS image (one pad slot per eight elements, as syncest_kernel's).
//   * a lane owns EIGHT neighbouring positions and slides a register window over the image: one ds_read_b64 per tap feeds
//     the eight positions, i.e. 16 packed FMAs of c and 16 FMAs of e.  conj(p) comes by scalar loads as SGPR operands of
//     v_pk_fma_f32 (sgpr_mac.hpp), eight taps per block; the taps past P in the last block are SKIPPED (a wave-uniform
//     branch), not padded with zeros: a NaN symbol reaches the windows that hold it and no other.
//   * per tap j, ascending from accumulators of +0:  cr = fma(yr, pr, cr); ci = fma(yi, pr, ci); cr = fma(yi, pi, cr);
//     ci = fma(-yr, pi, ci); e = fma(yr, yr, e); e = fma(yi, yi, e).  Then m = (cr cr + ci ci) / (Ep e), each operation
//     rounded on its own.  A position's c, e and m depend on its own P symbols only: the same bits in every call or tile.
//   * the 2048 + 2 G metrics of a tile stay in LDS; the guard scan runs only for positions with m >= thr.  A winning lane
//     forms c and e of its position again with the same chain of FMAs and appends {k, c, m, e} to the handle's list through
//     an ordinary vector atomic counter.  Detections are more than G apart, so a call has at most ceil(n / (G + 1)): the
//     list is sized to that bound before the launch and cannot overflow.  The host copies the count and the entries back and
//     sorts them by index: the order of arrival does not show.
//   * workgroup 0 writes the new history to the other half of the ping-pong pair (History, common.hpp).
#include <cmath>
#include <vector>

#include "common.hpp"
#include "fir_handle.hpp"
#include "sgpr_mac.hpp"
#include "stream_call.hpp"

namespace comms {

constexpr int FS_WG = 256;                  // lanes per workgroup
constexpr int FS_OPL = 8;                   // neighbouring positions per lane
constexpr int FS_PASS = FS_WG * FS_OPL;     // metrics per pass of the workgroup
constexpr int FS_TILE = 2048;               // decided positions per tile
constexpr int FS_SLACK = 16;                // image elements past the staged ones that the register window may load (unused values)
constexpr size_t FS_MIN_WORD = 2, FS_MAX_WORD = 512, FS_MAX_GUARD = 512;

// LDS image: element e at e + (e >> 3), so that lanes eight elements (72 bytes) apart spread over all the banks
__host__ __device__ __forceinline__ int fs_slot(int e) { return e + (e >> 3); }

struct FsArgs {
    const float2* in;       // n symbols
    const float2* hist;     // the H symbols in front of them, time order
    float2* new_hist;
    const float* tre;       // re p[j], padded with zeros to a multiple of eight
    const float* tim;       // -im p[j]
    size_t n, tiles;
    long long k_first;      // stream index of the call's first decided position
    long long origin;       // positions below it are no detections
    int P, G, H;
    int NM, NS;             // metrics and staged symbols per tile: FS_TILE + 2 G, NM + P - 1
    float thr, Ep;
    unsigned* count;
    comms_frame_detection_t* list;
    unsigned list_cap;
};

__device__ __forceinline__ float fs_metric(float cr, float ci, float e, float Ep) {
    const float num = __fadd_rn(__fmul_rn(cr, cr), __fmul_rn(ci, ci));
    const float den = __fmul_rn(Ep, e);
    return e == 0.0f ? 0.0f : num / den;
}

__global__ __launch_bounds__(FS_WG) void framesync_kernel(const FsArgs a) {
    extern __shared__ __attribute__((aligned(16))) cf fs_smem[];
    const int tid = threadIdx.x;
    const int P = a.P, G = a.G, NM = a.NM, NS = a.NS;
    cf* ys = fs_smem;                                                         // fs_slot(NS + FS_SLACK) + 1 slots
    float* ms = reinterpret_cast<float*>(ys + fs_slot(NS + FS_SLACK) + 1);   // NM metrics
    typedef const __attribute__((address_space(4))) v2f* const_v2f_ptr;       // constant address space: scalar loads
    const const_v2f_ptr tre = (const_v2f_ptr)a.tre, tim = (const_v2f_ptr)a.tim;

    for (size_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const size_t q0 = tile * static_cast<size_t>(FS_TILE);   // first decided position of the tile, counted in the call
        // metric mi of the tile is position q0 - G + mi; its tap j meets staged element mi + j, symbol g0 + mi + j of the call
        const long long g0 = static_cast<long long>(q0) - a.H;
        __syncthreads();  // the previous tile's image and metrics have been read
        for (int base = 0; base < NS; base += 4 * FS_WG) {
            float2 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = base + u * FS_WG + tid;
                v[u] = j < NS ? stream_at(a.in, a.hist, a.H, g0 + j, a.n) : make_float2(0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = base + u * FS_WG + tid;
                if (j < NS) ys[fs_slot(j)] = cf{v[u].x, v[u].y};
            }
        }
        __syncthreads();

        // ---- metrics: lane t of a pass holds mi0 .. mi0 + 7; w[i] is staged element mi0 + jb + i
        for (int pb = 0; pb < NM; pb += FS_PASS) {
            const int mi0 = pb + FS_OPL * tid;
            if (mi0 >= NM) continue;
            cf acc[FS_OPL];
            float en[FS_OPL];
#pragma unroll
            for (int c = 0; c < FS_OPL; ++c) {
                acc[c] = cf{0.f, 0.f};
                en[c] = 0.f;
            }
            cf w[16];
            const cf* wp = ys + fs_slot(mi0);  // mi0 is a multiple of eight: elements 0 .. 7 are contiguous, 8 .. 15 start at 9
#pragma unroll
            for (int i = 0; i < 8; ++i) w[i] = wp[i];
            for (int jb = 0; jb < P; jb += 8) {
#pragma unroll
                for (int i = 0; i < 8; ++i) w[8 + i] = wp[9 + i];
                v2f pr[4], pi[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    pr[i] = tre[jb / 2 + i];
                    pi[i] = tim[jb / 2 + i];
                }
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) {
                    if (jb + jj < P) {  // wave-uniform
#pragma unroll
                        for (int c = 0; c < FS_OPL; ++c) {
                            const cf u = w[c + jj];
                            mac_tap<false>(acc[c], u, pr[jj / 2], pi[jj / 2], jj & 1);
                            en[c] = __builtin_fmaf(u.x, u.x, en[c]);
                            en[c] = __builtin_fmaf(u.y, u.y, en[c]);
                        }
                    }
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) w[i] = w[8 + i];
                wp += 9;
            }
#pragma unroll
            for (int c = 0; c < FS_OPL; ++c)
                if (mi0 + c < NM) ms[mi0 + c] = fs_metric(acc[c].x, acc[c].y, en[c], a.Ep);
        }
        __syncthreads();

        // ---- decisions: position q0 + r has metric r + G; comparisons with a NaN are false
        for (int r = tid; r < FS_TILE; r += FS_WG) {
            const size_t q = q0 + static_cast<size_t>(r);
            if (q >= a.n) break;
            const float m = ms[r + G];
            const long long k = a.k_first + static_cast<long long>(q);
            if (!(m >= a.thr) || k < a.origin) continue;
            bool peak = true;
            for (int j = 1; j <= G && peak; ++j) peak = (m > ms[r + G - j]) && (m >= ms[r + G + j]);
            if (!peak) continue;
            float cr = 0.f, ci = 0.f, e = 0.f;
            for (int j = 0; j < P; ++j) {
                const cf u = ys[fs_slot(r + G + j)];
                const float tr = a.tre[j], ti = a.tim[j];
                cr = __builtin_fmaf(u.x, tr, cr);
                ci = __builtin_fmaf(u.y, tr, ci);
                cr = __builtin_fmaf(-u.y, ti, cr);
                ci = __builtin_fmaf(u.x, ti, ci);
                e = __builtin_fmaf(u.x, u.x, e);
                e = __builtin_fmaf(u.y, u.y, e);
            }
            const unsigned at = atomicAdd(a.count, 1u);
            if (at < a.list_cap) {  // always: detections are more than G apart
                comms_frame_detection_t d;
                d.index = static_cast<uint64_t>(k);
                d.corr_re = cr;
                d.corr_im = ci;
                d.metric = fs_metric(cr, ci, e, a.Ep);
                d.energy = e;
                a.list[at] = d;
            }
        }
    }

    hist_advance(a.hist, a.in, a.n, a.new_hist, a.H);
}

}  // namespace comms

using namespace comms;

struct comms_framesync : Handle {
    int P = 0, G = 0, H = 0, NM = 0, NS = 0;
    float thr = 0.f, Ep = 0.f;
    uint64_t T = 0;            // symbols seen: the stream index of the next one
    long long origin = 0;      // positions below it are no detections (0; the position of the last flush)
    size_t lds = 0;
    unsigned max_grid = 1;
    DevBuf<float> d_taps;      // [2][P padded to a multiple of eight]: re p, -im p
    int NP8 = 0;
    DevBuf<float2> d_zero;     // P + G zero symbols (flush)
    Scratch list;              // count (8 bytes), then the detections of a call
    History hist;              // last H symbols
};
static_assert(!std::is_copy_constructible_v<comms_framesync>, "a handle is never copied");

namespace {

comms_status_t check_word_guard(size_t n_word, size_t guard) {
    COMMS_ARG(n_word >= FS_MIN_WORD && n_word <= FS_MAX_WORD, "n_word must be %zu ... %zu symbols (got %zu)", FS_MIN_WORD, FS_MAX_WORD, n_word);
    COMMS_ARG(guard <= FS_MAX_GUARD, "guard must be at most %zu positions (got %zu)", FS_MAX_GUARD, guard);
    return COMMS_OK;
}

size_t framesync_tiles(size_t n) { return (n + FS_TILE - 1) / FS_TILE; }
size_t framesync_grid(const comms_framesync* h, size_t n) { return tile_grid(framesync_tiles(n), h->max_grid); }

// One launch on n symbols at d_in and its detections (detection_step); history and position advance.  Ends synchronised.
comms_status_t framesync_step(comms_framesync* h, const comms_c32* d_in, size_t n, comms_frame_detection_t* out, size_t cap,
                              size_t* n_found, void* stream) {
    hipStream_t s = nullptr;
    COMMS_TRY(h->enter(stream, &s));
    auto launch = [&](unsigned* count, comms_frame_detection_t* list, unsigned list_cap) -> comms_status_t {
        FsArgs a{};
        a.in = reinterpret_cast<const float2*>(d_in);
        a.hist = h->hist.cur<float2>();
        a.new_hist = h->hist.next<float2>();
        a.tre = h->d_taps.get();
        a.tim = h->d_taps.get() + h->NP8;
        a.n = n;
        a.tiles = framesync_tiles(n);
        a.k_first = static_cast<long long>(h->T) - (h->P + h->G) + 1;
        a.origin = h->origin;
        a.P = h->P;
        a.G = h->G;
        a.H = h->H;
        a.NM = h->NM;
        a.NS = h->NS;
        a.thr = h->thr;
        a.Ep = h->Ep;
        a.count = count;
        a.list = list;
        a.list_cap = list_cap;
        h->tic(s);
        const comms_status_t st = launch_kernel<framesync_kernel>("framesync_kernel", dim3(static_cast<unsigned>(framesync_grid(h, n))),
                                                                  dim3(FS_WG), h->lds, s, {}, a);
        h->toc(s);
        COMMS_TRY(st);
        h->hist.flip();
        h->T += n;
        return COMMS_OK;
    };
    return detection_step(h->list, detection_bound(n, static_cast<size_t>(h->G)), s, "framesync_kernel", launch, out, cap, n_found);
}

}  // namespace

extern "C" {

comms_status_t comms_framesync_state_len(size_t n_word, size_t guard, size_t* out_len) {
    COMMS_ARG(out_len != nullptr, "out_len is NULL");
    COMMS_TRY(check_word_guard(n_word, guard));
    *out_len = n_word + 2 * guard - 1;
    return COMMS_OK;
}

comms_status_t comms_framesync_create(const comms_c32* word, size_t n_word, double threshold, size_t guard, int32_t device,
                                      comms_framesync_t** out) {
    COMMS_ARG(out != nullptr, "out is NULL");
    *out = nullptr;
    COMMS_ARG(word != nullptr, "word is NULL");
    COMMS_TRY(check_word_guard(n_word, guard));
    COMMS_TRY(check_threshold(threshold));
    double ep = 0.0;
    for (size_t j = 0; j < n_word; ++j) {
        COMMS_ARG(std::isfinite(word[j].re) && std::isfinite(word[j].im), "word[%zu] is not finite", j);
        ep += static_cast<double>(word[j].re) * word[j].re + static_cast<double>(word[j].im) * word[j].im;
    }
    COMMS_ARG(static_cast<float>(ep) > 0.0f && std::isfinite(static_cast<float>(ep)), "the word has no energy (or too much for f32)");
    HandlePtr<comms_framesync> h;
    COMMS_TRY(make_handle(device, &h));
    h->P = static_cast<int>(n_word);
    h->G = static_cast<int>(guard);
    h->H = h->P + 2 * h->G - 1;
    h->NM = FS_TILE + 2 * h->G;
    h->NS = h->NM + h->P - 1;
    h->thr = static_cast<float>(threshold);
    h->Ep = static_cast<float>(ep);
    h->NP8 = (h->P + 7) / 8 * 8;
    h->lds = static_cast<size_t>(fs_slot(h->NS + FS_SLACK) + 1) * sizeof(float2) + static_cast<size_t>(h->NM) * sizeof(float);
    h->max_grid = resident_workgroups(h->lds);
    std::vector<float> taps(2 * static_cast<size_t>(h->NP8), 0.0f);
    for (size_t j = 0; j < n_word; ++j) {
        taps[j] = word[j].re;
        taps[h->NP8 + j] = -word[j].im;
    }
    COMMS_HIP_TRY(h->d_taps.upload(taps));
    COMMS_HIP_TRY(h->d_zero.alloc_zero(static_cast<size_t>(h->P + h->G)));
    COMMS_HIP_TRY(h->hist.alloc(static_cast<size_t>(h->H), sizeof(comms_c32)));
    *out = h.release();
    return COMMS_OK;
}

comms_status_t comms_framesync_run_dev(comms_framesync_t* h, const comms_c32* d_in, size_t n, comms_frame_detection_t* out, size_t cap,
                                       size_t* n_found, void* stream) {
    COMMS_TRY(detect_prologue(h, d_in, n, true, out, cap, n_found));
    if (!n) return COMMS_OK;
    return framesync_step(h, d_in, n, out, cap, n_found, stream);
}

comms_status_t comms_framesync_run(comms_framesync_t* h, const comms_c32* in, size_t n, comms_frame_detection_t* out, size_t cap,
                                   size_t* n_found) {
    COMMS_TRY(detect_prologue(h, in, n, false, out, cap, n_found));
    if (!n) return COMMS_OK;
    const void* d = nullptr;
    COMMS_TRY(stage_input(h, in, n * 8, &d));
    return framesync_step(h, static_cast<const comms_c32*>(d), n, out, cap, n_found, COMMS_STREAM_HANDLE);
}

comms_status_t comms_framesync_flush(comms_framesync_t* h, comms_frame_detection_t* out, size_t cap, size_t* n_found) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    const comms_c32* zeros = reinterpret_cast<const comms_c32*>(h->d_zero.get());
    const size_t n = static_cast<size_t>(h->P + h->G);
    COMMS_TRY(detect_prologue(h, zeros, n, true, out, cap, n_found));
    const uint64_t T = h->T;
    COMMS_TRY(framesync_step(h, zeros, n, out, cap, n_found, COMMS_STREAM_HANDLE));
    h->T = T;
    h->origin = static_cast<long long>(T);
    COMMS_HIP_TRY(h->hist.upload(nullptr, 0));  // zeros (the step ended synchronised)
    return COMMS_OK;
}

comms_status_t comms_framesync_get_state(comms_framesync_t* h, comms_c32* state, size_t n_state) {
    return get_history_state(h, state, n_state, "symbols");
}

// (n_state must be H = P + 2 G - 1 >= 1: a NULL state never comes with a length the setter accepts)
comms_status_t comms_framesync_set_state(comms_framesync_t* h, const comms_c32* state, size_t n_state) {
    return set_history_state(h, state, n_state, "symbols");
}

comms_status_t comms_framesync_get_position(const comms_framesync_t* h, uint64_t* out_position) { return get_position(h, out_position); }

comms_status_t comms_framesync_set_position(comms_framesync_t* h, uint64_t position) {
    return set_position(h, position, [&] { h->origin = 0; });
}

comms_status_t comms_framesync_set_threshold(comms_framesync_t* h, double threshold) { return set_threshold(h, threshold); }

comms_status_t comms_framesync_get_kernel(const comms_framesync_t* h, size_t n, char* name, size_t name_len) {
    COMMS_ARG(h && name && name_len, "NULL argument");
    std::snprintf(name, name_len, "framesync_kernel tile=%d wg=%d word=%d guard=%d lds=%zu tiles=%zu grid=%zu max_grid=%u", FS_TILE, FS_WG,
                  h->P, h->G, h->lds, framesync_tiles(n), framesync_grid(h, n), h->max_grid);
    return COMMS_OK;
}

comms_status_t comms_framesync_set_timer(comms_framesync_t* h, comms_timer_t* t) { return set_handle_timer(h, t); }

comms_status_t comms_framesync_destroy(comms_framesync_t* h) { return destroy_handle(h); }

}  // extern "C"
