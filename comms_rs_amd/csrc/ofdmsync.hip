// ofdmsync.hip -- OFDM stream synchroniser: the stream correlated with itself at a lag (Schmidl-Cox in its repeated-symbol
// form), the peak search and the threshold in one launch that writes nothing but its detections; and the per-frame
// derotation of extracted records by their own frequency offset in a second one.
//
// The reference has no such block; the contract is include/comms_hip.h's ("OFDM synchroniser"):
//   P[d] = sum_{m<W} conj(r[d+m]) r[d+m+L],  R[d] = 1/2 sum_{m<W} (|r[d+m]|^2 + |r[d+m+L]|^2),  m[d] = |P|^2 / R^2
//   d is a detection iff  d >= origin + A,  m[d] >= thr,  m[d] > m[d-j] and m[d] >= m[d+j] for j = 1 .. G;  index = d - A.
//
// ofdmsync_detect_kernel (1 <= L <= 2048, 2 <= W <= 2048, G <= 512), 8 bytes of HBM read per sample, nothing written per sample:
//   * a call on n samples decides the n positions d_first .. d_first + n - 1, d_first = T - (W + L + G) + 1; the handle's
//     History holds the H = W + L + 2 G - 1 raw samples in front of the call, the reach of the first position's guard window.
//   * one workgroup per tile of 2048 decided positions (a plain grid).  A tile stages the samples of its 2048 + 2 G metrics,
//     from the 32-aligned ABSOLUTE index at or below its first one, into a padded LDS image (one pad slot per 32 elements:
//     lanes 32 elements apart meet different banks).
//   * per absolute index i:  q[i] = conj(r[i]) r[i+L]  as  qr = fma(ai, ci, ar cr), qi = fma(-ai, cr, ar ci)  and
//     b[i] = fma(ci, ci, fma(cr, cr, fma(ai, ai, ar ar)))   (a = r[i], c = r[i+L]; the inner product rounded first).
//   * blocks of 32 absolute indices [32 k, 32 k + 32).  One lane per block walks it twice: ascending from +0 for the prefix
//     sums pre[i] = q[32 k] + ... + q[i] and the block total F[k] = pre[32 k + 31]; descending from +0 for the suffix sums
//     suf[i] = q[i] + (q[i+1] + ...).  Half of the workgroup takes the prefixes, the other half the suffixes.
//   * with e = d + W - 1, kd = floor(d / 32), ke = floor(e / 32):
//       ke > kd:   P[d] = (suf[d] + mid) + pre[e],  mid = (((+0 + F[kd+1]) + F[kd+2]) + ...) + F[ke-1]
//       ke == kd:  P[d] = ((+0 + q[d]) + q[d+1]) + ... + q[e]
//     and the sum B[d] of b likewise; R = B / 2; m = (Pr Pr + Pi Pi) / (R R), every operation rounded on its own, 0 where
//     R == 0.  Every term is a function of absolute indices in [d, e + L] only: the same bits in every call and tile, and a NaN
//     reaches the windows that hold it and no other.
//   * a lane owns EIGHT neighbouring positions 8 g .. 8 g + 7 (absolute, so all in one block): they share `mid` up to the
//     block of the first one's end, and the positions whose end lies one block further add that block.
//   * the metrics of a tile stay in LDS; the guard scan runs only where m >= thr.  A winning lane forms P and B of its position
//     again in the same order and appends {d - A, P, m, R} to the handle's list through an ordinary vector atomic counter.
//   * workgroup 0 writes the new history to the other half of the ping-pong pair (History, common.hpp).
//
// ofdmsync_correct_kernel: out[f][n] = in[f][n] exp(-i cfo[f] n) over the flattened (frame, eight samples) space.  A lane
// takes the f64 anchor sincos(-(cfo n0)) at n0 = 8 j, rounds it to f32 and steps it by the frame's f32 rotor exp(-i cfo)
// (formed in f64 on the host): 16-byte loads and stores where the record length is even.
#include <cmath>
#include <vector>

#include "common.hpp"
#include "fir_handle.hpp"
#include "stream_call.hpp"

namespace comms {

constexpr int OS_WG = 512;                  // lanes per workgroup of the detect kernel
constexpr int OS_HALF = OS_WG / 2;          // lanes that take prefixes; the others take suffixes (whole waves each)
constexpr int OS_OPL = 8;                   // neighbouring positions per lane
constexpr int OS_TILE = 2048;               // decided positions per tile
constexpr int OS_BLK = 32;                  // absolute indices per block of prefix / suffix sums
constexpr size_t OS_MAX_LAG = 2048, OS_MIN_WINDOW = 2, OS_MAX_WINDOW = 2048, OS_MAX_GUARD = 512, OS_MAX_ADVANCE = 2048;
constexpr size_t OS_MAX_FRAME = size_t(1) << 20;
constexpr int OC_WG = 256;                  // lanes per workgroup of the correct kernel
constexpr int OC_RUN = 8;                   // samples per lane and anchor

// LDS images: element e at e + (e >> 5)
__host__ __device__ __forceinline__ int os_slot(int e) { return e + (e >> 5); }

// What a tile needs at most, whatever its first index is modulo 32 (host and device agree on the layout through OsArgs)
struct OsLayout {
    int NM;      // metrics per tile: OS_TILE + 2 G
    int NBLK;    // blocks that hold a window's index
    int NS;      // staged samples: 32 NBLK + L
    int NSUFB;   // blocks that hold a position
    int NPREB;   // blocks that hold a window's end
    size_t lds;
};
inline OsLayout os_layout(int L, int W, int G) {
    OsLayout y{};
    y.NM = OS_TILE + 2 * G;
    y.NBLK = ((OS_BLK - 1 + y.NM + W - 2) >> 5) + 1;
    y.NS = OS_BLK * y.NBLK + L;
    y.NSUFB = ((OS_BLK - 1 + y.NM - 1) >> 5) + 1;
    y.NPREB = ((y.NM - 1) >> 5) + 2;
    y.lds = static_cast<size_t>(os_slot(y.NS) + 1) * sizeof(float2) +
            (3 * static_cast<size_t>(os_slot(OS_BLK * y.NSUFB) + os_slot(OS_BLK * y.NPREB) + y.NBLK) + static_cast<size_t>(y.NM)) * sizeof(float);
    return y;
}

struct OsArgs {
    const float2* in;       // n samples
    const float2* hist;     // the H samples in front of them, time order
    float2* new_hist;
    size_t n;
    long long d_first;      // stream index of the call's first decided position
    long long d_min;        // origin + A: positions below it are no detections
    int L, W, G, A, H;
    OsLayout y;
    float thr;
    unsigned* count;
    comms_frame_detection_t* list;
    unsigned list_cap;
};

// The three LDS arrays of one kind of sum
struct OsTriple {
    float *r, *i, *b;
};
struct OsLds {
    const float2* ys;
    OsTriple suf, pre, F;
    int pre_blk;  // the block that element 0 of `pre` belongs to
};

__device__ __forceinline__ void os_prod(const float2* ys, int idx, int L, float& qr, float& qi, float& b) {
    const float2 a = ys[os_slot(idx)], c = ys[os_slot(idx + L)];
    qr = __builtin_fmaf(a.y, c.y, __fmul_rn(a.x, c.x));
    qi = __builtin_fmaf(-a.y, c.x, __fmul_rn(a.x, c.y));
    b = __builtin_fmaf(c.y, c.y, __builtin_fmaf(c.x, c.x, __builtin_fmaf(a.y, a.y, __fmul_rn(a.x, a.x))));
}

// ke == kd: the window lies inside one block
__device__ __forceinline__ void os_direct(const OsLds& s, int d, int e, int L, float& pr, float& pi, float& pb) {
    pr = pi = pb = 0.f;
    for (int i = d; i <= e; ++i) {
        float qr, qi, b;
        os_prod(s.ys, i, L, qr, qi, b);
        pr = __fadd_rn(pr, qr);
        pi = __fadd_rn(pi, qi);
        pb = __fadd_rn(pb, b);
    }
}

// `mid` of the header's order, the only place that forms it: the full blocks [from, to) added in ascending order to (mr, mi,
// mb), which hold +0 or the sum of the blocks in front of `from`.  Extending a sum by one block is the same chain of additions
// as forming it anew, so a lane may share the blocks of its eight positions.
__device__ __forceinline__ void os_mid(const OsLds& s, int from, int to, float& mr, float& mi, float& mb) {
    for (int k = from; k < to; ++k) {
        mr = __fadd_rn(mr, s.F.r[k]);
        mi = __fadd_rn(mi, s.F.i[k]);
        mb = __fadd_rn(mb, s.F.b[k]);
    }
}

// ke > kd, with `mid` given
__device__ __forceinline__ void os_join(const OsLds& s, int d, int e, float mr, float mi, float mb, float& pr, float& pi, float& pb) {
    const int sd = os_slot(d), se = os_slot(e - OS_BLK * s.pre_blk);
    pr = __fadd_rn(__fadd_rn(s.suf.r[sd], mr), s.pre.r[se]);
    pi = __fadd_rn(__fadd_rn(s.suf.i[sd], mi), s.pre.i[se]);
    pb = __fadd_rn(__fadd_rn(s.suf.b[sd], mb), s.pre.b[se]);
}

// P and B of one position (the winners)
__device__ __forceinline__ void os_position(const OsLds& s, int d, int W, int L, float& pr, float& pi, float& pb) {
    const int e = d + W - 1, kd = d >> 5, ke = e >> 5;
    if (ke == kd) {
        os_direct(s, d, e, L, pr, pi, pb);
        return;
    }
    float mr = 0.f, mi = 0.f, mb = 0.f;
    os_mid(s, kd + 1, ke, mr, mi, mb);
    os_join(s, d, e, mr, mi, mb, pr, pi, pb);
}

__device__ __forceinline__ float os_metric(float pr, float pi, float R) {
    const float num = __fadd_rn(__fmul_rn(pr, pr), __fmul_rn(pi, pi));
    const float den = __fmul_rn(R, R);
    return R == 0.0f ? 0.0f : num / den;
}

__global__ __launch_bounds__(OS_WG) void ofdmsync_detect_kernel(const OsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float2 os_smem[];
    const int tid = threadIdx.x;
    const int L = a.L, W = a.W, G = a.G, NM = a.y.NM;
    float2* ys = os_smem;
    float* fl = reinterpret_cast<float*>(ys + os_slot(a.y.NS) + 1);
    const int n_suf = os_slot(OS_BLK * a.y.NSUFB), n_pre = os_slot(OS_BLK * a.y.NPREB);
    OsLds s;
    s.ys = ys;
    s.suf = OsTriple{fl, fl + n_suf, fl + 2 * n_suf};
    fl += 3 * n_suf;
    s.pre = OsTriple{fl, fl + n_pre, fl + 2 * n_pre};
    fl += 3 * n_pre;
    s.F = OsTriple{fl, fl + a.y.NBLK, fl + 2 * a.y.NBLK};
    float* ms = fl + 3 * a.y.NBLK;  // NM metrics

    const size_t q0 = static_cast<size_t>(blockIdx.x) * OS_TILE;  // first decided position of the tile, counted in the call
    // metric mi of the tile is position d_first + q0 - G + mi; `off` is the place of metric 0 in its block of 32 absolute
    // indices, and image element idx = off + mi + m is sample g0 + idx of the call
    const long long p0 = a.d_first + static_cast<long long>(q0) - G;
    const int off = static_cast<int>(((p0 % OS_BLK) + OS_BLK) % OS_BLK);
    const long long g0 = static_cast<long long>(q0) - a.H - off;
    const int nblk = ((off + NM + W - 2) >> 5) + 1;        // <= NBLK
    const int nsufb = ((off + NM - 1) >> 5) + 1;           // <= NSUFB
    s.pre_blk = (off + W - 1) >> 5;                        // nblk - pre_blk <= NPREB
    const int ns = OS_BLK * nblk + L;                      // <= NS

    for (int base = 0; base < ns; base += 4 * OS_WG) {
        float2 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = base + u * OS_WG + tid;
            v[u] = j < ns ? stream_at(a.in, a.hist, a.H, g0 + j, a.n) : make_float2(0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = base + u * OS_WG + tid;
            if (j < ns) ys[os_slot(j)] = v[u];
        }
    }
    __syncthreads();

    // ---- prefix and suffix sums: lane -> block; the halves of the workgroup are whole waves
    {
        const bool prefix = tid < OS_HALF;
        for (int k = tid & (OS_HALF - 1); k < nblk; k += OS_HALF) {
            float ar = 0.f, ai = 0.f, ab = 0.f;
            if (prefix) {
                const bool keep = k >= s.pre_blk;
                const int at = keep ? os_slot(OS_BLK * (k - s.pre_blk)) : 0;
#pragma unroll 4
                for (int j = 0; j < OS_BLK; ++j) {
                    float qr, qi, b;
                    os_prod(ys, OS_BLK * k + j, L, qr, qi, b);
                    ar = __fadd_rn(ar, qr);
                    ai = __fadd_rn(ai, qi);
                    ab = __fadd_rn(ab, b);
                    if (keep) {
                        s.pre.r[at + j] = ar;
                        s.pre.i[at + j] = ai;
                        s.pre.b[at + j] = ab;
                    }
                }
                s.F.r[k] = ar;
                s.F.i[k] = ai;
                s.F.b[k] = ab;
            } else if (k < nsufb) {
                const int at = os_slot(OS_BLK * k);
#pragma unroll 4
                for (int j = OS_BLK - 1; j >= 0; --j) {
                    float qr, qi, b;
                    os_prod(ys, OS_BLK * k + j, L, qr, qi, b);
                    ar = __fadd_rn(qr, ar);
                    ai = __fadd_rn(qi, ai);
                    ab = __fadd_rn(b, ab);
                    s.suf.r[at + j] = ar;
                    s.suf.i[at + j] = ai;
                    s.suf.b[at + j] = ab;
                }
            }
        }
    }
    __syncthreads();

    // ---- metrics: lane -> image elements 8 g .. 8 g + 7, one block
    const int groups = (off + NM + OS_OPL - 1) / OS_OPL;
    for (int g = tid; g < groups; g += OS_WG) {
        const int idx0 = g * OS_OPL, kd = idx0 >> 5, ke0 = (idx0 + W - 1) >> 5;
        // a position's end lies in block ke0 or ke0 + 1: mid over [kd + 1, ke0), and the same extended by block ke0.  A block
        // past nblk belongs only to positions that are not stored.
        float mr = 0.f, mi = 0.f, mb = 0.f;
        os_mid(s, kd + 1, min(ke0, nblk), mr, mi, mb);
        float nr = mr, ni = mi, nb = mb;
        os_mid(s, max(ke0, kd + 1), min(ke0 + 1, nblk), nr, ni, nb);
#pragma unroll
        for (int c = 0; c < OS_OPL; ++c) {
            const int d = idx0 + c, m_at = d - off;
            if (m_at < 0 || m_at >= NM) continue;
            const int e = d + W - 1, ke = e >> 5;
            float pr, pi, pb;
            if (ke == kd)
                os_direct(s, d, e, L, pr, pi, pb);
            else if (ke == ke0)
                os_join(s, d, e, mr, mi, mb, pr, pi, pb);
            else
                os_join(s, d, e, nr, ni, nb, pr, pi, pb);
            ms[m_at] = os_metric(pr, pi, __fmul_rn(0.5f, pb));
        }
    }
    __syncthreads();

    // ---- decisions: position q0 + r has metric r + G; comparisons with a NaN are false
    for (int r = tid; r < OS_TILE; r += OS_WG) {
        const size_t q = q0 + static_cast<size_t>(r);
        if (q >= a.n) break;
        const float m = ms[r + G];
        const long long d_abs = a.d_first + static_cast<long long>(q);
        if (!(m >= a.thr) || d_abs < a.d_min) continue;
        bool peak = true;
        for (int j = 1; j <= G && peak; ++j) peak = (m > ms[r + G - j]) && (m >= ms[r + G + j]);
        if (!peak) continue;
        float pr, pi, pb;
        os_position(s, off + r + G, W, L, pr, pi, pb);
        const unsigned at = atomicAdd(a.count, 1u);
        if (at < a.list_cap) {  // always: detections are more than G apart
            const float R = __fmul_rn(0.5f, pb);
            comms_frame_detection_t det;
            det.index = static_cast<uint64_t>(d_abs - a.A);
            det.corr_re = pr;
            det.corr_im = pi;
            det.metric = os_metric(pr, pi, R);
            det.energy = R;
            a.list[at] = det;
        }
    }

    hist_advance(a.hist, a.in, a.n, a.new_hist, a.H);
}

// ---- the correct stage
struct OcDesc {
    double cfo;     // rad / sample
    float c1, s1;   // exp(-i cfo), f64 rounded to f32
};
struct OcArgs {
    const float2* in;
    float2* out;
    const OcDesc* desc;
    size_t lanes;        // n_frames * runs
    unsigned n_frame;
    unsigned runs;       // ceil(n_frame / 8)
    int wide;            // n_frame is even: every run starts on 16 bytes
};

__device__ __forceinline__ float2 oc_turn(float2 x, float c, float s) {
    return make_float2(__builtin_fmaf(-x.y, s, __fmul_rn(x.x, c)), __builtin_fmaf(x.y, c, __fmul_rn(x.x, s)));
}

__global__ __launch_bounds__(OC_WG) void ofdmsync_correct_kernel(const OcArgs a) {
    const size_t lane = static_cast<size_t>(blockIdx.x) * OC_WG + threadIdx.x;
    if (lane >= a.lanes) return;
    const size_t f = lane / a.runs;
    const unsigned n0 = static_cast<unsigned>(lane - f * a.runs) * OC_RUN;
    const OcDesc d = a.desc[f];
    double sn, cs;
    sincos(-(d.cfo * static_cast<double>(n0)), &sn, &cs);
    float c = static_cast<float>(cs), s = static_cast<float>(sn);
    const size_t at = f * a.n_frame + n0;
    const unsigned left = a.n_frame - n0;
    if (a.wide && left >= OC_RUN) {
        const float4* src = reinterpret_cast<const float4*>(a.in + at);
        float4 v[OC_RUN / 2];
#pragma unroll
        for (int u = 0; u < OC_RUN / 2; ++u) v[u] = src[u];
#pragma unroll
        for (int u = 0; u < OC_RUN / 2; ++u) {
            const float2 y0 = oc_turn(make_float2(v[u].x, v[u].y), c, s);
            float c2 = __builtin_fmaf(-s, d.s1, __fmul_rn(c, d.c1)), s2 = __builtin_fmaf(s, d.c1, __fmul_rn(c, d.s1));
            const float2 y1 = oc_turn(make_float2(v[u].z, v[u].w), c2, s2);
            c = __builtin_fmaf(-s2, d.s1, __fmul_rn(c2, d.c1));
            s = __builtin_fmaf(s2, d.c1, __fmul_rn(c2, d.s1));
            v[u] = make_float4(y0.x, y0.y, y1.x, y1.y);
        }
        float4* dst = reinterpret_cast<float4*>(a.out + at);
#pragma unroll
        for (int u = 0; u < OC_RUN / 2; ++u) dst[u] = v[u];
    } else {
        const unsigned cnt = left < OC_RUN ? left : OC_RUN;
        for (unsigned u = 0; u < cnt; ++u) {
            a.out[at + u] = oc_turn(a.in[at + u], c, s);
            const float c2 = __builtin_fmaf(-s, d.s1, __fmul_rn(c, d.c1));
            s = __builtin_fmaf(s, d.c1, __fmul_rn(c, d.s1));
            c = c2;
        }
    }
}

}  // namespace comms

using namespace comms;

struct comms_ofdmsync : Handle {
    int L = 0, W = 0, G = 0, A = 0, H = 0;
    size_t n_frame = 0;        // record length of the correct stage (0: none)
    OsLayout y{};
    float thr = 0.f;
    uint64_t T = 0;            // samples seen: the stream index of the next one
    long long origin = 0;      // indices below it are not reported (0; the position of the last flush)
    DevBuf<float2> d_zero;     // W + L + G zero samples (flush)
    Scratch list;              // count (8 bytes), then the detections of a call
    History hist;              // last H samples
    Pinned desc_host;          // the cfo table of a correct call as the host writes it ...
    Scratch desc_dev;          // ... and where the launch reads it
};
static_assert(!std::is_copy_constructible_v<comms_ofdmsync>, "a handle is never copied");

namespace {

comms_status_t check_shape(size_t lag, size_t window, size_t guard) {
    COMMS_ARG(lag >= 1 && lag <= OS_MAX_LAG, "lag must be 1 ... %zu samples (got %zu)", OS_MAX_LAG, lag);
    COMMS_ARG(window >= OS_MIN_WINDOW && window <= OS_MAX_WINDOW, "window must be %zu ... %zu samples (got %zu)", OS_MIN_WINDOW,
              OS_MAX_WINDOW, window);
    COMMS_ARG(guard <= OS_MAX_GUARD, "guard must be at most %zu positions (got %zu)", OS_MAX_GUARD, guard);
    return COMMS_OK;
}

size_t tiles_of(size_t n) { return (n + OS_TILE - 1) / OS_TILE; }

// One launch on n samples at d_in and its detections (detection_step), then their CFO column; history and position advance.
// Ends synchronised.
comms_status_t detect_step(comms_ofdmsync* h, const comms_c32* d_in, size_t n, comms_frame_detection_t* out, double* cfo_out, size_t cap,
                           size_t* n_found, void* stream) {
    hipStream_t s = nullptr;
    COMMS_TRY(h->enter(stream, &s));
    COMMS_ARG(tiles_of(n) <= 0x7FFFFFFFull, "n is too long for one call");
    auto launch = [&](unsigned* count, comms_frame_detection_t* list, unsigned list_cap) -> comms_status_t {
        OsArgs a{};
        a.in = reinterpret_cast<const float2*>(d_in);
        a.hist = h->hist.cur<float2>();
        a.new_hist = h->hist.next<float2>();
        a.n = n;
        a.d_first = static_cast<long long>(h->T) - (h->W + h->L + h->G) + 1;
        a.d_min = h->origin + h->A;
        a.L = h->L;
        a.W = h->W;
        a.G = h->G;
        a.A = h->A;
        a.H = h->H;
        a.y = h->y;
        a.thr = h->thr;
        a.count = count;
        a.list = list;
        a.list_cap = list_cap;
        COMMS_TRY(launch_kernel<ofdmsync_detect_kernel>("ofdmsync_detect_kernel", dim3(static_cast<unsigned>(tiles_of(n))), dim3(OS_WG), h->y.lds,
                                                        s, h->take_events(), a));
        h->hist.flip();
        h->T += n;
        return COMMS_OK;
    };
    COMMS_TRY(detection_step(h->list, detection_bound(n, static_cast<size_t>(h->G)), s, "ofdmsync_detect_kernel", launch, out, cap, n_found));
    if (cfo_out)
        for (size_t i = 0; i < *n_found && i < cap; ++i)
            cfo_out[i] = std::atan2(static_cast<double>(out[i].corr_im), static_cast<double>(out[i].corr_re)) / static_cast<double>(h->L);
    return COMMS_OK;
}

// records of n_frame samples in and out
FrameCall correct_call(const comms_ofdmsync* h) {
    const size_t bytes = h->n_frame * sizeof(comms_c32);
    return {bytes, bytes, 16, 16, (size_t(1) << 31) / h->n_frame};
}

}  // namespace

extern "C" {

comms_status_t comms_ofdmsync_state_len(size_t lag, size_t window, size_t guard, size_t* out_len) {
    COMMS_ARG(out_len != nullptr, "out_len is NULL");
    COMMS_TRY(check_shape(lag, window, guard));
    *out_len = window + lag + 2 * guard - 1;
    return COMMS_OK;
}

comms_status_t comms_ofdmsync_create(size_t lag, size_t window, double threshold, size_t guard, size_t advance, size_t n_frame, int32_t device,
                                     comms_ofdmsync_t** out) {
    COMMS_ARG(out != nullptr, "out is NULL");
    *out = nullptr;
    COMMS_TRY(check_shape(lag, window, guard));
    COMMS_TRY(check_threshold(threshold));
    COMMS_ARG(advance <= OS_MAX_ADVANCE, "advance must be at most %zu samples (got %zu)", OS_MAX_ADVANCE, advance);
    COMMS_ARG(n_frame <= OS_MAX_FRAME, "n_frame must be 0 or 1 ... %zu samples (got %zu)", OS_MAX_FRAME, n_frame);
    HandlePtr<comms_ofdmsync> h;
    COMMS_TRY(make_handle(device, &h));
    h->L = static_cast<int>(lag);
    h->W = static_cast<int>(window);
    h->G = static_cast<int>(guard);
    h->A = static_cast<int>(advance);
    h->H = h->W + h->L + 2 * h->G - 1;
    h->n_frame = n_frame;
    h->y = os_layout(h->L, h->W, h->G);
    h->thr = static_cast<float>(threshold);
    COMMS_HIP_TRY(h->d_zero.alloc_zero(static_cast<size_t>(h->W + h->L + h->G)));
    COMMS_HIP_TRY(h->hist.alloc(static_cast<size_t>(h->H), sizeof(comms_c32)));
    *out = h.release();
    return COMMS_OK;
}

comms_status_t comms_ofdmsync_run_dev(comms_ofdmsync_t* h, const comms_c32* d_in, size_t n, comms_frame_detection_t* out, double* cfo_out,
                                      size_t cap, size_t* n_found, void* stream) {
    COMMS_TRY(detect_prologue(h, d_in, n, true, out, cap, n_found));
    if (!n) return COMMS_OK;
    return detect_step(h, d_in, n, out, cfo_out, cap, n_found, stream);
}

comms_status_t comms_ofdmsync_run(comms_ofdmsync_t* h, const comms_c32* in, size_t n, comms_frame_detection_t* out, double* cfo_out, size_t cap,
                                  size_t* n_found) {
    COMMS_TRY(detect_prologue(h, in, n, false, out, cap, n_found));
    if (!n) return COMMS_OK;
    const void* d = nullptr;
    COMMS_TRY(stage_input(h, in, n * 8, &d));
    return detect_step(h, static_cast<const comms_c32*>(d), n, out, cfo_out, cap, n_found, COMMS_STREAM_HANDLE);
}

comms_status_t comms_ofdmsync_flush(comms_ofdmsync_t* h, comms_frame_detection_t* out, double* cfo_out, size_t cap, size_t* n_found) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    const comms_c32* zeros = reinterpret_cast<const comms_c32*>(h->d_zero.get());
    const size_t n = static_cast<size_t>(h->W + h->L + h->G);
    COMMS_TRY(detect_prologue(h, zeros, n, true, out, cap, n_found));
    const uint64_t T = h->T;
    COMMS_TRY(detect_step(h, zeros, n, out, cfo_out, cap, n_found, COMMS_STREAM_HANDLE));
    h->T = T;
    h->origin = static_cast<long long>(T);
    COMMS_HIP_TRY(h->hist.upload(nullptr, 0));  // zeros (the step ended synchronised)
    return COMMS_OK;
}

comms_status_t comms_ofdmsync_correct_run_dev(comms_ofdmsync_t* h, const comms_c32* d_in, size_t n_frames, const double* cfo, comms_c32* d_out,
                                              void* stream) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG(h->n_frame != 0, "the handle was created with n_frame = 0: it has no correct stage");
    COMMS_TRY(check_frame_call(h, correct_call, d_in, n_frames, d_out, true));
    if (!n_frames) return COMMS_OK;
    COMMS_ARG(cfo != nullptr, "cfo is NULL");
    for (size_t f = 0; f < n_frames; ++f) COMMS_ARG(std::isfinite(cfo[f]), "cfo[%zu] is not finite", f);
    COMMS_TRY(use_device(h->device));
    hipStream_t s = nullptr;
    COMMS_TRY(h->enter(stream, &s));
    COMMS_TRY(h->desc_host.reserve(n_frames * sizeof(OcDesc)));
    COMMS_TRY(h->desc_dev.reserve(n_frames * sizeof(OcDesc)));
    OcDesc* hd = static_cast<OcDesc*>(h->desc_host.h);
    for (size_t f = 0; f < n_frames; ++f) {
        hd[f].cfo = cfo[f];
        hd[f].c1 = static_cast<float>(std::cos(cfo[f]));
        hd[f].s1 = static_cast<float>(-std::sin(cfo[f]));
    }
    COMMS_HIP_TRY(hipMemcpyAsync(h->desc_dev.p, hd, n_frames * sizeof(OcDesc), hipMemcpyHostToDevice, s));
    OcArgs a{};
    a.in = reinterpret_cast<const float2*>(d_in);
    a.out = reinterpret_cast<float2*>(d_out);
    a.desc = static_cast<const OcDesc*>(h->desc_dev.p);
    a.n_frame = static_cast<unsigned>(h->n_frame);
    a.runs = static_cast<unsigned>((h->n_frame + OC_RUN - 1) / OC_RUN);
    a.lanes = n_frames * a.runs;
    a.wide = h->n_frame % 2 == 0;
    const size_t blocks = (a.lanes + OC_WG - 1) / OC_WG;  // <= 2^31 / 256: max_frames of correct_call
    COMMS_TRY(launch_kernel<ofdmsync_correct_kernel>("ofdmsync_correct_kernel", dim3(static_cast<unsigned>(blocks)), dim3(OC_WG), 0, s,
                                                     h->take_events(), a));
    const hipError_t e = hipStreamSynchronize(s);  // the cfo table is rewritten by the next call
    if (e != hipSuccess) return fail(COMMS_ERR_DEVICE, "OFDM synchroniser, correct stage: %s", hipGetErrorString(e));
    return COMMS_OK;
}

comms_status_t comms_ofdmsync_correct_run(comms_ofdmsync_t* h, const comms_c32* in, size_t n_frames, const double* cfo, comms_c32* out) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG(h->n_frame != 0, "the handle was created with n_frame = 0: it has no correct stage");
    return run_frame_call(h, correct_call, in, n_frames, out, [&](void* d_in, void* d_out) {
        return comms_ofdmsync_correct_run_dev(h, static_cast<const comms_c32*>(d_in), n_frames, cfo, static_cast<comms_c32*>(d_out),
                                              COMMS_STREAM_HANDLE);
    });
}

comms_status_t comms_ofdmsync_get_state(comms_ofdmsync_t* h, comms_c32* state, size_t n_state) {
    return get_history_state(h, state, n_state, "samples");
}

// (n_state must be H = W + L + 2 G - 1 >= 2: a NULL state never comes with a length the setter accepts)
comms_status_t comms_ofdmsync_set_state(comms_ofdmsync_t* h, const comms_c32* state, size_t n_state) {
    return set_history_state(h, state, n_state, "samples");
}

comms_status_t comms_ofdmsync_get_position(const comms_ofdmsync_t* h, uint64_t* out_position) { return get_position(h, out_position); }

comms_status_t comms_ofdmsync_set_position(comms_ofdmsync_t* h, uint64_t position) {
    return set_position(h, position, [&] { h->origin = 0; });
}

comms_status_t comms_ofdmsync_set_threshold(comms_ofdmsync_t* h, double threshold) { return set_threshold(h, threshold); }

comms_status_t comms_ofdmsync_get_kernel(const comms_ofdmsync_t* h, size_t n, char* name, size_t name_len) {
    COMMS_ARG(h && name && name_len, "NULL argument");
    std::snprintf(name, name_len, "ofdmsync_detect_kernel tile=%d wg=%d lag=%d window=%d guard=%d lds=%zu tiles=%zu grid=%zu", OS_TILE, OS_WG,
                  h->L, h->W, h->G, h->y.lds, tiles_of(n), tiles_of(n));
    return COMMS_OK;
}

comms_status_t comms_ofdmsync_set_timer(comms_ofdmsync_t* h, comms_timer_t* t) { return set_handle_timer(h, t); }

comms_status_t comms_ofdmsync_destroy(comms_ofdmsync_t* h) { return destroy_handle(h); }

}  // extern "C"
