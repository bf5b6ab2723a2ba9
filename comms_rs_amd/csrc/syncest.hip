// syncest.hip -- the synchronisation estimates of a Complex<f32> stream: timing and frequency from ONE read of the samples,
// and the two phase estimators on Complex<f32> symbols.
//
//   TimingEstimator::push      src/demodulation/timing_estimator.rs:85-112   -n arg( sum qout[i] dout[i] ) / (2 pi)
//   frequency_offset_estimate  src/demodulation/frequency_estimator.rs:27-42 arg( sum x[i+1] conj(x[i]) )
//   psk_phase_estimate(m)      src/demodulation/phase_estimator.rs:26-33     arg( sum x^m ) / m
//   qam_phase_estimate         src/demodulation/phase_estimator.rs:58-65     arg( sum -x^4 ) / 4
// each defined on X[i] = (double) x[i].  The f64 entries (demod.hip, estimators.hip) take 16 bytes per sample and nothing on
// the device widens a Complex<f32> stream; the receive link's stream has 24 significant bits and the timing estimate's own
// accuracy is 0.003 samples, so the timing FILTER runs in f32 here and only the products that are summed are f64.
//
// syncest_kernel (1 <= n <= 256, 2 n d + 1 <= 1024 taps), 8 bytes of HBM read per sample:
//   * the rotor exp(-i pi i / n) has period 2 n: a table of 2 n values, made on the host in f64 and rounded to f32, is
//     copied to LDS and indexed by i mod 2 n in integers -- no sincos, no rotor recurrence, the same value for sample i
//     whichever tile or lane meets it.
//   * workgroups are persistent and walk tiles of 2048 consecutive samples, tile t, t + gridDim.x, ...  A tile stages, from one
//     load per sample, the MIXED window qin = conj(x) r (f32, unfused) of its outputs and the q(t) filter's reach in front of
//     them, and the RAW samples [i0 - n d, i0 + 2048] -- the delayed samples of the final product and the frequency
//     estimator's pairs, x[i0 + 2048] included: the pair that straddles two tiles belongs to the tile of its FIRST sample and
//     to no other.  Samples in front of the stream and past its end stage as zeros (the reference's zero filter state).
//   * a lane holds eight consecutive outputs and slides a register window over the LDS image as timing_kernel does (blocks
//     of four positions rotating through three register sets, one ds_read_b64 per position feeds eight packed FMAs); the
//     taps -- f32, padded with zeros to a multiple of 12 -- are wave-uniform and come by scalar loads as SGPR operands of
//     v_pk_fma_f32 (sgpr_mac.hpp).  k ascends from an accumulator of +0, one FMA per tap.
//   * din = x r is f32 (unfused); each product qout dout, each pair product x[i+1] conj(x[i]) (its four real products are
//     exact in f64) and both sums are f64.  Lanes accumulate over their tiles, waves reduce by shuffles, one partial of four
//     doubles per workgroup goes to HBM; the fixed-order sum of the partials, atan2 and the scaling run on the host.  The
//     grid depends on the length alone, so the same input and length give the same bits on every run.
// The zero taps that pad the filter multiply real samples: a NaN or Inf sample may reach outputs up to 11 samples beyond its
// taps.
//
// phase_c32_kernel: estimators.hip's estimator_kernel (kinds 1 and 2) with the widening in the load.
#include <cmath>
#include <vector>

#include "common.hpp"
#include "sgpr_mac.hpp"
#include "stream_call.hpp"
#include "zpow.hpp"

namespace comms {

constexpr double kSePi = 3.14159265358979323846264338327950288;
constexpr int SE_WG = 256;                  // lanes per workgroup
constexpr int SE_OPL = 8;                   // consecutive outputs per lane
constexpr int SE_TILE = SE_WG * SE_OPL;     // outputs per tile
constexpr uint32_t SE_MAX_N = 256, SE_MAX_TAPS = 1024;

// LDS images: element e at e + (e >> 3) -- one pad slot per eight elements, so that lanes reading at a stride of eight
// elements (their eight consecutive outputs; 72 bytes apart) spread over all the banks
__host__ __device__ __forceinline__ int se_slot(int e) { return e + (e >> 3); }

struct SeArgs {
    const float2* x;     // len samples (8-byte aligned)
    size_t len;
    const float* taps;   // nk taps, zero beyond the filter
    const float2* rot;   // n2 rotor values, rot[m] = exp(-i pi m / n)
    int nk;              // taps staged: a multiple of 12
    int nd;              // n d: the delay
    int n2;              // 2 n: the rotor's period
    double* partials;    // [gridDim.x][4]: timing re, im, frequency re, im
};

__global__ __launch_bounds__(SE_WG) void syncest_kernel(const SeArgs a) {
    extern __shared__ __attribute__((aligned(16))) cf se_smem[];
    const int tid = threadIdx.x;
    const int nk = a.nk, nd = a.nd, n2 = a.n2;
    const int win = SE_TILE + nk - 1;                 // mixed elements 0 .. win + 1 are staged (win + 2 of them)
    cf* qs = se_smem;                                 // mixed window, padded image: se_slot(win + 1) + 1 slots
    cf* xs = qs + se_slot(win + 1) + 1;               // raw samples i0 - nd + r, r <= SE_TILE + nd + 1, padded image
    cf* rot = xs + se_slot(SE_TILE + nd + 1) + 1;     // n2 rotor values
    __shared__ double wsum[SE_WG / 64][4];
    typedef const __attribute__((address_space(4))) v2f* const_v2f_ptr;  // constant address space: scalar loads
    const const_v2f_ptr taps = (const_v2f_ptr)a.taps;

    for (int m = tid; m < n2; m += SE_WG) {
        const float2 r = a.rot[m];
        rot[m] = cf{r.x, r.y};
    }
    const size_t ntiles = (a.len + SE_TILE - 1) / SE_TILE;
    const long long len = static_cast<long long>(a.len);
    // rotor index of the first staged element of this workgroup's tile, (i0 - (nk - 1)) mod n2, stepped from tile to tile
    const long long w_first = static_cast<long long>(blockIdx.x) * SE_TILE - (nk - 1);
    int mt = static_cast<int>(((w_first % n2) + n2) % n2);
    const int mt_step = static_cast<int>((static_cast<unsigned long long>(gridDim.x) * SE_TILE) % static_cast<unsigned>(n2));
    const int m_wg = SE_WG % n2;
    double tre = 0.0, tim = 0.0, fre = 0.0, fim = 0.0;

    for (size_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long i0 = static_cast<long long>(tile) * SE_TILE;
        const long long w0 = i0 - (nk - 1);
        __syncthreads();  // the previous tile's images have been read (first tile: the rotor table is complete)
        // ---- stage: element j is sample w0 + j; four loads requested before the first is used
        int m = (mt + tid) % n2;
        for (int base = 0; base <= win + 1; base += 4 * SE_WG) {
            float2 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = base + u * SE_WG + tid;
                const long long idx = w0 + j;
                v[u] = (j <= win + 1 && idx >= 0 && idx < len) ? a.x[idx] : make_float2(0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = base + u * SE_WG + tid;
                if (j <= win + 1) {
                    const cf r = rot[m];
                    // s.conj() * r
                    qs[se_slot(j)] = cf{v[u].x * r.x + v[u].y * r.y, v[u].x * r.y - v[u].y * r.x};
                    const int rr = j - (nk - 1) + nd;  // the same sample in the raw image
                    if (rr >= 0) xs[se_slot(rr)] = cf{v[u].x, v[u].y};
                }
                m += m_wg;
                if (m >= n2) m -= n2;
            }
        }
        __syncthreads();

        // ---- q_c = sum_k t[k] qin[n_c - k],  n_c = i0 + 8 tid + c:  window element of (c, k) is e0 + c - k
        const int e0 = (nk - 1) + SE_OPL * tid;
        cf q[SE_OPL];
#pragma unroll
        for (int c = 0; c < SE_OPL; ++c) q[c] = cf{0.f, 0.f};
        // Window positions p = e0 - e grow with k: tap k of output c reads position k - c.  Positions live in register blocks
        // of four; the taps of block b (k = 4 b .. 4 b + 3) touch blocks b - 2, b - 1 and b, which rotate through three
        // register sets.  Block b holds the elements e0 - 4 b - m, m < 4: its lowest element is 0 or 4 modulo 8 in every
        // lane (nk is a multiple of 12, so e0 + 8 is 3 or 7 modulo 8), i.e. a block never straddles a pad slot.
        int eb = e0 + 5;  // lowest element of block -2
        auto load_block = [&](cf(&R)[4]) {  // called for blocks -2, -1, 0, 1, ... in this order
            const cf* p = qs + se_slot(eb);
#pragma unroll
            for (int mm = 0; mm < 4; ++mm) R[mm] = p[3 - mm];
            eb -= 4;
        };
        auto mac_block = [&](int blk, const cf(&P2)[4], const cf(&P1)[4], const cf(&Q)[4]) {
            const v2f t01 = taps[2 * blk], t23 = taps[2 * blk + 1];  // wave-uniform: scalar loads
#pragma unroll
            for (int mm = 0; mm < 4; ++mm) {
#pragma unroll
                for (int c = 0; c < SE_OPL; ++c) {
                    const int d = mm - c;
                    const cf v = d >= 0 ? Q[d] : d >= -4 ? P1[4 + d] : P2[8 + d];
                    if (mm & 1) mac_s_hi(q[c], v, mm < 2 ? t01 : t23);
                    else mac_s_lo(q[c], v, mm < 2 ? t01 : t23);
                }
            }
        };
        cf R0[4], R1[4], R2[4];
        load_block(R0);
        load_block(R1);
        const int nblk = nk / 4;  // a multiple of 3
        for (int blk = 0; blk < nblk; blk += 3) {
            load_block(R2);
            mac_block(blk, R0, R1, R2);
            load_block(R0);
            mac_block(blk + 1, R1, R2, R0);
            load_block(R1);
            mac_block(blk + 2, R2, R0, R1);
        }

        // ---- the delayed product qout[i] * (x[i - nd] r[i - nd]) and the pair x[i + 1] conj(x[i]), in f64
        int md = (mt + SE_OPL * tid + (nk - 1) - nd) % n2;  // rotor index of sample i - nd (nk - 1 >= 2 nd)
#pragma unroll
        for (int c = 0; c < SE_OPL; ++c) {
            const long long i = i0 + SE_OPL * tid + c;
            if (i < len && i >= nd) {
                const cf s = xs[se_slot(SE_OPL * tid + c)], r = rot[md];
                const float dre = s.x * r.x - s.y * r.y, dim = s.x * r.y + s.y * r.x;  // s * r
                const double qr = q[c].x, qi = q[c].y, dr = dre, di = dim;
                tre += qr * dr - qi * di;
                tim += qr * di + qi * dr;
            }
            if (++md == n2) md = 0;
            if (i + 1 < len) {
                const cf x1 = xs[se_slot(nd + SE_OPL * tid + c + 1)], x0 = xs[se_slot(nd + SE_OPL * tid + c)];
                const double ar = x1.x, ai = x1.y, br = x0.x, bi = -static_cast<double>(x0.y);  // conj
                fre += ar * br - ai * bi;
                fim += ar * bi + ai * br;
            }
        }
        mt += mt_step;
        if (mt >= n2) mt -= n2;
    }

    // wave reduction by shuffles, then one LDS hop across the 4 waves
    double acc[4] = {tre, tim, fre, fim};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc[k] += __shfl_down(acc[k], off);
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) wsum[tid >> 6][k] = acc[k];
    }
    __syncthreads();
    if (tid < 4) {
        double s = wsum[0][tid];
        for (int w = 1; w < SE_WG / 64; ++w) s += wsum[w][tid];
        a.partials[static_cast<size_t>(blockIdx.x) * 4 + tid] = s;
    }
}

// KIND 1: x^m;  2: -x^4  (estimator_kernel's terms, grid-stride loop and reduction; the symbol is widened in the load)
template <int KIND>
__global__ __launch_bounds__(256) void phase_c32_kernel(const float2* __restrict__ x, size_t n, unsigned m,
                                                        double2* __restrict__ partials) {
    const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    auto term = [&](size_t i) {
        const float2 s = x[i];
        const double2 p = zpowi(make_double2(static_cast<double>(s.x), static_cast<double>(s.y)), KIND == 1 ? m : 4u);
        return KIND == 1 ? p : make_double2(-1.0 * p.x, -1.0 * p.y);
    };
    double2 a4[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) a4[u] = make_double2(0.0, 0.0);
    size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    for (; i + 3 * stride < n; i += 4 * stride) {
        double2 p[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) p[u] = term(i + u * stride);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            a4[u].x += p[u].x;
            a4[u].y += p[u].y;
        }
    }
    for (; i < n; i += stride) {
        const double2 p = term(i);
        a4[0].x += p.x;
        a4[0].y += p.y;
    }
    double2 acc = make_double2((a4[0].x + a4[1].x) + (a4[2].x + a4[3].x), (a4[0].y + a4[1].y) + (a4[2].y + a4[3].y));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        acc.x += __shfl_down(acc.x, off);
        acc.y += __shfl_down(acc.y, off);
    }
    __shared__ double2 wsum[4];
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double2 s = wsum[0];
        for (int w = 1; w < 4; ++w) {
            s.x += wsum[w].x;
            s.y += wsum[w].y;
        }
        partials[blockIdx.x] = s;
    }
}

constexpr size_t kPhaseMaxBlocks = 8u * kNumCU;

static comms_status_t phase_c32(int kind, const comms_c32* d_x, size_t n, unsigned m, double* out, int32_t device, void* stream) {
    COMMS_ARG(out != nullptr && (d_x || !n), "NULL argument");
    COMMS_ARG((reinterpret_cast<uintptr_t>(d_x) & 7) == 0, "symbols must be aligned to one sample");
    COMMS_TRY(use_device(device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    size_t blocks = (n + 255) / 256;
    if (blocks > kPhaseMaxBlocks) blocks = kPhaseMaxBlocks;
    if (blocks < 1) blocks = 1;
    // per-thread, per-device partials buffer, allocated once, as estimators.hip's: every call ends with a stream sync
    static thread_local double2* tl_part[64] = {};
    COMMS_ARG(device >= 0 && device < 64, "device index out of range");
    if (!tl_part[device]) COMMS_HIP_TRY(hipMalloc(&tl_part[device], kPhaseMaxBlocks * sizeof(double2)));
    double2* d_part = tl_part[device];
    const float2* x = reinterpret_cast<const float2*>(d_x);
    if (kind == 1)
        phase_c32_kernel<1><<<dim3(static_cast<unsigned>(blocks)), dim3(256), 0, s>>>(x, n, m, d_part);
    else
        phase_c32_kernel<2><<<dim3(static_cast<unsigned>(blocks)), dim3(256), 0, s>>>(x, n, m, d_part);
    COMMS_TRY(launch_ok("phase_c32_kernel"));
    std::vector<double2> part(blocks);
    hipError_t e = hipMemcpyAsync(part.data(), d_part, blocks * sizeof(double2), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(COMMS_ERR_DEVICE, "phase estimator copy-back: %s", hipGetErrorString(e));
    double re = 0.0, im = 0.0;
    for (size_t b = 0; b < blocks; ++b) {
        re += part[b].x;
        im += part[b].y;
    }
    *out = std::atan2(im, re) / (kind == 1 ? static_cast<double>(m) : 4.0);  // Complex::arg
    return COMMS_OK;
}

static comms_status_t phase_c32_host(int kind, const comms_c32* x, size_t n, unsigned m, double* out, int32_t device) {
    COMMS_ARG(out != nullptr && (x || !n), "NULL argument");
    COMMS_ARG(n <= SIZE_MAX / 8, "n overflows");
    COMMS_TRY(use_device(device));
    Handle* h = nullptr;
    COMMS_TRY(thread_handle(device, &h));
    const void* d = nullptr;
    if (n) COMMS_TRY(stage_input(h, x, n * 8, &d));
    return phase_c32(kind, static_cast<const comms_c32*>(d), n, m, out, device, h->stream);
}

}  // namespace comms

using namespace comms;

struct comms_syncest : Handle {
    uint32_t n = 0, d = 0;
    int nk = 0;                   // taps staged (2 n d + 1 padded to a multiple of 12)
    size_t lds = 0;
    unsigned max_grid = 1;
    DevBuf<float> d_taps;   // nk
    DevBuf<float2> d_rot;   // 2 n
    DevBuf<double> d_part;  // [max_grid][4]
};
static_assert(!std::is_copy_constructible_v<comms_syncest>, "a handle is never copied");

namespace {

size_t syncest_tiles(size_t len) { return (len + SE_TILE - 1) / SE_TILE; }
size_t syncest_grid(const comms_syncest* h, size_t len) { return tile_grid(syncest_tiles(len), h->max_grid); }

}  // namespace

extern "C" {

comms_status_t comms_syncest_create(uint32_t n, uint32_t d, double alpha, int32_t device, comms_syncest_t** out) {
    COMMS_ARG(out != nullptr, "out is NULL");
    *out = nullptr;
    COMMS_ARG(n >= 1 && n <= SE_MAX_N, "samples per symbol must be 1 ... %u (got %u)", SE_MAX_N, n);
    COMMS_ARG(d >= 1, "the filter delay d must be >= 1 symbol");
    COMMS_ARG(2ull * n * d + 1 <= SE_MAX_TAPS, "at most %u taps (2 n d + 1 = %llu)", SE_MAX_TAPS, 2ull * n * d + 1);
    const uint32_t n_q = 2 * n * d + 1;  // odd: qfilt_taps returns exactly n_q
    std::vector<double> t64(n_q);
    COMMS_TRY(comms_qfilt_taps(n_q, alpha, n, t64.data()));  // alpha outside [0, 1]: COMMS_ERR_ARG
    HandlePtr<comms_syncest> h;
    COMMS_TRY(make_handle(device, &h));
    h->n = n;
    h->d = d;
    h->nk = static_cast<int>((n_q + 11) / 12 * 12);  // the kernel walks the taps in blocks of 12; zero taps add nothing
    const int nd = static_cast<int>(n * d), win = SE_TILE + h->nk - 1;
    h->lds = (static_cast<size_t>(se_slot(win + 1) + 1) + static_cast<size_t>(se_slot(SE_TILE + nd + 1) + 1) + 2 * n) * sizeof(float2);
    h->max_grid = resident_workgroups(h->lds);
    std::vector<float> taps(h->nk, 0.0f);
    for (uint32_t k = 0; k < n_q; ++k) taps[k] = static_cast<float>(t64[k]);
    std::vector<float2> rot(2 * n);
    for (uint32_t m = 0; m < 2 * n; ++m) {
        // Complex::new(0.0, -PI * i as f64 / n as f64).exp(), rounded to f32
        const double th = (-kSePi * static_cast<double>(m)) / static_cast<double>(n);
        rot[m] = make_float2(static_cast<float>(std::cos(th)), static_cast<float>(std::sin(th)));
    }
    COMMS_HIP_TRY(h->d_taps.upload(taps));
    COMMS_HIP_TRY(h->d_rot.upload(rot));
    COMMS_HIP_TRY(h->d_part.alloc(static_cast<size_t>(h->max_grid) * 4));
    *out = h.release();
    return COMMS_OK;
}

comms_status_t comms_syncest_run_dev(comms_syncest_t* h, const comms_c32* d_in, size_t len, comms_sync_estimate_t* out, void* stream) {
    COMMS_ARG(h != nullptr && out != nullptr, "NULL argument");
    COMMS_ARG(d_in || !len, "NULL device pointer");
    COMMS_ARG((reinterpret_cast<uintptr_t>(d_in) & 7) == 0, "input must be aligned to one sample");
    COMMS_ARG(len <= SIZE_MAX / 8, "len overflows");
    COMMS_TRY(use_device(h->device));
    double sum[4] = {0.0, 0.0, 0.0, 0.0};
    if (len) {
        hipStream_t s = nullptr;
        COMMS_TRY(h->enter(stream, &s));  // the partials buffer is the handle's: one stream at a time
        const size_t grid = syncest_grid(h, len);
        SeArgs a{};
        a.x = reinterpret_cast<const float2*>(d_in);
        a.len = len;
        a.taps = h->d_taps.get();
        a.rot = h->d_rot.get();
        a.nk = h->nk;
        a.nd = static_cast<int>(h->n * h->d);
        a.n2 = static_cast<int>(2 * h->n);
        a.partials = h->d_part.get();
        h->tic(s);
        syncest_kernel<<<dim3(static_cast<unsigned>(grid)), dim3(SE_WG), h->lds, s>>>(a);
        h->toc(s);
        COMMS_TRY(launch_ok("syncest_kernel"));
        std::vector<double> part(grid * 4);
        hipError_t e = hipMemcpyAsync(part.data(), h->d_part.get(), part.size() * sizeof(double), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return fail(COMMS_ERR_DEVICE, "sync estimator copy-back: %s", hipGetErrorString(e));
        for (size_t b = 0; b < grid; ++b)
            for (int k = 0; k < 4; ++k) sum[k] += part[4 * b + k];
    }
    out->timing_sum[0] = sum[0];
    out->timing_sum[1] = sum[1];
    out->freq_sum[0] = sum[2];
    out->freq_sum[1] = sum[3];
    // -(self.n as f64) * sum_value.arg() / (2.0 * PI)
    out->timing = (-static_cast<double>(h->n) * std::atan2(sum[1], sum[0])) / (2.0 * kSePi);
    out->freq = std::atan2(sum[3], sum[2]);
    return COMMS_OK;
}

comms_status_t comms_syncest_run(comms_syncest_t* h, const comms_c32* in, size_t len, comms_sync_estimate_t* out) {
    COMMS_ARG(h != nullptr && out != nullptr, "NULL argument");
    COMMS_ARG(in || !len, "NULL host pointer");
    COMMS_ARG(len <= SIZE_MAX / 8, "len overflows");
    COMMS_TRY(use_device(h->device));
    const void* d = nullptr;
    if (len) COMMS_TRY(stage_input(h, in, len * 8, &d));
    return comms_syncest_run_dev(h, static_cast<const comms_c32*>(d), len, out, COMMS_STREAM_HANDLE);
}

comms_status_t comms_syncest_get_kernel(const comms_syncest_t* h, size_t len, char* name, size_t name_len) {
    COMMS_ARG(h && name && name_len, "NULL argument");
    std::snprintf(name, name_len, "syncest_kernel tile=%d wg=%d taps=%d lds=%zu tiles=%zu grid=%zu max_grid=%u", SE_TILE, SE_WG,
                  h->nk, h->lds, syncest_tiles(len), syncest_grid(h, len), h->max_grid);
    return COMMS_OK;
}

comms_status_t comms_syncest_set_timer(comms_syncest_t* h, comms_timer_t* t) { return set_handle_timer(h, t); }

comms_status_t comms_syncest_destroy(comms_syncest_t* h) { return destroy_handle(h); }

comms_status_t comms_psk_phase_estimate_c32_dev(const comms_c32* d_symbols, size_t n, uint32_t m, double* out, int32_t device,
                                                void* stream) {
    COMMS_ARG(m >= 1 && m <= (1u << 20), "PSK order m out of range");
    return phase_c32(1, d_symbols, n, m, out, device, stream);
}
comms_status_t comms_qam_phase_estimate_c32_dev(const comms_c32* d_symbols, size_t n, double* out, int32_t device, void* stream) {
    return phase_c32(2, d_symbols, n, 4, out, device, stream);
}
comms_status_t comms_psk_phase_estimate_c32(const comms_c32* symbols, size_t n, uint32_t m, double* out, int32_t device) {
    COMMS_ARG(m >= 1 && m <= (1u << 20), "PSK order m out of range");
    return phase_c32_host(1, symbols, n, m, out, device);
}
comms_status_t comms_qam_phase_estimate_c32(const comms_c32* symbols, size_t n, double* out, int32_t device) {
    return phase_c32_host(2, symbols, n, 4, out, device);
}

}  // extern "C"
