// spectrum.hip -- spectrum estimator: windowed, overlapping segments of a Complex<f32> stream -> forward transform -> |X|^2 ->
// the sum of K segments per output row (Welch), every row of a call by ONE launch (two when K > 32).
//
// The reference has no such block; the contract is include/comms_hip.h's ("spectrum estimator"), and tests/spectrum_ref.py
// restates it in float64.  A call on the stream positions [T, T + n) completes the segments s with T < s H + N <= T + n;
// the host turns T into relative numbers once (SpCall), so that the kernels never see the stream index itself: a row's bits
// cannot depend on it.
//   spectrum_kernel<N, DIRECT>  persistent, grid-stride under the library's grid cap.  A work item is one CHUNK, the <= 32
//                 consecutive segments of one row whose sum the contract fixes, and one wave takes a whole chunk: the
//                 ascending-s sum needs no ordering between waves.  Four waves per workgroup are four chunks; the waves
//                 share the tables and nothing else (no workgroup barrier behind the table load).
//     segment     lanes hold a segment as the OFDM kernels hold a symbol (ofdm_transform.hpp): 16 points per lane, L = N / 16
//                 lanes per segment, 1024 / N segments per wave at a time.  Lane l loads x[s H + l + L a], a < 16 --
//                 consecutive lanes, consecutive samples, 8 bytes each -- from the input, or from the history for positions
//                 before the call, multiplies by the window (LDS) and transforms (of_transform<N, -1>).
//     sum         N = 1024: one segment per wave at a time, a lane adds its 16 powers to 16 registers.  N < 1024: the powers
//                 of the wave's 1024 / N segments go through the wave's own exchange buffer (segment q at q (N + L): every
//                 bank once) and lane j adds bins j, j + 64, ... in segment order.
//     store       DIRECT (K <= 32, a row is one chunk, the waterfall case): scale c_0 straight to the output row, or c_0 into
//                 the accumulator state when the call ends inside the row.  Otherwise c_m to the handle's scratch
//                 [row][chunk][N] for spectrum_rows_kernel.  64 consecutive floats per store; the centred order is an index
//                 rotation (bin b to column b ^ N / 2) in the store to the output alone.
//   spectrum_rows_kernel (K > 32)  one lane per (row, bin): R from the carried R (the call's first row) or +0, plus the chunk
//                 sums in ascending m; scale R to the output for a completed row, R and the incomplete chunk's sum into the
//                 accumulator state for the last, incomplete one.
// Carries: the accumulators are a ping-pong pair like the history.  A launch reads acc[cur] (the call's first chunk and first
// row only) and writes all of acc[next]; the host flips both pairs once the launches are queued.  A replay of a launch
// computes the same values again.
// Workgroup 0 writes the new history to the other half of the ping-pong pair (History, common.hpp).
#include <cmath>
#include <vector>

#include "common.hpp"
#include "fir_handle.hpp"
#include "ofdm_transform.hpp"
#include "stream_call.hpp"

namespace comms {

constexpr int SP_WG = 256, SP_WAVES = SP_WG / 64;
constexpr int SP_CHUNK = COMMS_SPECTRUM_CHUNK;
constexpr int SP_ROWS_WG = 256;
constexpr size_t SP_MAX_HOP = size_t(1) << 20, SP_MAX_AVG = size_t(1) << 24;
constexpr size_t SP_MAX_SCRATCH = size_t(1) << 32;   // bytes of chunk sums of one call

constexpr size_t spectrum_lds(int n) { return static_cast<size_t>(n) * (sizeof(float2) + sizeof(float)) + SP_WAVES * OF_WAVE_BUF * sizeof(float2); }

// A call in relative numbers.  Segments are counted from the call's first one (q = 0 ... nseg - 1), rows from the row of
// that segment (rr = 0 ...), whose segments in front of the call number j_lo; item i is chunk (i + m_lo) mod cpr of row
// (i + m_lo) div cpr.
struct SpCall {
    size_t nseg = 0;       // segments the call completes
    long long off0 = 0;    // call offset of segment 0's first sample (> -N)
    unsigned j_lo = 0;     // (first segment) mod K
    unsigned m_lo = 0;     // j_lo / 32
    unsigned cpr = 1;      // chunks per row: ceil(K / 32)
    size_t items = 0;
    size_t rr_last = 0;    // row of the last segment
    unsigned m_last = 0;   // ... and its chunk
    bool chunk_done = false, row_done = false;   // the call's last segment ends its chunk / its row
    size_t rows = 0;       // rows completed
};

struct SpArgs {
    const float2* in;      // n samples
    const float2* hist;    // the N - 1 samples in front of them, time order
    float2* new_hist;
    const float2* tw;      // W_N^j
    const float* win;
    const float* acc;      // R[N], c[N]: read
    float* acc_next;       // ... written, all of it, by the launch that sums last
    float* out;
    float* work;           // [item][N] chunk sums (K > 32)
    size_t n, nseg, items;
    long long off0;
    unsigned H, K, cpr, j_lo, m_lo;
    int centred;
    float scale;
};

template <int N, bool DIRECT>
__global__ __launch_bounds__(SP_WG) void spectrum_kernel(const SpArgs a) {
    using G = OfGeom<N>;
    constexpr int HL = N - 1;
    constexpr int NB = N == 1024 ? 16 : N / 64;   // bins a lane sums
    constexpr int NPS = N + G::L;                 // a segment's powers in the exchange buffer
    extern __shared__ __align__(16) unsigned char sp_smem[];
    cf* tw = reinterpret_cast<cf*>(sp_smem);
    float* win = reinterpret_cast<float*>(tw + N);
    cf* ex = reinterpret_cast<cf*>(win + N);
    for (int i = threadIdx.x; i < N; i += SP_WG) {
        tw[i] = to_cf(a.tw[i]);
        win[i] = a.win[i];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane / G::L, l = lane % G::L;
    cf* wbuf = ex + wave * OF_WAVE_BUF;
    cf* buf = wbuf + q * G::NP;
    float* pbuf = reinterpret_cast<float*>(wbuf);   // SPW * NPS = 1088 floats of its 2176
    float w[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) w[i] = win[l + G::L * i];

    // `item` and everything derived from it but `live` is wave-uniform: every lane of a wave takes part in the exchanges
    for (size_t item = static_cast<size_t>(blockIdx.x) * SP_WAVES + wave; item < a.items; item += static_cast<size_t>(gridDim.x) * SP_WAVES) {
        const size_t g = item + a.m_lo, rr = g / a.cpr;
        const unsigned m = static_cast<unsigned>(g % a.cpr);
        const unsigned k_end = a.K < SP_CHUNK * (m + 1) ? a.K : SP_CHUNK * (m + 1);
        const long long base = static_cast<long long>(rr * a.K) - a.j_lo;   // segment of the row's k = 0
        long long qa = base + SP_CHUNK * m, qb = base + k_end;
        const bool complete = qb <= static_cast<long long>(a.nseg);
        qa = qa < 0 ? 0 : qa;                                               // (the call's first chunk: its head came earlier)
        qb = complete ? qb : static_cast<long long>(a.nseg);
        const bool carry = item == 0 && (a.j_lo % SP_CHUNK) != 0;

        float acc[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int b = N == 1024 ? G::bin(l, j) : lane + 64 * j;
            acc[j] = carry ? a.acc[N + b] : 0.f;
        }
        for (long long s0 = qa; s0 < qb; s0 += G::SPW) {
            const long long left = qb - s0;
            const int cnt = left < G::SPW ? static_cast<int>(left) : G::SPW;
            const bool live = q < cnt;
            cf v[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) v[i] = cf{0.f, 0.f};
            if (live) {
                const long long p0 = a.off0 + (s0 + q) * static_cast<long long>(a.H) + l;   // >= -HL, and p0 + 15 L < n
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const long long p = p0 + G::L * i;
                    const float2 x = *(p >= 0 ? a.in + p : a.hist + (HL + p));
                    v[i] = cf{__fmul_rn(w[i], x.x), __fmul_rn(w[i], x.y)};
                }
            }
            of_transform<N, -1>(v, buf, tw, l);
            if constexpr (N == 1024) {
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] = __fadd_rn(acc[i], __fmaf_rn(v[i].x, v[i].x, __fmul_rn(v[i].y, v[i].y)));
            } else {
#pragma unroll
                for (int i = 0; i < 16; ++i) pbuf[q * NPS + G::bin(l, i)] = __fmaf_rn(v[i].x, v[i].x, __fmul_rn(v[i].y, v[i].y));
                of_wave_sync();
                for (int sq = 0; sq < cnt; ++sq) {   // in segment order
#pragma unroll
                    for (int j = 0; j < NB; ++j) acc[j] = __fadd_rn(acc[j], pbuf[sq * NPS + lane + 64 * j]);
                }
                of_wave_sync();
            }
        }

        const bool last = item + 1 == a.items;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int b = N == 1024 ? G::bin(l, j) : lane + 64 * j;
            if constexpr (DIRECT) {
                if (complete) a.out[rr * N + (a.centred ? b ^ (N / 2) : b)] = __fmul_rn(a.scale, acc[j]);
                if (last) {
                    a.acc_next[b] = 0.f;
                    a.acc_next[N + b] = complete ? 0.f : acc[j];
                }
            } else {
                a.work[item * N + b] = acc[j];
            }
        }
    }

    hist_advance(a.hist, a.in, a.n, a.new_hist, HL);
}

struct SpRowsArgs {
    const float* work;
    const float* acc;
    float* acc_next;
    float* out;
    size_t items, rr_last, cells;   // cells = (rr_last + 1) * N
    unsigned N, cpr, m_lo, m_last;
    int carry_r, chunk_done, row_done, centred;
    float scale;
};

__global__ __launch_bounds__(SP_ROWS_WG) void spectrum_rows_kernel(const SpRowsArgs a) {
    for (size_t cell = static_cast<size_t>(blockIdx.x) * SP_ROWS_WG + threadIdx.x; cell < a.cells; cell += static_cast<size_t>(gridDim.x) * SP_ROWS_WG) {
        const size_t rr = cell / a.N;
        const unsigned b = static_cast<unsigned>(cell % a.N);
        const bool last_row = rr == a.rr_last;
        const size_t m0 = rr == 0 ? a.m_lo : 0;
        const size_t m1 = last_row ? a.m_last + (a.chunk_done ? 1u : 0u) : a.cpr;   // complete chunks: [m0, m1)
        float R = rr == 0 && a.carry_r ? a.acc[b] : 0.f;
        const float* c = a.work + (rr * a.cpr + m0 - a.m_lo) * a.N + b;   // chunk m is item rr cpr + m - m_lo
        size_t m = m0;
        for (; m + 16 <= m1; m += 16, c += 16 * static_cast<size_t>(a.N)) {   // sixteen loads in flight, added in order
            float t[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) t[u] = c[u * static_cast<size_t>(a.N)];
#pragma unroll
            for (int u = 0; u < 16; ++u) R = __fadd_rn(R, t[u]);
        }
        for (; m < m1; ++m, c += a.N) R = __fadd_rn(R, *c);
        if (!last_row || a.row_done) a.out[rr * a.N + (a.centred ? b ^ (a.N / 2) : b)] = __fmul_rn(a.scale, R);
        if (last_row) {
            a.acc_next[b] = a.row_done ? 0.f : R;
            a.acc_next[a.N + b] = a.chunk_done ? 0.f : a.work[(a.items - 1) * a.N + b];
        }
    }
}

}  // namespace comms

using namespace comms;

struct comms_spectrum : Handle {
    unsigned N = 0, H = 0, K = 0;
    int order = 0;
    float scale = 0.f;
    uint64_t T = 0;          // samples seen: the stream index of the next one
    size_t lds = 0;
    unsigned max_grid = 1, rows_max_grid = 1;
    DevBuf<float2> tw;
    DevBuf<float> win;
    DevBuf<float> acc[2];    // R[N], c[N]; acc[acc_idx] is current
    int acc_idx = 0;
    Scratch work;            // chunk sums of a call (K > 32)
    History hist;            // last N - 1 samples
};
static_assert(!std::is_copy_constructible_v<comms_spectrum>, "a handle is never copied");

namespace {

bool sp_size_ok(int32_t n_fft) { return n_fft == 64 || n_fft == 128 || n_fft == 256 || n_fft == 512 || n_fft == 1024; }

// S(T): segments completed before stream position T
uint64_t sp_segments(uint64_t T, uint64_t N, uint64_t H) { return T >= N ? (T - N) / H + 1 : 0; }

SpCall sp_call(const comms_spectrum* h, size_t n) {
    SpCall c;
    const uint64_t N = h->N, H = h->H, K = h->K;
    const uint64_t s_lo = sp_segments(h->T, N, H), s_hi = sp_segments(h->T + n, N, H);
    c.cpr = static_cast<unsigned>((K + SP_CHUNK - 1) / SP_CHUNK);
    c.rows = static_cast<size_t>(s_hi / K - s_lo / K);
    c.nseg = static_cast<size_t>(s_hi - s_lo);
    if (!c.nseg) return c;
    c.off0 = static_cast<long long>(s_lo * H) - static_cast<long long>(h->T);   // (s_lo H + N > T: above -N)
    c.j_lo = static_cast<unsigned>(s_lo % K);
    c.m_lo = c.j_lo / SP_CHUNK;
    const uint64_t u_last = c.j_lo + (c.nseg - 1), k_last = u_last % K;
    c.rr_last = static_cast<size_t>(u_last / K);
    c.m_last = static_cast<unsigned>(k_last / SP_CHUNK);
    c.items = c.rr_last * c.cpr + c.m_last - c.m_lo + 1;
    c.row_done = k_last + 1 == K;
    c.chunk_done = c.row_done || (k_last + 1) % SP_CHUNK == 0;
    return c;
}

size_t sp_grid(const comms_spectrum* h, const SpCall& c) { return capped_grid((c.items + SP_WAVES - 1) / SP_WAVES, h->max_grid); }
size_t sp_rows_grid(const comms_spectrum* h, const SpCall& c) {
    return capped_grid(((c.rr_last + 1) * h->N + SP_ROWS_WG - 1) / SP_ROWS_WG, h->rows_max_grid);
}

template <int N>
comms_status_t sp_launch_n(comms_spectrum* h, const SpArgs& a, dim3 grid, hipStream_t s) {
    if (h->K <= SP_CHUNK) return launch_kernel<spectrum_kernel<N, true>>("spectrum_kernel", grid, dim3(SP_WG), h->lds, s, h->take_events(), a);
    return launch_kernel<spectrum_kernel<N, false>>("spectrum_kernel", grid, dim3(SP_WG), h->lds, s, h->take_events(), a);
}

comms_status_t sp_check_call(const comms_spectrum* h, const void* in, size_t n, const void* out, bool device, SpCall* c) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG(in || !n, "%s is NULL", device ? "d_in" : "in");
    COMMS_ARG(n <= (size_t(1) << 40) && h->T + n <= (1ull << 62), "n is too long for one call, or the position would pass 2^62");
    *c = sp_call(h, n);
    COMMS_ARG(out || !c->rows, "%s is NULL", device ? "d_out" : "out");
    COMMS_ARG(h->K <= SP_CHUNK || c->items <= SP_MAX_SCRATCH / (h->N * sizeof(float)), "n is too long for one call");
    if (device) {
        COMMS_ARG(aligned(in, 8) && aligned(out, 4), "d_in must be aligned to one sample (8 bytes) and d_out to 4 bytes");
        COMMS_ARG(!n || !c->rows || !ranges_overlap(in, n * sizeof(comms_c32), out, c->rows * h->N * sizeof(float)),
                  "the input and the output rows overlap");
    }
    return COMMS_OK;
}

// The launches of a call that passed sp_check_call, n > 0, on the stream the handle follows; history, accumulators and
// position advance
comms_status_t sp_step(comms_spectrum* h, const SpCall& c, const comms_c32* d_in, size_t n, float* d_out, void* stream) {
    COMMS_TRY(use_device(h->device));
    const bool two = h->K > SP_CHUNK;
    if (two && c.items) COMMS_TRY(h->work.reserve(c.items * h->N * sizeof(float)));
    hipStream_t s = nullptr;
    COMMS_TRY(h->enter(stream, &s));
    SpArgs a{};
    a.in = reinterpret_cast<const float2*>(d_in);
    a.hist = h->hist.cur<float2>();
    a.new_hist = h->hist.next<float2>();
    a.tw = h->tw.get();
    a.win = h->win.get();
    a.acc = h->acc[h->acc_idx].get();
    a.acc_next = h->acc[h->acc_idx ^ 1].get();
    a.out = d_out;
    a.work = static_cast<float*>(h->work.p);
    a.n = n;
    a.nseg = c.nseg;
    a.items = c.items;
    a.off0 = c.off0;
    a.H = h->H;
    a.K = h->K;
    a.cpr = c.cpr;
    a.j_lo = c.j_lo;
    a.m_lo = c.m_lo;
    a.centred = h->order == COMMS_SPECTRUM_CENTRED;
    a.scale = h->scale;
    const dim3 grid(static_cast<unsigned>(sp_grid(h, c)));
    switch (h->N) {
        case 64: COMMS_TRY(sp_launch_n<64>(h, a, grid, s)); break;
        case 128: COMMS_TRY(sp_launch_n<128>(h, a, grid, s)); break;
        case 256: COMMS_TRY(sp_launch_n<256>(h, a, grid, s)); break;
        case 512: COMMS_TRY(sp_launch_n<512>(h, a, grid, s)); break;
        default: COMMS_TRY(sp_launch_n<1024>(h, a, grid, s)); break;
    }
    h->hist.flip();
    h->T += n;
    if (two && c.items) {
        SpRowsArgs r{};
        r.work = a.work;
        r.acc = a.acc;
        r.acc_next = a.acc_next;
        r.out = d_out;
        r.items = c.items;
        r.rr_last = c.rr_last;
        r.cells = (c.rr_last + 1) * h->N;
        r.N = h->N;
        r.cpr = c.cpr;
        r.m_lo = c.m_lo;
        r.m_last = c.m_last;
        r.carry_r = c.j_lo > 0;
        r.chunk_done = c.chunk_done;
        r.row_done = c.row_done;
        r.centred = a.centred;
        r.scale = h->scale;
        COMMS_TRY(launch_kernel<spectrum_rows_kernel>("spectrum_rows_kernel", dim3(static_cast<unsigned>(sp_rows_grid(h, c))), dim3(SP_ROWS_WG), 0,
                                                      s, {}, r));
    }
    if (c.items) h->acc_idx ^= 1;   // (a call that completes no segment leaves the accumulators as they are)
    return COMMS_OK;
}

}  // namespace

extern "C" {

comms_status_t comms_spectrum_state_len(int32_t n_fft, size_t* out_len) {
    COMMS_ARG(out_len != nullptr, "out_len is NULL");
    COMMS_ARG(sp_size_ok(n_fft), "n_fft must be 64, 128, 256, 512 or 1024 (got %d)", n_fft);
    *out_len = static_cast<size_t>(n_fft) - 1;
    return COMMS_OK;
}

comms_status_t comms_spectrum_create(int32_t n_fft, const float* window, size_t hop, size_t avg, float scale, int32_t order, int32_t device,
                                     comms_spectrum_t** out) {
    COMMS_ARG(out != nullptr, "out is NULL");
    *out = nullptr;
    COMMS_ARG(sp_size_ok(n_fft), "n_fft must be 64, 128, 256, 512 or 1024 (got %d)", n_fft);
    COMMS_ARG(window != nullptr, "window is NULL");
    COMMS_ARG(hop >= 1 && hop <= SP_MAX_HOP, "hop must be 1 ... 2^20 samples (got %zu)", hop);
    COMMS_ARG(avg >= 1 && avg <= SP_MAX_AVG, "avg must be 1 ... 2^24 segments (got %zu)", avg);
    COMMS_ARG(std::isfinite(scale) && scale > 0.f, "scale must be finite and positive");
    COMMS_ARG(order == COMMS_SPECTRUM_NATURAL || order == COMMS_SPECTRUM_CENTRED,
              "order must be COMMS_SPECTRUM_NATURAL or COMMS_SPECTRUM_CENTRED (got %d)", order);
    const size_t N = static_cast<size_t>(n_fft);
    for (size_t i = 0; i < N; ++i) COMMS_ARG(std::isfinite(window[i]), "window[%zu] is not finite", i);
    std::vector<float2> tw(N);
    for (size_t j = 0; j < N; ++j) {
        const double t = 2.0 * 3.14159265358979323846 * static_cast<double>(j) / static_cast<double>(N);
        tw[j] = make_float2(static_cast<float>(std::cos(t)), static_cast<float>(-std::sin(t)));
    }
    HandlePtr<comms_spectrum> h;
    COMMS_TRY(make_handle(device, &h));
    h->N = static_cast<unsigned>(n_fft);
    h->H = static_cast<unsigned>(hop);
    h->K = static_cast<unsigned>(avg);
    h->order = order;
    h->scale = scale;
    h->lds = spectrum_lds(n_fft);
    h->max_grid = persistent_cap(h->lds);
    h->rows_max_grid = persistent_cap(0);
    COMMS_HIP_TRY(h->tw.upload(tw));
    COMMS_HIP_TRY(h->win.upload(window, N));
    COMMS_HIP_TRY(h->acc[0].alloc_zero(2 * N));
    COMMS_HIP_TRY(h->acc[1].alloc_zero(2 * N));
    COMMS_HIP_TRY(h->hist.alloc(N - 1, sizeof(comms_c32)));
    *out = h.release();
    return COMMS_OK;
}

comms_status_t comms_spectrum_out_len(const comms_spectrum_t* h, size_t n, size_t* rows) {
    COMMS_ARG(h && rows, "NULL argument");
    COMMS_ARG(n <= (size_t(1) << 40) && h->T + n <= (1ull << 62), "n is too long for one call, or the position would pass 2^62");
    *rows = sp_call(h, n).rows;
    return COMMS_OK;
}

comms_status_t comms_spectrum_run_dev(comms_spectrum_t* h, const comms_c32* d_in, size_t n, float* d_out, void* stream) {
    SpCall c;
    COMMS_TRY(sp_check_call(h, d_in, n, d_out, true, &c));
    if (!n) return COMMS_OK;
    return sp_step(h, c, d_in, n, d_out, stream);
}

comms_status_t comms_spectrum_run(comms_spectrum_t* h, const comms_c32* in, size_t n, float* out) {
    SpCall c;
    COMMS_TRY(sp_check_call(h, in, n, out, false, &c));
    if (!n) return COMMS_OK;
    COMMS_TRY(use_device(h->device));
    const void* d = nullptr;
    COMMS_TRY(stage_input(h, in, n * sizeof(comms_c32), &d));
    const size_t bytes = c.rows * h->N * sizeof(float);
    COMMS_TRY(h->out_scratch.reserve(bytes ? bytes : 8));
    COMMS_TRY(sp_step(h, c, static_cast<const comms_c32*>(d), n, static_cast<float*>(h->out_scratch.p), COMMS_STREAM_HANDLE));
    if (bytes) COMMS_HIP_TRY(hipMemcpyAsync(out, h->out_scratch.p, bytes, hipMemcpyDeviceToHost, h->stream));
    COMMS_HIP_TRY(hipStreamSynchronize(h->stream));   // (also: the staged input is free again)
    return COMMS_OK;
}

comms_status_t comms_spectrum_get_state(comms_spectrum_t* h, comms_c32* state, size_t n_state) {
    return get_history_state(h, state, n_state, "samples");
}
comms_status_t comms_spectrum_set_state(comms_spectrum_t* h, const comms_c32* state, size_t n_state) {
    return set_history_state(h, state, n_state, "samples");
}

comms_status_t comms_spectrum_get_position(const comms_spectrum_t* h, uint64_t* out_position) { return get_position(h, out_position); }

comms_status_t comms_spectrum_set_position(comms_spectrum_t* h, uint64_t position) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG(position <= (1ull << 62), "position is out of range");
    COMMS_TRY(use_device(h->device));
    COMMS_TRY(h->quiesce());
    COMMS_HIP_TRY(zero_device(h->acc[h->acc_idx].get(), 2 * static_cast<size_t>(h->N) * sizeof(float)));
    h->T = position;
    return COMMS_OK;
}

comms_status_t comms_spectrum_get_acc(comms_spectrum_t* h, float* acc, size_t n_acc) {
    COMMS_TRY(state_access(h, h ? 2 * static_cast<size_t>(h->N) : 0, acc, n_acc, true, "floats"));
    COMMS_HIP_TRY(hipMemcpy(acc, h->acc[h->acc_idx].get(), n_acc * sizeof(float), hipMemcpyDeviceToHost));
    return COMMS_OK;
}
comms_status_t comms_spectrum_set_acc(comms_spectrum_t* h, const float* acc, size_t n_acc) {
    COMMS_TRY(state_access(h, h ? 2 * static_cast<size_t>(h->N) : 0, acc, n_acc, true, "floats"));
    COMMS_HIP_TRY(hipMemcpy(h->acc[h->acc_idx].get(), acc, n_acc * sizeof(float), hipMemcpyHostToDevice));
    return COMMS_OK;
}

comms_status_t comms_spectrum_get_kernel(const comms_spectrum_t* h, size_t n, char* name, size_t name_len) {
    COMMS_ARG(h && name && name_len, "NULL argument");
    COMMS_ARG(n <= (size_t(1) << 40) && h->T + n <= (1ull << 62), "n is too long for one call, or the position would pass 2^62");
    const SpCall c = sp_call(h, n);
    const bool two = h->K > SP_CHUNK;
    const int len = std::snprintf(name, name_len, "spectrum_kernel<%u,%s> wg=%d hop=%u avg=%u chunks=%u rows=%zu items=%zu grid=%zu max_grid=%u lds=%zu",
                                  h->N, two ? "chunks" : "direct", SP_WG, h->H, h->K, c.cpr, c.rows, c.items, n ? sp_grid(h, c) : size_t(0),
                                  h->max_grid, h->lds);
    if (two && c.items && len > 0 && static_cast<size_t>(len) < name_len)
        std::snprintf(name + len, name_len - static_cast<size_t>(len), " + spectrum_rows_kernel wg=%d cells=%zu grid=%zu", SP_ROWS_WG,
                      (c.rr_last + 1) * h->N, sp_rows_grid(h, c));
    return COMMS_OK;
}

comms_status_t comms_spectrum_set_timer(comms_spectrum_t* h, comms_timer_t* t) { return set_handle_timer(h, t); }

comms_status_t comms_spectrum_destroy(comms_spectrum_t* h) { return destroy_handle(h); }

}  // extern "C"
