// resample.hip -- rational resampler: upsample by L, FIR, decimate by M over an f32 or Complex<f32> stream in one launch.
//
//   UpsampleNode(L) -> BatchFirNode(Complex(taps, 0)) -> DecimateNode(M)
//   (src/util/resample_node.rs:53-65,120-131; src/filter/fir.rs:87-102; for f32 samples with the casts of
//   examples/fm_radio.rs:93-141 either side of the filter)
// The series spends all N multiply-adds on every one of the n L upsampled samples, although all but 1/L of the products
// are with stuffed zeros, and then drops all but 1/M of the results.  Only the products that survive are computed here:
//   out[j] = sum_{q >= 0} h[p + L q] x[i - q],   p = (j M) mod L,  i = (j M) div L      (j M in 64 bits)
// with x[-1], x[-2], ... the last input samples of earlier calls: the node's state is Q = (N - 1) div L INPUT samples.
// The decimator restarts at sample 0 of every call (any n), the history advances by all n samples.
//
// resample_kernel (L <= 256, M <= 256, M <= 64 L, tap table of at most 24 KiB), E + E L / M bytes of HBM per input sample:
//   * the taps are stored phase-major, tab[p][q] = h[p + L q], rows RS floats apart: RS = taps per phase rounded up to
//     four, plus four where that makes RS / 4 odd -- a lane reads four taps of ITS row by one ds_read_b128, and rows whose
//     numbers differ by less than 16 then start in different 16-byte bank groups.  Neighbouring lanes are on different
//     phases (the phase advances by M mod L per output), so a tap cannot be a scalar operand as in rfir_decim_kernel.
//   * workgroups are persistent: each copies the table into LDS once and then walks tiles of TO consecutive outputs,
//     tile t, t + gridDim.x, ...  A tile stages the (TO M) / L + 4 NB input samples its outputs reach with whole-row
//     buffer loads (the stream's end reads as zero); the tiles at the front read the handle's history buffer.
//   * lane t of a pass holds output jb + t: consecutive lanes hold consecutive outputs, so the stores are whole lines as
//     they are and need no second trip through LDS.  Phase and sample index of a lane's outputs advance by additions
//     with a carry; the only divisions are two per lane and one per workgroup at the start of the launch.
//   * the summation order of an output -- q ascending from an accumulator of +0, one FMA each, the zero taps that pad a
//     row included -- depends on nothing but the taps, L and the output's phase: an output has the same bits wherever a
//     call or a tile boundary falls.
//   * workgroup 0 writes the new history to the other half of a ping-pong pair.
// A table that leaves no room for a tile of samples beside it in LDS (few phases with thousands of taps each) stays in
// global memory and is read through the vector cache (TAB_LDS = false).
//
// Every other (L, M, N) runs the reference's nodes as launches in series on scratch buffers; comms_resample_get_kernel
// tells the two apart.
//
// Taps are real and applied as Complex(h, 0): the complex product's cross terms h * im - 0 * re are not formed, so signed
// zeros and non-finite samples may differ from the literal product.  The zero taps that pad a phase multiply real
// samples: a NaN or Inf sample may reach outputs up to 4 L - 1 upsampled samples beyond its N taps.
#include <algorithm>
#include <numeric>
#include <vector>

#include "common.hpp"
#include "fir_handle.hpp"
#include "stream_call.hpp"

namespace comms {

struct RsArgs {
    const void* in;         // n samples
    const void* hist;       // last Q samples before this call, time order
    void* new_hist;
    void* out;              // n_out outputs
    const float* taps;      // [L][RS]: taps[p][q] = h[p + L q] (zero beyond the filter)
    size_t n, n_out, tiles;
    int Q, L, M, RS, NB;    // NB: blocks of four taps per phase
    int TO;                 // outputs per tile
    int S;                  // samples staged per tile: (L - 1 + (TO - 1) M) / L + 4 NB
    unsigned step_i, step_p;  // (gridDim.x TO M) div L, mod L: from one tile of a workgroup to its next
    unsigned wg_i, wg_p;      // (blockDim.x M) div L, mod L: from one output of a lane to its next
};

template <class T>
struct RsElem;
template <>
struct RsElem<float> {
    static __device__ __forceinline__ float zero() { return 0.f; }
    static __device__ __forceinline__ float load(__amdgpu_buffer_rsrc_t rs, unsigned lane, unsigned row) {
        return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, lane, row, 0));
    }
    static __device__ __forceinline__ void mac(float& acc, float w, float x) { acc = __builtin_fmaf(w, x, acc); }
};
template <>
struct RsElem<float2> {
    static __device__ __forceinline__ float2 zero() { return make_float2(0.f, 0.f); }
    static __device__ __forceinline__ float2 load(__amdgpu_buffer_rsrc_t rs, unsigned lane, unsigned row) {
        return BufRows<const float2*>::get_from(rs, lane, row);
    }
    static __device__ __forceinline__ void mac(float2& acc, float w, float2 x) {
        acc.x = __builtin_fmaf(w, x.x, acc.x);
        acc.y = __builtin_fmaf(w, x.y, acc.y);
    }
};

template <class T, bool TAB_LDS>
__global__ __launch_bounds__(256) void resample_kernel(const RsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float rs_smem[];
    using EL = RsElem<T>;
    constexpr unsigned E = sizeof(T);
    const int tid = threadIdx.x, WG = blockDim.x;
    const int L = a.L, RS = a.RS, NB = a.NB;
    const int tab_floats = TAB_LDS ? L * RS : 0;  // a multiple of four
    T* xs = reinterpret_cast<T*>(rs_smem + tab_floats);
    const T* in = static_cast<const T*>(a.in);
    const T* hist = static_cast<const T*>(a.hist);
    T* out = static_cast<T*>(a.out);
    const float* tab = a.taps;
    if (TAB_LDS) {
        const float4* src = reinterpret_cast<const float4*>(a.taps);
        float4* dst = reinterpret_cast<float4*>(rs_smem);
        for (int i = tid; i < tab_floats / 4; i += WG) dst[i] = src[i];
        tab = rs_smem;
    }

    // output jb + t of a tile that starts at phase pb: phase (pb + t M) mod L, sample (pb + t M) div L beyond the tile's
    unsigned lane_p = static_cast<unsigned>(tid) * a.M % L, lane_i = static_cast<unsigned>(tid) * a.M / L;
    const unsigned long long first = static_cast<unsigned long long>(blockIdx.x) * a.TO * a.M;
    unsigned long long ib = first / L;                      // input sample of the tile's first output
    unsigned pb = static_cast<unsigned>(first % L);         // ... and its phase
    const int back = 4 * NB - 1;                            // samples staged in front of it

    for (size_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const long long g0 = static_cast<long long>(ib) - back;  // stream index of the tile's first staged sample
        __syncthreads();  // the table is in place; the previous tile's samples have been read
        if (g0 >= 0) {
            // rows of WG samples, four requested before the first is written; past the stream's end a buffer load returns zero
            const size_t left = a.n - static_cast<size_t>(g0);
            const size_t have = left < static_cast<size_t>(a.S) ? left : static_cast<size_t>(a.S);
            const __amdgpu_buffer_rsrc_t rs = make_rsrc(in + g0, have * E);
            for (int base = 0; base < a.S; base += 4 * WG) {
                T v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = EL::load(rs, tid * E, (base + u * WG) * E);
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (base + u * WG + tid < a.S) xs[base + u * WG + tid] = v[u];
            }
        } else {  // the tiles that reach back into the history (or in front of it: zeros)
            for (int s = tid; s < a.S; s += WG) {
                const long long g = g0 + s;
                T v = EL::zero();
                if (g >= 0) {
                    if (static_cast<size_t>(g) < a.n) v = in[g];
                } else if (g >= -static_cast<long long>(a.Q)) {
                    v = hist[a.Q + g];
                }
                xs[s] = v;
            }
        }
        __syncthreads();

        // ---- filter: q ascending; tap q of a lane's output meets the staged sample (its index) - q
        const size_t jb = tile * static_cast<size_t>(a.TO);
        unsigned p = pb + lane_p, di = lane_i;
        if (p >= static_cast<unsigned>(L)) {
            p -= L;
            ++di;
        }
        for (int t = tid; t < a.TO; t += WG) {
            const float* tr = tab + p * RS;
            const T* xp = xs + di + back;
            T acc = EL::zero();
#pragma unroll 2
            for (int b = 0; b < NB; ++b) {
                const float4 w = *reinterpret_cast<const float4*>(tr + 4 * b);
                const T x0 = xp[-4 * b], x1 = xp[-4 * b - 1], x2 = xp[-4 * b - 2], x3 = xp[-4 * b - 3];
                EL::mac(acc, w.x, x0);
                EL::mac(acc, w.y, x1);
                EL::mac(acc, w.z, x2);
                EL::mac(acc, w.w, x3);
            }
            const size_t j = jb + t;
            if (j < a.n_out) out[j] = acc;
            p += a.wg_p;
            di += a.wg_i;
            if (p >= static_cast<unsigned>(L)) {
                p -= L;
                ++di;
            }
        }

        ib += a.step_i;
        pb += a.step_p;
        if (pb >= static_cast<unsigned>(L)) {
            pb -= L;
            ++ib;
        }
    }

    // ---- new_hist = last Q samples of concat(old_hist, in)
    if (blockIdx.x == 0) {
        T* nh = static_cast<T*>(a.new_hist);
        for (int j = tid; j < a.Q; j += WG) {
            const size_t q = a.n + static_cast<size_t>(j);
            nh[j] = q < static_cast<size_t>(a.Q) ? hist[q] : in[q - a.Q];
        }
    }
}

}  // namespace comms

using namespace comms;

struct comms_resample : Handle {
    int elem = COMMS_RESAMPLE_F32;  // bytes per sample: 4 (f32) or 8 (Complex<f32>)
    size_t n_taps = 0;
    size_t up = 1, down = 1;        // >= 1 (0 is the copy, like 1)
    size_t Q = 0;                   // state: (n_taps - 1) / up input samples
    size_t unit = 1;                // down / gcd(up, down) input samples = up / gcd outputs
    bool series = false;
    // resample_kernel
    int RS = 4, NB = 1, TO = 0, S = 0, WG = 256;
    bool tab_lds = true;
    size_t lds = 0;
    unsigned max_grid = 1;
    DevBuf<float> d_tab;
    History hist;                   // last Q samples
    // the series: the complex FIR node carries the state (of the UPSAMPLED stream); two scratch streams of n up samples
    InnerHandle<comms_fir_t, comms_fir_destroy> fir;
    Scratch sa, sb;
};
static_assert(!std::is_copy_constructible_v<comms_resample>, "a handle is never copied");

namespace {

constexpr size_t RS_MAX_UP = 256, RS_MAX_DOWN = 256, RS_MAX_RATIO = 64, RS_MAX_TABLE = 24 * 1024;
constexpr size_t RS_LDS_MAX = 64 * 1024;    // what the project's kernels request per workgroup
constexpr size_t RS_LDS_FOUR = 40 * 1024;   // four workgroups per CU: four waves per SIMD keep the LDS reads in flight

size_t rs_samples(size_t TO, size_t L, size_t M, size_t NB) { return (L - 1 + (TO - 1) * M) / L + 4 * NB; }

// Tile size: the largest of 1024 ... 16 outputs whose samples fit beside the table -- within 40 KiB if a tile of at least
// 256 does, otherwise within the 64 KiB limit; and if even 16 do not fit there, with the table left in global memory.
bool plan_tile(comms_resample* h, size_t tab_bytes) {
    const size_t L = h->up, M = h->down, NB = h->NB, E = h->elem;
    for (size_t limit : {RS_LDS_FOUR, RS_LDS_MAX})
        for (size_t TO = 1024; TO >= (limit == RS_LDS_FOUR ? 256u : 16u); TO /= 2) {
            const size_t S = rs_samples(TO, L, M, NB), lds = tab_bytes + S * E;
            if (lds > limit) continue;
            h->TO = static_cast<int>(TO);
            h->S = static_cast<int>(S);
            h->lds = lds;
            return true;
        }
    return false;
}

template <class T, bool TAB_LDS>
comms_status_t launch_resample(const RsArgs& a, unsigned blocks, int wg, size_t lds, hipStream_t s) {
    return launch_kernel<resample_kernel<T, TAB_LDS>>("resample_kernel", dim3(blocks), dim3(wg), lds, s, {}, a);
}

size_t resample_out_len(size_t n, size_t up, size_t down) {  // n * up does not overflow (checked by the callers)
    const size_t nu = n * up;
    return nu / down + (nu % down ? 1 : 0);
}

// tiles of a call that writes n_out samples, and the grid that walks them
size_t resample_tiles(const comms_resample* h, size_t n_out) { return (n_out + h->TO - 1) / h->TO; }
size_t resample_grid(const comms_resample* h, size_t n_out) { return tile_grid(resample_tiles(h, n_out), h->max_grid); }

// The reference's nodes one by one: upsampler, [cast,] complex FIR (its handle keeps the history), [cast,] decimator
comms_status_t run_series(comms_resample* h, const void* d_in, size_t n, void* d_out, hipStream_t s) {
    const size_t nu = n * h->up;
    COMMS_ARG(nu <= SIZE_MAX / 8, "n * up overflows");
    COMMS_TRY(h->sa.reserve(nu * 8));
    COMMS_TRY(h->sb.reserve(nu * 8));
    comms_c32* xa = static_cast<comms_c32*>(h->sa.p);
    comms_c32* xb = static_cast<comms_c32*>(h->sb.p);
    if (h->elem == COMMS_RESAMPLE_C32) {
        COMMS_TRY(comms_upsample_run_dev(d_in, n, 8, h->up, xa, nullptr, h->device, s));
        COMMS_TRY(comms_fir_run_dev(h->fir.get(), xa, nu, xb, s));
        return comms_decimate_run_dev(xb, nu, 8, h->down, d_out, nullptr, h->device, s);
    }
    float* fa = reinterpret_cast<float*>(xa);
    float* fb = reinterpret_cast<float*>(xb);
    COMMS_TRY(comms_upsample_run_dev(d_in, n, 4, h->up, fb, nullptr, h->device, s));
    COMMS_TRY(comms_iq_real_to_c32_dev(fb, nu, xa, h->device, s));
    COMMS_TRY(comms_fir_run_dev(h->fir.get(), xa, nu, xb, s));
    COMMS_TRY(comms_iq_c32_re_dev(xb, nu, fa, h->device, s));
    return comms_decimate_run_dev(fa, nu, 4, h->down, d_out, nullptr, h->device, s);
}

}  // namespace

extern "C" {

comms_status_t comms_resample_out_len(size_t n, size_t up, size_t down, size_t* out_len) {
    COMMS_ARG(out_len != nullptr, "out_len is NULL");
    if (up < 1) up = 1;
    if (down < 1) down = 1;
    COMMS_ARG(n <= SIZE_MAX / up, "n * up overflows");
    *out_len = resample_out_len(n, up, down);
    return COMMS_OK;
}

comms_status_t comms_resample_state_len(size_t n_taps, size_t up, size_t* out_len) {
    COMMS_ARG(out_len != nullptr, "out_len is NULL");
    COMMS_ARG(n_taps > 0, "taps must hold at least one tap");
    *out_len = (n_taps - 1) / (up < 1 ? 1 : up);
    return COMMS_OK;
}

comms_status_t comms_resample_create(const float* taps, size_t n_taps, size_t up, size_t down, int32_t elem, int32_t device,
                                     comms_resample_t** out) {
    COMMS_ARG(out != nullptr, "out is NULL");
    *out = nullptr;
    COMMS_ARG(taps != nullptr && n_taps > 0, "taps must hold at least one tap (the reference panics on an empty state)");
    COMMS_ARG(elem == COMMS_RESAMPLE_F32 || elem == COMMS_RESAMPLE_C32, "elem must be COMMS_RESAMPLE_F32 (4) or COMMS_RESAMPLE_C32 (8), got %d", elem);
    COMMS_ARG(up <= 0x7fffffffu && down <= 0x7fffffffu, "rates %zu / %zu are out of range", up, down);
    COMMS_ARG(n_taps <= (1u << 20), "too many taps (%zu)", n_taps);
    HandlePtr<comms_resample> h;
    COMMS_TRY(make_handle(device, &h));
    h->elem = elem;
    h->n_taps = n_taps;
    h->up = up < 1 ? 1 : up;
    h->down = down < 1 ? 1 : down;
    h->Q = (n_taps - 1) / h->up;
    h->unit = h->down / std::gcd(h->up, h->down);
    const size_t L = h->up, M = h->down, QP = h->Q + 1;
    h->series = L > RS_MAX_UP || M > RS_MAX_DOWN || M > RS_MAX_RATIO * L || L * QP * 4 > RS_MAX_TABLE;
    if (h->series) {
        std::vector<comms_c32> ct(n_taps);
        for (size_t k = 0; k < n_taps; ++k) ct[k] = comms_c32{taps[k], 0.0f};
        comms_fir_t* fir = nullptr;
        COMMS_TRY(comms_fir_create(ct.data(), n_taps, nullptr, 0, device, &fir));
        h->fir.reset(fir);
        *out = h.release();
        return COMMS_OK;
    }
    h->NB = static_cast<int>((QP + 3) / 4);
    h->RS = 4 * (h->NB | 1);  // RS / 4 odd
    const size_t tab_floats = L * h->RS;
    h->tab_lds = plan_tile(h.get(), tab_floats * 4);
    if (!h->tab_lds && !plan_tile(h.get(), 0))
        return fail(COMMS_ERR_DEVICE, "resample: no tile fits (up %zu, down %zu, %zu taps)", L, M, n_taps);
    h->WG = tile_workgroup(h->TO);
    h->max_grid = resident_workgroups(h->lds);
    COMMS_HIP_TRY(h->d_tab.upload(polyphase_rows(taps, n_taps, L, static_cast<size_t>(h->RS))));
    COMMS_HIP_TRY(h->hist.alloc(h->Q, static_cast<size_t>(elem)));
    *out = h.release();
    return COMMS_OK;
}

comms_status_t comms_resample_run_dev(comms_resample_t* h, const void* d_in, size_t n, void* d_out, void* stream) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG((d_in && d_out) || !n, "NULL device pointer");
    COMMS_TRY(use_device(h->device));
    if (!n) return COMMS_OK;
    const size_t E = static_cast<size_t>(h->elem);
    COMMS_ARG(n <= SIZE_MAX / 8 / h->up, "n * up overflows");
    const size_t n_out = resample_out_len(n, h->up, h->down);
    COMMS_ARG(n_out <= SIZE_MAX / 8, "the output's byte count overflows");
    COMMS_ARG(!ranges_overlap(d_in, n * E, d_out, n_out * E), "the resampler cannot run in place");
    COMMS_ARG(((reinterpret_cast<uintptr_t>(d_in) | reinterpret_cast<uintptr_t>(d_out)) & (E - 1)) == 0, "pointers must be aligned to one sample");
    hipStream_t s = nullptr;
    COMMS_TRY(h->enter(stream, &s));
    if (h->series) return run_series(h, d_in, n, d_out, s);
    const unsigned grid = static_cast<unsigned>(resample_grid(h, n_out));
    RsArgs a{};
    a.in = d_in;
    a.hist = h->hist.cur();
    a.new_hist = h->hist.next();
    a.out = d_out;
    a.taps = h->d_tab.get();
    a.n = n;
    a.n_out = n_out;
    a.tiles = resample_tiles(h, n_out);
    a.Q = static_cast<int>(h->Q);
    a.L = static_cast<int>(h->up);
    a.M = static_cast<int>(h->down);
    a.RS = h->RS;
    a.NB = h->NB;
    a.TO = h->TO;
    a.S = h->S;
    const unsigned long long step = static_cast<unsigned long long>(grid) * h->TO * h->down;
    a.step_i = static_cast<unsigned>(step / h->up);
    a.step_p = static_cast<unsigned>(step % h->up);
    const unsigned wstep = static_cast<unsigned>(h->WG) * static_cast<unsigned>(h->down);
    a.wg_i = wstep / static_cast<unsigned>(h->up);
    a.wg_p = wstep % static_cast<unsigned>(h->up);
    h->tic(s);
    comms_status_t st;
    if (h->elem == COMMS_RESAMPLE_F32)
        st = h->tab_lds ? launch_resample<float, true>(a, grid, h->WG, h->lds, s) : launch_resample<float, false>(a, grid, h->WG, h->lds, s);
    else
        st = h->tab_lds ? launch_resample<float2, true>(a, grid, h->WG, h->lds, s) : launch_resample<float2, false>(a, grid, h->WG, h->lds, s);
    h->toc(s);
    COMMS_TRY(st);
    h->hist.flip();
    return COMMS_OK;
}

comms_status_t comms_resample_run(comms_resample_t* h, const void* in, size_t n, void* out) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG((in && out) || !n, "NULL host pointer");
    COMMS_TRY(use_device(h->device));
    if (!n) return COMMS_OK;
    const size_t E = static_cast<size_t>(h->elem);
    COMMS_ARG(n <= SIZE_MAX / 8 / h->up, "n * up overflows");
    const size_t n_out = resample_out_len(n, h->up, h->down);
    COMMS_ARG(n_out <= SIZE_MAX / 8, "the output's byte count overflows");
    // a unit = down / gcd input samples = up / gcd outputs: chunks are cut where the decimator's restart is phase-neutral
    const size_t unit_out = h->unit * h->up / h->down;
    return h->run_host_units(in, n * E, h->unit * E, out, n_out * E, unit_out * E, [&](void* d_in, void* d_out, size_t ib, size_t) {
        return comms_resample_run_dev(h, d_in, ib / E, d_out, COMMS_STREAM_HANDLE);
    });
}

comms_status_t comms_resample_get_state(comms_resample_t* h, void* state, size_t n_state) {
    if (!h || !h->series) return get_history_state(h, state, n_state, "samples");
    COMMS_TRY(state_access(h, h->Q, state, n_state, false, "samples"));
    if (!n_state) return COMMS_OK;
    const size_t E = static_cast<size_t>(h->elem);
    {
        // the inner state is that of the upsampled stream, newest first: entry up - 1 + up q holds input sample n - 1 - q
        const size_t m = h->up * n_state;
        std::vector<comms_c32> cs(m);
        COMMS_TRY(comms_fir_get_state(h->fir.get(), cs.data(), m));
        for (size_t q = 0; q < n_state; ++q) {
            const comms_c32 v = cs[h->up - 1 + h->up * q];
            if (E == 8) static_cast<comms_c32*>(state)[q] = v;
            else static_cast<float*>(state)[q] = v.re;
        }
        return COMMS_OK;
    }
}

comms_status_t comms_resample_set_state(comms_resample_t* h, const void* state, size_t n_state) {
    if (!h || !h->series) return set_history_state(h, state, n_state, "samples");
    COMMS_TRY(state_access(h, h->Q, state, n_state, true, "samples"));
    const size_t E = static_cast<size_t>(h->elem);
    std::vector<comms_c32> cs(h->n_taps, comms_c32{0.0f, 0.0f});  // the stuffed zeros between the input samples
    for (size_t q = 0; q < n_state; ++q)
        cs[h->up - 1 + h->up * q] = E == 8 ? static_cast<const comms_c32*>(state)[q] : comms_c32{static_cast<const float*>(state)[q], 0.0f};
    return comms_fir_set_state(h->fir.get(), cs.data(), cs.size());
}

comms_status_t comms_resample_get_kernel(const comms_resample_t* h, size_t n, char* name, size_t name_len) {
    COMMS_ARG(h && name && name_len, "NULL argument");
    if (h->series) {
        char fir[64] = {0};
        COMMS_TRY(comms_fir_get_kernel(h->fir.get(), n * h->up, fir, sizeof fir));
        if (h->elem == COMMS_RESAMPLE_C32)
            std::snprintf(name, name_len, "series: upsample_kernel + %s + decimate_kernel", fir);
        else
            std::snprintf(name, name_len, "series: upsample_kernel + real_to_c32_kernel + %s + c32_re_kernel + decimate_kernel", fir);
    } else {
        const size_t n_out = resample_out_len(n, h->up, h->down);
        std::snprintf(name, name_len, "resample_kernel<%s, %s> tile=%d lds=%zu tiles=%zu grid=%zu max_grid=%u",
                      h->elem == COMMS_RESAMPLE_C32 ? "c32" : "f32", h->tab_lds ? "taps in LDS" : "taps in global memory", h->TO, h->lds,
                      resample_tiles(h, n_out), resample_grid(h, n_out), h->max_grid);
    }
    return COMMS_OK;
}

comms_status_t comms_resample_set_timer(comms_resample_t* h, comms_timer_t* t) {
    COMMS_TRY(set_handle_timer(h, t));
    if (h->fir.get()) return comms_fir_set_timer(h->fir.get(), t);  // the series: the pair brackets its FIR launch
    return COMMS_OK;
}

comms_status_t comms_resample_destroy(comms_resample_t* h) { return destroy_handle(h); }

}  // extern "C"
