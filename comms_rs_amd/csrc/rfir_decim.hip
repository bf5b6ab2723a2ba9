// rfir_decim.hip -- FIR + decimator over a REAL f32 stream: the audio stage of examples/fm_radio.rs in one launch.
//
//   Convert2Node (x -> Complex(x, 0)) -> BatchFirNode<f32>(real taps) -> Convert3Node (.re) -> DecimateNode<f32>(R)
//   (examples/fm_radio.rs:93-164; src/filter/fir.rs:87-102; src/util/resample_node.rs:53-65)
// With real samples and real taps the reference's complex product is (h x - 0 0, h 0 + 0 x): nothing of the detour
// survives in the values, so the node is  y[i] = sum_k h[k] x[i - k],  out = y[0], y[R], y[2R], ...  with the FIR history
// carried across calls and the decimator restarting at sample 0 of every call (any n, not only multiples of R).
//
// rfir_decim_kernel (n_taps <= 257, rate 1 ... 64) computes only the kept outputs, 4 + 4/R bytes of HBM per input sample:
//   * a workgroup owns a tile of TO = WG x OUT consecutive outputs.  Its R (TO + Qp) input samples are loaded as whole
//     rows (4 bytes per lane, buffer-addressed: the stream's end reads as zero) and staged in LDS as R PHASE ARRAYS,
//     sample s at [s mod R][s div R].  The halo in front is R Qp samples, a multiple of R, so the phase of tap k's
//     sample is (-k) mod R for EVERY output: tap k = R m - r lives in phase r at element (output + Qp - m).
//   * a lane holds OUT consecutive outputs and walks phase after phase; within a phase the taps m = 0, 1, ... meet
//     CONSECUTIVE elements, so a block of eight taps reads a window of 8 + OUT - 1 floats once and spends 8 OUT
//     multiply-adds on it (OUT = 5: 0.3 LDS reads per multiply-add).  OUT is odd or 1: the lanes of a ds_read_b32 are
//     OUT banks apart and never meet.  The eight taps of a block come from a phase-major table ([R][MP], MP = taps per
//     phase rounded up to eight, zero beyond the filter) by one scalar load: they are operands in SGPRs.
//   * the summation order of an output -- phases ascending, taps of a phase ascending, one FMA each -- depends on
//     nothing but the filter and the rate: an output has the same bits wherever a call or a tile boundary falls.
//   * outputs go through LDS once more so that the stores are whole lines; workgroup 0 advances the history.
// The staging writes scatter over the phase arrays; their stride is chosen per (rate, tile) by trying all 32 residues
// against the 32-lane write pattern (plan_stride), which is NOTES.md round 5's rule (stride = lanes per phase modulo
// the banks) without its restriction to rates that divide the group.
//
// Every other (taps, rate) runs the reference's four nodes as four launches on scratch buffers (the series), so the node
// takes any filter and any rate; comms_rfir_get_kernel tells the two apart.
//
// Non-finite input: the zero taps that pad a phase to a multiple of eight multiply real samples, so a NaN or Inf sample
// reaches a few outputs beyond its n_taps (at most 8 R - 1 samples further) -- the time-domain form of the deviation
// DESIGN.md section 2 documents for the frequency-domain kernels.
#include <algorithm>
#include <vector>

#include "common.hpp"
#include "fir_handle.hpp"
#include "stream_call.hpp"

namespace comms {

struct RfArgs {
    const float* in;        // n samples
    const float* hist;      // last hist_len samples before this call, time order
    float* new_hist;
    float* out;             // n_out kept outputs
    const float* taps;      // [R][MP]: taps[r][m] = h[R m - r] (zero outside the filter)
    size_t n, n_out;
    int hist_len, R, MP;
    int TO;                 // outputs per tile = blockDim.x * OUT
    int stride;             // floats between phase arrays (>= TO + MP - 1)
    int dp, de;             // blockDim.x mod R, blockDim.x div R: a lane's step from one staged row to its next
};

constexpr int RF_B = 8;  // taps per block

template <int OUT>
__global__ __launch_bounds__(256) void rfir_decim_kernel(const RfArgs a) {
    extern __shared__ __attribute__((aligned(16))) float rf_smem[];
    const int tid = threadIdx.x, WG = blockDim.x;
    const int R = a.R, MP = a.MP, Qp = MP - 1;
    const int L = a.TO + Qp;                  // elements per phase array
    float* xs = rf_smem;                      // [R][stride]
    float* ys = rf_smem + R * a.stride;       // [TO]
    const long long jb = static_cast<long long>(blockIdx.x) * a.TO;  // first output of the tile
    const long long g0 = (jb - Qp) * R;       // stream index of the tile's first staged sample
    const int count = R * L;

    // ---- stage: sample s of the tile -> xs[s mod R][s div R]
    int p = tid % R, e = tid / R;
    auto step = [&]() {
        p += a.dp;
        e += a.de;
        if (p >= R) {
            p -= R;
            ++e;
        }
    };
    if (g0 >= 0) {
        // rows of WG samples, eight requested before the first is written; past the stream's end (and past the tile) a
        // buffer load returns zero
        const size_t left = a.n - static_cast<size_t>(g0);
        const size_t have = left < static_cast<size_t>(count) ? left : static_cast<size_t>(count);
        const __amdgpu_buffer_rsrc_t rs = make_rsrc(a.in + g0, have * 4);
        for (int base = 0; base < count; base += 8 * WG) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                v[u] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, tid * 4, (base + u * WG) * 4, 0));
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (base + u * WG + tid < count) xs[p * a.stride + e] = v[u];
                step();
            }
        }
    } else {  // the tiles that reach back into the history (or in front of it: zeros)
        for (int s = tid; s < count; s += WG) {
            const long long g = g0 + s;
            float v = 0.f;
            if (g >= 0) {
                if (static_cast<size_t>(g) < a.n) v = a.in[g];
            } else if (g >= -static_cast<long long>(a.hist_len)) {
                v = a.hist[a.hist_len + g];
            }
            xs[p * a.stride + e] = v;
            step();
        }
    }
    __syncthreads();

    // ---- filter: phases ascending, taps of a phase ascending; tap (r, m) of output t meets xs[r][t + Qp - m]
    float acc[OUT];
#pragma unroll
    for (int o = 0; o < OUT; ++o) acc[o] = 0.f;
    const float* ph = xs + OUT * tid + (Qp - (RF_B - 1));
    for (int r = 0; r < R; ++r) {
        const float* tr = a.taps + r * MP;
        const float* pr = ph + r * a.stride;
        for (int m0 = 0; m0 < MP; m0 += RF_B) {
            float w[RF_B + OUT - 1], t[RF_B];
#pragma unroll
            for (int i = 0; i < RF_B + OUT - 1; ++i) w[i] = pr[i - m0];
#pragma unroll
            for (int q = 0; q < RF_B; ++q) t[q] = tr[m0 + q];
#pragma unroll
            for (int q = 0; q < RF_B; ++q)
#pragma unroll
                for (int o = 0; o < OUT; ++o) acc[o] = __builtin_fmaf(t[q], w[RF_B - 1 - q + o], acc[o]);
        }
    }

    // ---- store: through LDS, so that a wave writes whole lines
#pragma unroll
    for (int o = 0; o < OUT; ++o) ys[OUT * tid + o] = acc[o];
    __syncthreads();
#pragma unroll
    for (int u = 0; u < OUT; ++u) {
        const int t = tid + u * WG;
        const long long j = jb + t;
        if (j < static_cast<long long>(a.n_out)) a.out[j] = ys[t];
    }

    // ---- new_hist = last hist_len samples of concat(old_hist, in): the reference's `state` after the batch
    if (blockIdx.x == 0)
        for (int j = tid; j < a.hist_len; j += WG) {
            const size_t q = a.n + static_cast<size_t>(j);
            a.new_hist[j] = q < static_cast<size_t>(a.hist_len) ? a.hist[q] : a.in[q - a.hist_len];
        }
}

}  // namespace comms

using namespace comms;

struct comms_rfir : Handle {
    int n_eff = 0;     // taps that take part: min(n_taps, n_state)
    int rate = 1;      // >= 1 (0 is the copy, like 1)
    bool series = false;
    // rfir_decim_kernel
    int OUT = 1, WG = 256, MP = 8, stride = 0;
    size_t lds = 0;
    DevBuf<float> d_tab;
    History hist;      // last n_eff samples
    // the series: the complex FIR node carries the state; two Complex<f32> scratch streams
    InnerHandle<comms_fir_t, comms_fir_destroy> fir;
    Scratch sa, sb;
};
static_assert(!std::is_copy_constructible_v<comms_rfir>, "a handle is never copied");

namespace {

constexpr int RF_MAX_TAPS = 257, RF_MAX_RATE = 64;

// (the stride of the phase arrays: plan_stride, common.hpp)
template <int OUT>
comms_status_t launch_rfir(const RfArgs& a, unsigned blocks, int wg, size_t lds, hipStream_t s) {
    return launch_kernel<rfir_decim_kernel<OUT>>("rfir_decim_kernel", dim3(blocks), dim3(wg), lds, s, {}, a);
}

size_t rfir_out_len(size_t n, int rate) { return (n + rate - 1) / rate; }

// The reference graph node by node: cast, complex FIR (its handle keeps the history), cast, decimator
comms_status_t run_series(comms_rfir* h, const float* d_in, size_t n, float* d_out, hipStream_t s) {
    COMMS_ARG(n <= SIZE_MAX / 8, "n overflows");
    COMMS_TRY(h->sa.reserve(n * 8));
    COMMS_TRY(h->sb.reserve(n * 8));
    comms_c32* x = static_cast<comms_c32*>(h->sa.p);
    comms_c32* y = static_cast<comms_c32*>(h->sb.p);
    if (reinterpret_cast<uintptr_t>(d_in) & 7) {  // the cast reads pairs: a stream at an odd sample offset moves first
        COMMS_HIP_TRY(hipMemcpyAsync(y, d_in, n * 4, hipMemcpyDeviceToDevice, s));
        d_in = reinterpret_cast<const float*>(y);
    }
    COMMS_TRY(comms_iq_real_to_c32_dev(d_in, n, x, h->device, s));
    COMMS_TRY(comms_fir_run_dev(h->fir.get(), x, n, y, s));
    float* re = reinterpret_cast<float*>(x);
    COMMS_TRY(comms_iq_c32_re_dev(y, n, re, h->device, s));
    return comms_decimate_run_dev(re, n, 4, static_cast<size_t>(h->rate), d_out, nullptr, h->device, s);
}

}  // namespace

extern "C" {

comms_status_t comms_rfir_out_len(size_t n, size_t rate, size_t* out_len) { return comms_decimate_out_len(n, rate, out_len); }

comms_status_t comms_rfir_create(const float* taps, size_t n_taps, const float* state, size_t n_state, size_t rate,
                                 int32_t device, comms_rfir_t** out) {
    COMMS_ARG(out != nullptr, "out is NULL");
    *out = nullptr;
    COMMS_ARG(taps != nullptr && n_taps > 0, "taps must hold at least one tap (the reference panics on an empty state)");
    COMMS_ARG(state == nullptr || n_state > 0, "a user state must hold at least one sample");
    COMMS_ARG(rate <= 0x7fffffffu, "rate %zu is out of range", rate);
    size_t n_eff = n_taps;
    if (state && n_state < n_eff) n_eff = n_state;  // zip(taps, state), fir.rs:53
    COMMS_ARG(n_eff <= (1u << 20), "too many taps (%zu)", n_eff);
    HandlePtr<comms_rfir> h;
    COMMS_TRY(make_handle(device, &h));
    h->n_eff = static_cast<int>(n_eff);
    h->rate = rate < 1 ? 1 : static_cast<int>(rate);
    h->series = h->n_eff > RF_MAX_TAPS || h->rate > RF_MAX_RATE;
    if (h->series) {
        std::vector<comms_c32> ct(n_eff), cs(state ? n_eff : 0);
        for (size_t k = 0; k < n_eff; ++k) ct[k] = comms_c32{taps[k], 0.0f};
        for (size_t k = 0; k < cs.size(); ++k) cs[k] = comms_c32{state[k], 0.0f};
        comms_fir_t* fir = nullptr;
        COMMS_TRY(comms_fir_create(ct.data(), n_eff, state ? cs.data() : nullptr, cs.size(), device, &fir));
        h->fir.reset(fir);
        *out = h.release();
        return COMMS_OK;
    }
    const int R = h->rate, N = h->n_eff;
    // a lane's outputs and the workgroup's lanes: what keeps a tile's phase arrays within ~38 KiB (four workgroups per CU)
    h->OUT = R <= 6 ? 5 : R <= 12 ? 3 : 1;
    h->WG = R <= 32 ? 256 : 128;
    const int Q = (N - 1 + R - 1) / R;              // tap k = R m - r: m = 0 ... Q
    h->MP = (Q + 1 + RF_B - 1) / RF_B * RF_B;
    const int TO = h->WG * h->OUT;
    h->stride = plan_stride(R, TO + h->MP - 1);
    h->lds = (static_cast<size_t>(R) * h->stride + TO) * sizeof(float);
    std::vector<float> tab(static_cast<size_t>(R) * h->MP, 0.0f);
    for (int r = 0; r < R; ++r)
        for (int m = 0; m < h->MP; ++m) {
            const long long k = static_cast<long long>(R) * m - r;
            if (k >= 0 && k < N) tab[static_cast<size_t>(r) * h->MP + m] = taps[k];
        }
    if (h->lds > 64 * 1024) return fail(COMMS_ERR_DEVICE, "real FIR alloc: %s", hipGetErrorString(hipErrorInvalidValue));
    COMMS_HIP_TRY(h->d_tab.upload(tab));
    COMMS_HIP_TRY(h->hist.alloc(n_eff, sizeof(float)));
    if (state) COMMS_HIP_TRY(h->hist.upload(state, n_state));
    *out = h.release();
    return COMMS_OK;
}

comms_status_t comms_rfir_run_dev(comms_rfir_t* h, const float* d_in, size_t n, float* d_out, void* stream) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG((d_in && d_out) || !n, "NULL device pointer");
    COMMS_TRY(use_device(h->device));
    if (!n) return COMMS_OK;
    const size_t n_out = rfir_out_len(n, h->rate);
    COMMS_ARG(n <= SIZE_MAX / 4, "n overflows");
    COMMS_ARG(!ranges_overlap(d_in, n * 4, d_out, n_out * 4), "the real FIR cannot run in place");
    COMMS_ARG(((reinterpret_cast<uintptr_t>(d_in) | reinterpret_cast<uintptr_t>(d_out)) & 3) == 0, "pointers must be aligned to one sample");
    hipStream_t s = nullptr;
    COMMS_TRY(h->enter(stream, &s));
    if (h->series) return run_series(h, d_in, n, d_out, s);
    RfArgs a{};
    a.in = d_in;
    a.hist = h->hist.cur<float>();
    a.new_hist = h->hist.next<float>();
    a.out = d_out;
    a.taps = h->d_tab.get();
    a.n = n;
    a.n_out = n_out;
    a.hist_len = h->n_eff;
    a.R = h->rate;
    a.MP = h->MP;
    a.TO = h->WG * h->OUT;
    a.stride = h->stride;
    a.dp = h->WG % h->rate;
    a.de = h->WG / h->rate;
    const size_t tiles = (n_out + a.TO - 1) / a.TO;
    COMMS_ARG(tiles <= 0x7fffffffu, "batch too long for one launch (%zu samples)", n);
    h->tic(s);
    comms_status_t st;
    switch (h->OUT) {
        case 5: st = launch_rfir<5>(a, static_cast<unsigned>(tiles), h->WG, h->lds, s); break;
        case 3: st = launch_rfir<3>(a, static_cast<unsigned>(tiles), h->WG, h->lds, s); break;
        default: st = launch_rfir<1>(a, static_cast<unsigned>(tiles), h->WG, h->lds, s); break;
    }
    h->toc(s);
    COMMS_TRY(st);
    h->hist.flip();
    return COMMS_OK;
}

comms_status_t comms_rfir_run(comms_rfir_t* h, const float* in, size_t n, float* out) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG((in && out) || !n, "NULL host pointer");
    COMMS_TRY(use_device(h->device));
    if (!n) return COMMS_OK;
    COMMS_ARG(n <= SIZE_MAX / 4, "n overflows");
    // a unit = `rate` input samples, one output: chunks are cut where the decimator restarts anyway
    return h->run_host_units(in, n * 4, static_cast<size_t>(h->rate) * 4, out, rfir_out_len(n, h->rate) * 4, 4,
                             [&](void* d_in, void* d_out, size_t ib, size_t) {
                                 return comms_rfir_run_dev(h, static_cast<const float*>(d_in), ib / 4, static_cast<float*>(d_out), COMMS_STREAM_HANDLE);
                             });
}

comms_status_t comms_rfir_get_state(comms_rfir_t* h, float* state, size_t n_state) {
    COMMS_ARG(h && state, "NULL argument");  // this node refuses a NULL state even for an empty read
    if (!h->series) return get_history_state(h, state, n_state, "samples");
    COMMS_TRY(state_access(h, static_cast<size_t>(h->n_eff), state, n_state, false, "samples"));
    if (!n_state) return COMMS_OK;  // (an empty read: the series' inner getter takes no empty buffer)
    std::vector<comms_c32> cs(n_state);
    COMMS_TRY(comms_fir_get_state(h->fir.get(), cs.data(), n_state));
    for (size_t k = 0; k < n_state; ++k) state[k] = cs[k].re;
    return COMMS_OK;
}

// (n_state must be n_eff >= 1: a NULL state never comes with a length the setter accepts)
comms_status_t comms_rfir_set_state(comms_rfir_t* h, const float* state, size_t n_state) {
    if (!h || !h->series) return set_history_state(h, state, n_state, "samples");
    COMMS_TRY(state_access(h, static_cast<size_t>(h->n_eff), state, n_state, true, "samples"));
    std::vector<comms_c32> cs(n_state);
    for (size_t k = 0; k < n_state; ++k) cs[k] = comms_c32{state[k], 0.0f};
    return comms_fir_set_state(h->fir.get(), cs.data(), n_state);
}

comms_status_t comms_rfir_get_kernel(const comms_rfir_t* h, size_t n, char* name, size_t name_len) {
    COMMS_ARG(h && name && name_len, "NULL argument");
    if (h->series) {
        char fir[64] = {0};
        COMMS_TRY(comms_fir_get_kernel(h->fir.get(), n, fir, sizeof fir));
        std::snprintf(name, name_len, "series: real_to_c32_kernel + %s + c32_re_kernel + decimate_kernel", fir);
    } else {
        std::snprintf(name, name_len, "rfir_decim_kernel<%d>", h->OUT);
    }
    return COMMS_OK;
}

comms_status_t comms_rfir_set_timer(comms_rfir_t* h, comms_timer_t* t) {
    COMMS_TRY(set_handle_timer(h, t));
    if (h->fir.get()) return comms_fir_set_timer(h->fir.get(), t);  // the series: the pair brackets its FIR launch
    return COMMS_OK;
}

comms_status_t comms_rfir_destroy(comms_rfir_t* h) { return destroy_handle(h); }

}  // extern "C"
