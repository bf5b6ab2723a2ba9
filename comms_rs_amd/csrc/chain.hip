// chain.hip -- mixer / FIR / decimate-by-R [/ FM demod] as ONE node.
//
// An ADDITIONAL node (the reference has no fused nodes): same results as the
// reference nodes in series -- MixerNode -> BatchFirNode -> DecimateNode
// [-> FMDemodNode] (BASELINE config 3; examples/fm_radio.rs:146-148 order with a
// mixer in front) or BatchFirNode -> MixerNode -> DecimateNode (the BASELINE
// metric's chain).  plan_chain picks one kind per chain when it is created:
//   Series      mixer, FIR, decimator [, FM demod]: four launches through HBM temporaries
//   SeriesPost  FIR, then mixer + decimator in one pass over the kept samples [, FM demod]
//   Os1024      fir_os1024_kernel<.., MODE> (fir.hip): 1024-point overlap-save, the extra stages fused in registers
//   Decim       fir_decim_kernel (fir_decim.hip): time domain, computes only the kept outputs
//   DecimAny    fir_decim_any_kernel (fir_decim_any.hip): the same at any rate
//   Poly8       fir_poly8_kernel (fir_poly8.hip): polyphase branches in the frequency domain
//   Os4096Dec   fir_os4096_kernel (fir.hip), mixer and decimator in its store stage
//   Os16kDec    fir_os16k_kernel (fir.hip), the same
// Decim and DecimAny hand a call to fir_poly8_kernel where it is the faster form for that batch.
#include <cmath>
#include <vector>

#include "common.hpp"
#include "fir_handle.hpp"

using namespace comms;

// four-kernel path with the mixer in front: the FIR node's own history holds MIXED samples, so the
// chain keeps the last N RAW input samples beside it (what comms_chain_{get,set}_fir_state speak)
__global__ __launch_bounds__(256) void chain_raw_hist_kernel(const float2* __restrict__ old_hist,
                                                             const float2* __restrict__ in, size_t n,
                                                             float2* __restrict__ new_hist, int HL) {
    hist_advance(old_hist, in, n, new_hist, HL);
}

enum class ChainKind : uint8_t { Series, SeriesPost, Os1024, Decim, DecimAny, Poly8, Os4096Dec, Os16kDec };  // (the map above)

// one fused launch (+ the demodulator's own, if fm_separate)
static bool is_fused(ChainKind k) { return k != ChainKind::Series && k != ChainKind::SeriesPost; }
// the kernel converts raw i16 / u8 IQ in its load stage; the other kinds get one conversion pass first
static bool reads_wire_format(ChainKind k) {
    return k == ChainKind::Decim || k == ChainKind::DecimAny || k == ChainKind::Poly8 || k == ChainKind::Os4096Dec;
}
// the mixer runs in front of the FIR node, whose history then holds mixed samples: the raw ones are kept beside it
static bool has_raw_history(ChainKind k) { return k == ChainKind::Series; }
// the kernel takes the FM demodulator's state (fm_prev) as arguments
static bool has_fm_prev(ChainKind k) {
    return k == ChainKind::Os1024 || k == ChainKind::Decim || k == ChainKind::DecimAny || k == ChainKind::Poly8;
}

struct ChainPlan {
    ChainKind kind = ChainKind::Series;
    bool fm_separate = false;     // the FM demodulator runs as its own launch (behind the fused one, or last of the series)
    bool taps_modulated = false;  // the mixer in front is folded into the taps
    int32_t mode = 0;             // COMMS_CHAIN_* bits of the fused launch
};

struct comms_chain : Handle {
    ChainKind kind = ChainKind::Series;
    bool fm_separate = false;  // (ChainPlan)
    int32_t mode = 0;
    bool time_domain = false;  // COMMS_CHAIN_TIME_DOMAIN: Decim / DecimAny never hand a call to the polyphase kernel
    bool ran_poly8 = false;    // Decim / DecimAny: the last call ran fir_poly8_kernel (comms_chain_is_fused)
    size_t rate = 1;
    bool fm_demod = false;
    InnerHandle<comms_fir_t, comms_fir_destroy> fir;
    // fused kinds: oscillator phase and FM demod state
    uint64_t turns = 0, frac = 0;
    History fm_prev;  // has_fm_prev: FM.prev, one sample
    // series kinds
    InnerHandle<comms_mixer_t, comms_mixer_destroy> mixer;
    InnerHandle<comms_fmdemod_t, comms_fmdemod_destroy> fm;  // (and fm_separate)
    double dphase = 0.0;  // wrapped, as the mixer steps it
    Scratch t1, t2, t3;
    History raw_hist;                          // has_raw_history: last n_eff raw inputs
    std::vector<comms_c32> pending_raw;        // a user state not yet mixed into the FIR node's history
    int in_fmt = COMMS_IQ_C32;                 // wire format of d_in (comms_chain_set_input_format)
    float in_scale = 1.0f;
    Scratch t0;                                // converted input, for the kinds that read Complex<f32> only
    int out_bits = 0;                          // COMMS_SYM_BITS output: bits per symbol (0: Complex<f32> / FM angles)
    SymTable out_sym{};                        // ... and the decision table (comms_chain_set_output_format)
};
static_assert(!std::is_copy_constructible_v<comms_chain>, "a handle is never copied");

// bytes of a call's output of n_dec decimated samples
static size_t chain_out_bytes(const comms_chain* h, size_t n_dec) {
    if (h->out_bits) return (n_dec * static_cast<size_t>(h->out_bits) + 7) / 8;
    return n_dec * (h->fm_demod ? sizeof(float) : sizeof(comms_c32));
}

// four-kernel path with the mixer in front: the FIR node keeps MIXED samples, so a raw user history is
// mixed with the phases the oscillator had at samples -1, -2, ... (Mixer::mix arithmetic: f64 product
// rounded once, src/mixer.rs:77-78).  Done at the next run, so that set_fir_state and set_phase may
// come in either order.
static comms_status_t chain_flush_raw_state(comms_chain* h) {
    if (h->pending_raw.empty()) return COMMS_OK;
    double ph = 0.0;
    COMMS_TRY(comms_mixer_get_phase(h->mixer.get(), &ph));
    const size_t n_state = h->pending_raw.size();
    std::vector<comms_c32> mixed(n_state);
    for (size_t k = 0; k < n_state; ++k) {
        const double a = ph - static_cast<double>(k + 1) * h->dphase;
        const double c = std::cos(a), s = std::sin(a);
        const double re = h->pending_raw[k].re, im = h->pending_raw[k].im;
        mixed[k].re = static_cast<float>(re * c - im * s);
        mixed[k].im = static_cast<float>(re * s + im * c);
    }
    h->pending_raw.clear();
    return comms_fir_set_state(h->fir.get(), mixed.data(), n_state);
}

// Which kind runs this chain, decided once from the filter (the user's taps), the rate and the COMMS_CHAIN_* flags.
// Rules in order of precedence: forced and long polyphase, any-rate, the fused and time-domain forms, the long
// overlap-save decimating forms, the series.
static ChainPlan plan_chain(const comms_fir* fir, size_t rate, int32_t flags) {
    const bool fm = (flags & COMMS_CHAIN_FM_DEMOD) != 0;
    const bool after = (flags & COMMS_CHAIN_MIXER_AFTER_FIR) != 0;
    const size_t n_taps = static_cast<size_t>(fir->n_eff);
    const uint32_t r32 = static_cast<uint32_t>(rate);
    ChainPlan p;
    const int32_t poly_mode = (after ? COMMS_CHAIN_POST : COMMS_CHAIN_PRE) | COMMS_CHAIN_DEC | (fm ? COMMS_CHAIN_FM : 0);
    const bool force_poly8 = (flags & COMMS_CHAIN_POLYPHASE) && !(flags & COMMS_CHAIN_UNFUSED) &&
                             comms_fir_poly8_supported(fir, r32, poly_mode, static_cast<size_t>(1) << 26) != 0;
    // Filters too long for the other fusions (258 ... 513 taps; until round 5 these chains ran as overlap-save FIR + mixer-decimator
    // [+ demodulator]: 80 us at 2^24 samples and rate 8): the polyphase kernel with five to eight halo rows, where it takes every
    // call of the filter (asked with the shortest batch); the demodulator in the kernel where it has one (rates 8 and 4, 505
    // taps), as its own launch over the kept samples otherwise.
    bool poly_long = false, poly_long_fm = false;
    if (n_taps > 257 && !force_poly8 && !(flags & (COMMS_CHAIN_UNFUSED | COMMS_CHAIN_TIME_DOMAIN | COMMS_CHAIN_FREQ_DOMAIN))) {
        poly_long_fm = fm && comms_fir_poly8_supported(fir, r32, poly_mode, rate) == 2;
        poly_long = poly_long_fm || comms_fir_poly8_supported(fir, r32, poly_mode & ~COMMS_CHAIN_FM, rate) == 2;
    }
    if (force_poly8 || poly_long) {
        p.kind = ChainKind::Poly8;
        p.fm_separate = poly_long && fm && !poly_long_fm;
        p.mode = p.fm_separate ? (poly_mode & ~COMMS_CHAIN_FM) : poly_mode;
        return p;
    }
    const bool can_fuse_nofm = !(flags & COMMS_CHAIN_UNFUSED) && n_taps <= 257 && rate <= (1u << 20);
    // FM chains on the overlap-save path: mixer / FIR / decimate as the one fused launch, the demodulator as its
    // own kernel over the n / rate decimated samples.  That beats demodulating inside the overlap-save kernel at
    // every rate (2^24 samples, 127 taps: /2 85.8 against 95.9 us, /3 68 against 83, /8 60 against 82 -- the fused
    // form needs `rate` more halo samples per segment and an atan2 per output in a kernel short of issue slots) and
    // has no limit on taps + rate.
    const bool can_fuse = can_fuse_nofm && !fm;
    const bool can_hybrid = can_fuse_nofm && fm;
    // the time-domain kernel against what would run otherwise: an overlap-save fusion, or the four kernels in
    // series, which it beats up to many more MACs per input sample
    const int decim_ok = rate <= 16 ? comms_fir_decim_supported_for(fir, r32, fm ? 1 : 0, can_fuse || can_hybrid ? 1 : 0) : 0;
    // (rate 4 with a long filter: too many MACs for the time-domain kernel, but its chain kind is the one that reaches the polyphase
    // frequency-domain kernel, which takes every call from 64 taps -- fir_poly8.hip)
    const bool poly_pref = decim_ok >= 1 && !(flags & COMMS_CHAIN_TIME_DOMAIN) &&
                           comms_fir_poly8_supported(fir, r32, COMMS_CHAIN_DEC | (fm ? COMMS_CHAIN_FM : 0), static_cast<size_t>(1) << 26) == 2;
    // FM chains where that kernel runs without its demodulator (rates 12 ... 64; rate 4 beyond 249 taps): mixer / FIR / decimate on
    // it and the demodulator as its own small launch over the n / rate kept samples, where the kernel takes EVERY call of this
    // filter (asked with the shortest batch) -- rate 4, 255 taps, 2^24 samples: ~50 us against 70 for the overlap-save launch +
    // demodulator (up to 249 taps the demodulator runs in the kernel: poly_pref above)
    const bool poly_sep = fm && rate != 8 && !poly_pref && !(flags & (COMMS_CHAIN_TIME_DOMAIN | COMMS_CHAIN_FREQ_DOMAIN | COMMS_CHAIN_UNFUSED)) &&
                          comms_fir_poly8_supported(fir, r32, COMMS_CHAIN_DEC, rate) == 2;
    const bool can_decim = !(flags & (COMMS_CHAIN_UNFUSED | COMMS_CHAIN_FREQ_DOMAIN)) &&
                           (decim_ok == 2 || poly_pref || (poly_sep && decim_ok >= 1) || (decim_ok == 1 && (flags & COMMS_CHAIN_TIME_DOMAIN)));
    // Rates the per-rate kernel is not built for (17 and up; 11 / 13 / 15 with complex taps): the any-rate kernel (half
    // a wave per output).  Against the overlap-save launch it replaces (58-61 us at 2^24 samples whatever the rate): 255
    // taps 60 us at rate 17, 53 at 20, 39 at 32, 30 at 100, 11 at 1000; 127 taps 49 at 17; 63 taps 45 at 17
    // (profiles/r03_bench_chain_rates.txt) -- so from rate 17; taps up to 512, where the alternative is four kernels in
    // series.  COMMS_CHAIN_TIME_DOMAIN forces it wherever it can run.
    static const int any_min_rate = diag_knob("COMMS_ANY_MIN_RATE", 17);
    const size_t any_from = static_cast<size_t>(any_min_rate);
    const bool can_any = !can_decim && !(flags & (COMMS_CHAIN_UNFUSED | COMMS_CHAIN_FREQ_DOMAIN)) &&
                         comms_fir_decim_any_supported(fir, r32) && ((flags & COMMS_CHAIN_TIME_DOMAIN) || rate >= any_from);
    if (can_any) {
        // mixer in front: sum_k h[k] x[n-k] e^{i phi(n-k)} = e^{i phi(n)} sum_k (h[k] e^{-i k dphi}) x[n-k] -- the kernel
        // filters the RAW samples with modulated (complex) taps and mixes the kept outputs (the roundings fall
        // elsewhere than in the reference's order, inside the parity tolerance: test_chain_any_rate)
        p.kind = ChainKind::DecimAny;
        p.taps_modulated = !after;
        p.fm_separate = poly_sep;
        p.mode = COMMS_CHAIN_POST | COMMS_CHAIN_DEC | (fm && !poly_sep ? COMMS_CHAIN_FM : 0);
        return p;
    }
    if (can_fuse || can_decim || can_hybrid) {
        p.kind = can_decim ? ChainKind::Decim : ChainKind::Os1024;
        p.fm_separate = (!can_decim && !can_fuse) || (can_decim && poly_sep);
        p.mode = (after ? COMMS_CHAIN_POST : COMMS_CHAIN_PRE) | COMMS_CHAIN_DEC | (fm && !p.fm_separate ? COMMS_CHAIN_FM : 0);
        return p;
    }
    // 258 ... 1537 taps at the rates the polyphase kernel does not run: the 4096-point overlap-save kernel keeps, mixes and stores
    // every rate-th output itself (one launch instead of FIR + mixer-decimator; 383 taps at rate 5, 2^24 samples: 96 -> ~60 us);
    // FM demod follows as its own launch over the kept samples
    const uint32_t rate32 = static_cast<uint32_t>(rate < (1u << 21) ? rate : 0);
    const bool os_ok = !(flags & (COMMS_CHAIN_UNFUSED | COMMS_CHAIN_TIME_DOMAIN));
    const bool os_dec16 = os_ok && comms_fir_os16k_decim_supported(fir, rate32) != 0;  // (1538 ... 4097 taps: the 16384-point kernel)
    const bool os_dec = os_dec16 || (os_ok && comms_fir_os4096_decim_supported(fir, rate32) != 0);
    // Mixer in front of a long filter: sum_k h[k] x[n-k] e^{i phi_(n-k)} = e^{i phi_n} sum_k (h[k] e^{-i k dphi}) x[n-k],
    // so the chain runs as FIR (modulated taps, raw samples) -> mixer + decimator in one pass over the kept
    // samples, instead of a full-rate mixer pass in front of the FIR (511 taps / 16 at 2^24: 135 -> 95 us).  The
    // roundings fall elsewhere than in the reference's order (inside the parity tolerance); COMMS_CHAIN_UNFUSED
    // keeps the literal four nodes.
    p.taps_modulated = !after && !(flags & COMMS_CHAIN_UNFUSED);
    p.fm_separate = fm;
    if (os_dec) {
        p.kind = os_dec16 ? ChainKind::Os16kDec : ChainKind::Os4096Dec;
        p.mode = COMMS_CHAIN_POST | COMMS_CHAIN_DEC;
    } else {
        p.kind = after || p.taps_modulated ? ChainKind::SeriesPost : ChainKind::Series;
    }
    return p;
}

// h[k] e^{-i k dphase}: the taps with the mixer in front folded in (plan_chain)
static std::vector<comms_c32> modulated_taps(const comms_c32* taps, size_t n_taps, double dphase) {
    std::vector<comms_c32> mod(n_taps);
    for (size_t k = 0; k < n_taps; ++k) {
        const double ang = -dphase * static_cast<double>(k);
        const double cr = std::cos(ang), ci = std::sin(ang);
        const double tr = taps[k].re, ti = taps[k].im;
        mod[k].re = static_cast<float>(tr * cr - ti * ci);
        mod[k].im = static_cast<float>(tr * ci + ti * cr);
    }
    return mod;
}

extern "C" {

comms_status_t comms_chain_create_ex(double dphase, double phase, const comms_c32* taps, size_t n_taps,
                                     size_t rate, int32_t flags, int32_t device, comms_chain_t** out) {
    COMMS_ARG(out != nullptr, "out is NULL");
    *out = nullptr;
    COMMS_ARG(rate >= 1, "rate must be >= 1");
    COMMS_ARG(std::isfinite(dphase) && std::isfinite(phase), "dphase/phase must be finite");
    HandlePtr<comms_chain> h;
    COMMS_TRY(make_handle(device, &h));
    h->rate = rate;
    h->dphase = mix_wrap_dphase(dphase);
    h->fm_demod = (flags & COMMS_CHAIN_FM_DEMOD) != 0;
    h->time_domain = (flags & COMMS_CHAIN_TIME_DOMAIN) != 0;
    comms_fir_t* fir = nullptr;
    COMMS_TRY(comms_fir_create(taps, n_taps, nullptr, 0, device, &fir));
    h->fir.reset(fir);
    const ChainPlan p = plan_chain(fir, rate, flags);
    h->kind = p.kind;
    h->fm_separate = p.fm_separate;
    h->mode = p.mode;
    if (p.taps_modulated) {
        const std::vector<comms_c32> mod = modulated_taps(taps, n_taps, h->dphase);
        h->fir.reset();
        COMMS_TRY(comms_fir_create(mod.data(), n_taps, nullptr, 0, device, &fir));
        h->fir.reset(fir);
    }
    if (is_fused(p.kind)) {
        h->frac = mix_to_turns(h->dphase);
        h->turns = mix_to_turns(phase);
    } else {
        comms_mixer_t* mixer = nullptr;
        COMMS_TRY(comms_mixer_create(dphase, phase, device, &mixer));
        h->mixer.reset(mixer);
    }
    if (p.fm_separate) {
        comms_fmdemod_t* fm = nullptr;
        COMMS_TRY(comms_fmdemod_create(device, &fm));
        h->fm.reset(fm);
    }
    if (has_fm_prev(p.kind)) COMMS_HIP_TRY(h->fm_prev.alloc(1, sizeof(float2)));
    if (has_raw_history(p.kind)) COMMS_HIP_TRY(h->raw_hist.alloc(static_cast<size_t>(h->fir->n_eff), sizeof(float2)));
    *out = h.release();
    return COMMS_OK;
}

comms_status_t comms_chain_create(double dphase, double phase, const comms_c32* taps,
                                  size_t n_taps, size_t rate, int32_t fm_demod, int32_t device,
                                  comms_chain_t** out) {
    return comms_chain_create_ex(dphase, phase, taps, n_taps, rate, fm_demod ? COMMS_CHAIN_FM_DEMOD : 0, device, out);
}

comms_status_t comms_chain_is_fused(const comms_chain_t* h, int32_t* out_fused) {
    COMMS_ARG(h && out_fused, "NULL argument");
    switch (h->kind) {
        case ChainKind::Series:
        case ChainKind::SeriesPost: *out_fused = 0; break;
        case ChainKind::Decim: *out_fused = h->ran_poly8 ? 4 : 2; break;
        case ChainKind::DecimAny: *out_fused = h->ran_poly8 ? 4 : 3; break;
        case ChainKind::Poly8: *out_fused = 4; break;
        default: *out_fused = 1; break;  // the overlap-save kernels
    }
    return COMMS_OK;
}

comms_status_t comms_chain_run_dev(comms_chain_t* h, const comms_c32* d_in_any, size_t n,
                                   void* d_out, void* stream) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG((d_in_any && d_out) || !n, "NULL device pointer");
    const comms_c32* d_in = d_in_any;  // n samples in the chain's input format
    COMMS_ARG(n % h->rate == 0, "n (%zu) must be a multiple of the decimation rate %zu", n, h->rate);
    COMMS_TRY(use_device(h->device));
    if (!n) return COMMS_OK;
    const size_t in_elem = in_elem_bytes(h->in_fmt);
    COMMS_ARG(!ranges_overlap(d_in, n * in_elem, d_out, chain_out_bytes(h, n / h->rate)), "the chain cannot run in place");
    COMMS_ARG(!h->out_bits || (reinterpret_cast<uintptr_t>(d_out) & 3) == 0, "bits output (COMMS_SYM_BITS) must be 4-byte aligned");
    COMMS_ARG((reinterpret_cast<uintptr_t>(d_in) & (in_elem - 1)) == 0, "input must be aligned to one IQ sample");
    hipStream_t hs = nullptr;
    COMMS_TRY(h->enter(stream, &hs));  // the stages' state (history, prev) advances in stream order
    void* s = static_cast<void*>(hs);
    if (h->in_fmt != COMMS_IQ_C32 && !reads_wire_format(h->kind)) {
        // the kernels of the other kinds read Complex<f32>: one conversion pass first (same arithmetic, iqformat.hip)
        COMMS_TRY(h->t0.reserve(n * sizeof(comms_c32)));
        comms_c32* c = static_cast<comms_c32*>(h->t0.p);
        if (h->in_fmt == COMMS_IQ_I16)
            COMMS_TRY(comms_iq_i16_to_c32_dev(reinterpret_cast<const int16_t*>(d_in), n, h->in_scale, c, h->device, s));
        else
            COMMS_TRY(comms_iq_u8_to_c32_dev(reinterpret_cast<const uint8_t*>(d_in), n, c, h->device, s));
        d_in = c;
    }
    const size_t n_dec = n / h->rate;
    const uint32_t rate = static_cast<uint32_t>(h->rate);
    if (is_fused(h->kind)) {
        void* stage_out = d_out;
        // decimated filter output to scratch: the demodulator reads it, or (bits output of a kernel without the fused
        // decision stage) the decision pass
        const bool via_t3 = h->fm_separate || h->out_bits;
        if (via_t3) {
            COMMS_TRY(h->t3.reserve(n_dec * sizeof(comms_c32)));
            stage_out = h->t3.p;
        }
        bool decided = false;  // the launch wrote the bits itself
        float2* prev = h->fm_prev.cur<float2>();
        float2* prev_new = h->fm_prev.next<float2>();
        switch (h->kind) {
            case ChainKind::Os4096Dec:
                COMMS_TRY(comms_fir_run_os4096_decim_dev(h->fir.get(), d_in, n, stage_out, h->turns, h->frac, rate, s));
                break;
            case ChainKind::Os16kDec:
                COMMS_TRY(comms_fir_run_os16k_decim_dev(h->fir.get(), d_in, n, stage_out, h->turns, h->frac, rate, s));
                break;
            case ChainKind::Decim:
            case ChainKind::DecimAny:
                // long filters on long batches: the polyphase frequency-domain kernel, where it is the faster form (fir_poly8.hip)
                if (h->time_domain || comms_fir_poly8_supported(h->fir.get(), rate, h->mode, n) != 2) {
                    h->ran_poly8 = false;
                    if (h->kind == ChainKind::Decim && h->out_bits) {  // the decision in fir_decim_kernel's store stage
                        COMMS_TRY(comms_fir_run_decim_bits_dev(h->fir.get(), d_in, n, d_out, h->mode, h->turns, h->frac, rate, &h->out_sym, stage_out, s));
                        decided = true;
                    } else if (h->kind == ChainKind::Decim)
                        COMMS_TRY(comms_fir_run_decim_dev(h->fir.get(), d_in, n, stage_out, h->mode, h->turns, h->frac, rate, prev, prev_new, s));
                    else
                        COMMS_TRY(comms_fir_run_decim_any_dev(h->fir.get(), d_in, n, stage_out, h->mode, h->turns, h->frac, rate, prev, prev_new, s));
                    break;
                }
                [[fallthrough]];
            case ChainKind::Poly8:
                COMMS_TRY(comms_fir_run_poly8_dev(h->fir.get(), d_in, n, stage_out, h->mode, h->turns, h->frac, rate, prev, prev_new, s));
                h->ran_poly8 = true;
                break;
            default:
                COMMS_TRY(comms_fir_run_fused_dev(h->fir.get(), d_in, n, stage_out, h->mode, h->turns, h->frac, rate, prev, prev_new, s));
                break;
        }
        h->turns += static_cast<uint64_t>(n) * h->frac;
        if (h->out_bits && !decided)
            return sym_to_bits_launch(static_cast<const comms_c32*>(stage_out), n_dec, h->out_sym, static_cast<uint8_t*>(d_out), hs);
        if (h->fm_separate)
            return comms_fmdemod_run_dev(h->fm.get(), static_cast<const comms_c32*>(stage_out), n_dec, static_cast<float*>(d_out), s);
        if (h->fm_demod) h->fm_prev.flip();
        return COMMS_OK;
    }
    COMMS_TRY(h->t1.reserve(n * sizeof(comms_c32)));
    comms_c32* a = static_cast<comms_c32*>(h->t1.p);
    comms_c32* dec = static_cast<comms_c32*>(d_out);  // the decimated samples: the output, or the demodulator's / decision's input
    if (h->fm_demod || h->out_bits) {
        COMMS_TRY(h->t3.reserve(n_dec * sizeof(comms_c32)));
        dec = static_cast<comms_c32*>(h->t3.p);
    }
    if (h->kind == ChainKind::SeriesPost) {  // FIR, then mixer + decimate in one pass over the kept samples only
        COMMS_TRY(comms_fir_run_dev(h->fir.get(), d_in, n, a, s));
        COMMS_TRY(comms_mixer_run_decim_dev(h->mixer.get(), a, n, h->rate, dec, s));
    } else {
        COMMS_TRY(h->t2.reserve(n * sizeof(comms_c32)));
        comms_c32* b = static_cast<comms_c32*>(h->t2.p);
        COMMS_TRY(chain_flush_raw_state(h));
        COMMS_TRY(comms_mixer_run_dev(h->mixer.get(), d_in, n, a, s));
        COMMS_TRY(comms_fir_run_dev(h->fir.get(), a, n, b, s));
        chain_raw_hist_kernel<<<dim3(1), dim3(256), 0, hs>>>(h->raw_hist.cur<float2>(), reinterpret_cast<const float2*>(d_in), n,
                                                             h->raw_hist.next<float2>(), h->fir->n_eff);
        COMMS_TRY(launch_ok("chain_raw_hist_kernel"));
        h->raw_hist.flip();
        COMMS_TRY(comms_decimate_run_dev(b, n, sizeof(comms_c32), h->rate, dec, nullptr, h->device, s));
    }
    if (h->out_bits) return sym_to_bits_launch(dec, n_dec, h->out_sym, static_cast<uint8_t*>(d_out), hs);
    if (!h->fm_demod) return COMMS_OK;
    return comms_fmdemod_run_dev(h->fm.get(), dec, n_dec, static_cast<float*>(d_out), s);
}

comms_status_t comms_chain_run(comms_chain_t* h, const comms_c32* in, size_t n, void* out) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG((in && out) || !n, "NULL host pointer");
    COMMS_ARG(n % h->rate == 0, "n (%zu) must be a multiple of the decimation rate %zu", n, h->rate);
    COMMS_TRY(use_device(h->device));
    if (!n) return COMMS_OK;
    const size_t out_bytes = chain_out_bytes(h, n / h->rate);
    const size_t in_elem = in_elem_bytes(h->in_fmt);
    // (chunks of whole groups of `rate` samples: DecimateNode restarts its index with every batch, src/util/resample_node.rs:53-65,
    // and a chunk that starts on a multiple of the rate keeps the batch's indexing; bits output: of 32 / k groups, one whole
    // 32-bit word of bits, so that every chunk but the last starts on a word of the output)
    const size_t out_elem = h->out_bits ? 4 : h->fm_demod ? sizeof(float) : sizeof(comms_c32);
    const size_t unit = h->out_bits ? h->rate * static_cast<size_t>(32 / h->out_bits) : h->rate;
    COMMS_TRY(h->run_host_units(in, n * in_elem, unit * in_elem, out, out_bytes, out_elem, [&](void* d_in, void* d_out, size_t ib, size_t) {
        return comms_chain_run_dev(h, static_cast<const comms_c32*>(d_in), ib / in_elem, d_out, COMMS_STREAM_HANDLE);
    }));
    // (a long filter runs the 16384-point FIR kernel inside the series of launches: its failure is this call's)
    return h->fir ? fir_check_sticky(h->fir.get()) : COMMS_OK;
}

// d_in of the run entries then points to raw IQ samples of that format; the conversion (iqformat.hip's
// arithmetic, bit for bit) happens in the load stage of the time-domain chain kernel -- HBM sees 4 or 2
// bytes per input sample -- and as one extra pass in front of the other chain forms.
comms_status_t comms_chain_set_input_format(comms_chain_t* h, int32_t format, float scale) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG(format == COMMS_IQ_C32 || format == COMMS_IQ_I16 || format == COMMS_IQ_U8, "unknown sample format %d", format);
    COMMS_ARG(format != COMMS_IQ_I16 || std::isfinite(scale), "scale must be finite");
    h->in_fmt = format;
    h->in_scale = format == COMMS_IQ_I16 ? scale : 1.0f;
    if (reads_wire_format(h->kind)) COMMS_TRY(comms_fir_set_input_format(h->fir.get(), format, scale));
    return COMMS_OK;
}

// Hard-decision bits instead of Complex<f32> (the receive end: matched filter, symbol-rate sampler, decision).  Stateless:
// history, phase and the checkpoint hooks are the same whichever format a call writes.
comms_status_t comms_chain_set_output_format(comms_chain_t* h, int32_t format, int32_t bits_per_sym, const comms_c32* constellation) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG(format == COMMS_SYM_C32 || format == COMMS_SYM_BITS, "the chain writes COMMS_SYM_C32 or COMMS_SYM_BITS (got format %d)", format);
    if (format == COMMS_SYM_C32) {
        h->out_bits = 0;
        return COMMS_OK;
    }
    COMMS_ARG(!h->fm_demod, "a chain with FM demod writes angles: no bits output");
    SymTable t;
    COMMS_TRY(sym_table(bits_per_sym, constellation, &t));
    h->out_sym = t;
    h->out_bits = bits_per_sym;
    return COMMS_OK;
}

comms_status_t comms_chain_set_timer(comms_chain_t* h, comms_timer_t* t) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    return comms_fir_set_timer(h->fir.get(), t);
}

comms_status_t comms_chain_set_fir_state(comms_chain_t* h, const comms_c32* state, size_t n_state) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG(state || !n_state, "state is NULL");
    COMMS_TRY(use_device(h->device));
    COMMS_TRY(h->quiesce());
    if (!has_raw_history(h->kind)) return comms_fir_set_state(h->fir.get(), state, n_state);
    COMMS_ARG(n_state == static_cast<size_t>(h->fir->n_eff), "state must hold exactly the %d effective taps", h->fir->n_eff);
    COMMS_HIP_TRY(h->raw_hist.upload(state, n_state));
    h->pending_raw.assign(state, state + n_state);  // mixed into the FIR node's history at the next run
    return COMMS_OK;
}

comms_status_t comms_chain_get_fir_state(comms_chain_t* h, comms_c32* state, size_t n_state) {
    COMMS_ARG(h && state, "NULL argument");
    COMMS_TRY(use_device(h->device));
    COMMS_TRY(h->quiesce());
    if (!has_raw_history(h->kind)) return comms_fir_get_state(h->fir.get(), state, n_state);
    const size_t N = static_cast<size_t>(h->fir->n_eff);
    COMMS_ARG(n_state <= N, "n_state %zu exceeds the %zu effective taps", n_state, N);
    COMMS_HIP_TRY(h->raw_hist.download(state, n_state));
    return COMMS_OK;
}

// Oscillator phase of the next input sample (radians, as comms_mixer_get_phase).
comms_status_t comms_chain_get_phase(comms_chain_t* h, double* out_phase) {
    COMMS_ARG(h && out_phase, "NULL argument");
    if (!is_fused(h->kind)) return comms_mixer_get_phase(h->mixer.get(), out_phase);
    *out_phase = static_cast<double>(h->turns >> 11) * (kMixT * 0x1.0p-53);
    return COMMS_OK;
}

comms_status_t comms_chain_set_phase(comms_chain_t* h, double phase) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG(std::isfinite(phase), "phase must be finite");
    if (!is_fused(h->kind)) return comms_mixer_set_phase(h->mixer.get(), phase);
    h->turns = mix_to_turns(phase);
    return COMMS_OK;
}

// FM.prev of the chain's demodulator (src/modulation/analog.rs:9,31): the last DECIMATED filter
// output of the previous batch.  COMMS_ERR_ARG for a chain without FM demod.
comms_status_t comms_chain_get_fm_prev(comms_chain_t* h, comms_c32* out_prev) {
    COMMS_ARG(h && out_prev, "NULL argument");
    COMMS_ARG(h->fm_demod, "this chain has no FM demodulator");
    if (h->fm_separate) return comms_fmdemod_get_prev(h->fm.get(), out_prev);
    COMMS_TRY(use_device(h->device));
    COMMS_TRY(h->quiesce());
    COMMS_HIP_TRY(h->fm_prev.download(out_prev, 1));
    return COMMS_OK;
}

comms_status_t comms_chain_set_fm_prev(comms_chain_t* h, const comms_c32* prev) {
    COMMS_ARG(h && prev, "NULL argument");
    COMMS_ARG(h->fm_demod, "this chain has no FM demodulator");
    if (h->fm_separate) return comms_fmdemod_set_prev(h->fm.get(), prev);
    COMMS_TRY(use_device(h->device));
    COMMS_TRY(h->quiesce());
    COMMS_HIP_TRY(h->fm_prev.upload(prev, 1));
    return COMMS_OK;
}

comms_status_t comms_chain_destroy(comms_chain_t* h) { return destroy_handle(h); }

}  // extern "C"
