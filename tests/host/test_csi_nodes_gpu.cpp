// GPU test of the channel-state path in a graph: source -> OfdmSyncNode -> DeframeNode (COMMS_SYM_C32) -> OfdmCfoCorrectNode ->
// OfdmDemodCsiNode -> WeightedDemapNode -> sink must give the records, the channel state and the LLR records of the direct C
// calls (comms_ofdmsync_run, comms_deframe_run, comms_ofdmsync_correct_run, comms_ofdm_demod_csi_run, comms_demap_run_weighted)
// on the same messages, in the host-vector and the device-resident forms.  The stream is test_ofdmsync_nodes_gpu's: four QPSK
// frames of OfdmModNode (N = 64, CP = 16, two training symbols) between gaps, behind a two-tap channel whose null sits near
// carrier 10, turned by a carrier-frequency offset, plus noise.  The weighted LLRs must decide the transmitted bits on every
// carrier but the weakest, whose weights must be the smallest.
// Needs an MI355X (libcomms_hip has no CPU fallback).
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../comms_rs_amd/host/comms/nodes.hpp"

using namespace comms;
using C = Complex32;
using Z = std::complex<double>;

static int g_fail = 0;
#define CHECK(cond)                                                                       \
    do {                                                                                  \
        if (!(cond)) {                                                                    \
            std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_fail;                                                                     \
        }                                                                                 \
    } while (0)

static uint64_t next(uint64_t& s) {  // xorshift
    s ^= s << 13;
    s ^= s >> 7;
    s ^= s << 17;
    return s;
}
static float unit(uint64_t& s) { return static_cast<float>(static_cast<int64_t>(next(s) >> 40) - (1 << 23)) / (1 << 23); }

constexpr int N = 64, CP = 16;
constexpr size_t T = 2, S = 3, kFrames = 4, D = 48, SYM = N + CP, kFrame = (T + S) * SYM, kSyms = S * D;
constexpr size_t kGuard = 40, kAdvance = 8;
constexpr double kThr = 0.5, kPi = 3.14159265358979323846, kEps = 0.3 * kPi / SYM, kSigma = 0.01;
constexpr size_t kStart[kFrames] = {150, 700, 1290, 1900}, kLens[3] = {1000, 537, 1063};
constexpr int kNull = 10;   // the channel [1, 0.9 e^{i phi}] is weakest on this bin, a data carrier

static OfdmSpec make_spec() {
    OfdmSpec f{N, CP, std::vector<uint8_t>(N, COMMS_OFDM_NULL)};
    for (int k = -26; k <= 26; ++k)
        if (k) f.carrier_kind[(k + N) % N] = (k == 7 || k == -7 || k == 21 || k == -21) ? COMMS_OFDM_PILOT : COMMS_OFDM_DATA;
    f.pilots = {C(1, 0), C(0, 1), C(-1, 0), C(0, -1)};
    f.train.resize(N);
    for (int k = -26; k <= 26; ++k)
        if (k) f.train[(k + N) % N] = C((k * k + k / 3) % 2 ? 1.0f : -1.0f, 0.0f);
    f.n_train = T;
    f.n_syms = S;
    return f;
}
static DemapSpec make_demap() {
    DemapSpec d{2, {}, kSyms};
    d.llr_scale = 0.25f;
    return d;
}

struct Want {  // what one message emits at the end of the chain
    std::vector<comms_deframe_header_t> headers;
    std::vector<uint8_t> records, llr;
    std::vector<float> csi;
};
template <class V>
static bool same_bytes(const std::vector<V>& a, const std::vector<V>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(V)) == 0);
}
template <class V>
static bool starts_with(const std::vector<V>& got, const std::vector<V>& want) {   // (a device buffer of an empty message is longer)
    return got.size() >= want.size() && (want.empty() || std::memcmp(got.data(), want.data(), want.size() * sizeof(V)) == 0);
}

// The C entries on the same messages
static std::vector<Want> direct(const OfdmSpec& format, const OfdmSyncSpec& spec, const std::vector<std::vector<C>>& msgs) {
    comms_ofdmsync_t* h = nullptr;
    comms_deframe_t* d = nullptr;
    comms_ofdm_t* o = nullptr;
    comms_demap_t* q = nullptr;
    CHECK(comms_ofdmsync_create(spec.lag, spec.window, spec.threshold, spec.guard, spec.advance, kFrame, 0, &h) == COMMS_OK);
    CHECK(comms_deframe_create(kFrame, 0, spec.lookback(), 2, nullptr, 0, 0, &d) == COMMS_OK);
    CHECK(comms_deframe_set_output_format(d, COMMS_SYM_C32) == COMMS_OK);
    CHECK(comms_ofdm_create(N, CP, format.carrier_kind.data(), reinterpret_cast<const comms_c32*>(format.pilots.data()), nullptr, 0,
                            reinterpret_cast<const comms_c32*>(format.train.data()), T, S, 0, 0, &o) == COMMS_OK);
    CHECK(comms_demap_create(2, nullptr, kSyms, 0, 0, &q) == COMMS_OK);
    CHECK(comms_demap_set_llr_scale(q, make_demap().llr_scale) == COMMS_OK);
    const size_t fb = comms_deframe_frame_bytes(d);
    std::vector<Want> out;
    std::vector<std::pair<uint64_t, double>> known;
    for (const auto& m : msgs) {
        Want w;
        const auto* x = reinterpret_cast<const comms_c32*>(m.data());
        std::vector<comms_frame_detection_t> dets(m.size());
        std::vector<double> cfo_all(m.size());
        size_t found = 0, cap = 0, n_frames = 0;
        CHECK(comms_ofdmsync_run(h, x, m.size(), dets.data(), cfo_all.data(), m.size(), &found) == COMMS_OK);
        for (size_t i = 0; i < found; ++i) known.emplace_back(dets[i].index, cfo_all[i]);
        CHECK(comms_deframe_frames_ready(d, m.size(), dets.data(), found, &cap) == COMMS_OK);
        std::vector<uint8_t> raw(cap * fb), fixed(cap * fb);
        w.headers.resize(cap);
        CHECK(comms_deframe_run(d, x, m.size(), dets.data(), found, raw.data(), cap, w.headers.data(), &n_frames) == COMMS_OK);
        CHECK(n_frames == cap);
        std::vector<double> cfo;
        for (const auto& hd : w.headers)
            for (const auto& k : known)
                if (k.first == hd.index) cfo.push_back(k.second);
        CHECK(cfo.size() == cap);
        if (cfo.size() == cap)
            CHECK(comms_ofdmsync_correct_run(h, reinterpret_cast<const comms_c32*>(raw.data()), cap, cfo.data(),
                                             reinterpret_cast<comms_c32*>(fixed.data())) == COMMS_OK);
        w.records.resize(cap * kSyms * sizeof(C));
        w.csi.resize(cap * D);
        w.llr.resize(cap * kSyms * 2 * sizeof(float));
        CHECK(comms_ofdm_demod_csi_run(o, reinterpret_cast<const comms_c32*>(fixed.data()), cap, reinterpret_cast<comms_c32*>(w.records.data()),
                                       w.csi.data()) == COMMS_OK);
        CHECK(comms_demap_run_weighted(q, reinterpret_cast<const comms_c32*>(w.records.data()), w.csi.data(), D, cap, w.llr.data()) == COMMS_OK);
        out.push_back(std::move(w));
    }
    comms_ofdmsync_destroy(h);
    comms_deframe_destroy(d);
    comms_ofdm_destroy(o);
    comms_demap_destroy(q);
    return out;
}

static std::vector<uint8_t> host(const std::vector<uint8_t>& v) { return v; }
static std::vector<uint8_t> host(const DeviceBuf<uint8_t>& v) { return v.to_host(); }
static std::vector<float> host(const std::vector<float>& v) { return v; }
static std::vector<float> host(const DeviceBuf<float>& v) { return v.to_host(); }

template <class Sync, class Deframe, class Correct, class Demod, class Demap, class Msg, class Eq, class Out>
static void drive(const std::vector<Msg>& msgs, const std::vector<Want>& want, const OfdmSpec& format, const OfdmSyncSpec& spec) {
    Sync sync(spec);
    Deframe deframe(kFrame, 0, sync.lookback(), 2, COMMS_SYM_C32);
    Correct correct(kFrame);
    Demod demod(format);
    Demap demap(make_demap());
    CHECK(demod.data_carriers() == D && demod.in_frame_bytes() == kFrame * sizeof(C) && demod.kernel(1).find("ofdm_demod_kernel") != std::string::npos);
    NodeSender<Msg> src;
    NodeReceiver<Eq> tap;   // a second consumer of the demodulator's message
    NodeReceiver<Out> sink;
    connect_nodes(src, sync.input);
    connect_nodes(src, deframe.input);
    connect_nodes(sync.detections, deframe.detections);
    connect_nodes(sync.output, correct.found);
    connect_nodes(deframe.output, correct.input);
    connect_nodes(correct.output, demod.input);
    connect_nodes(demod.output, demap.input);
    connect_nodes(demod.output, tap);
    connect_nodes(demap.output, sink);
    CHECK(sync.is_connected() && deframe.is_connected() && correct.is_connected() && demod.is_connected() && demap.is_connected());
    for (size_t i = 0; i < msgs.size(); ++i) {
        for (auto& s : src) CHECK(s.first.send(msgs[i]));
        CHECK(sync.call().is_ok());
        CHECK(deframe.call().is_ok());
        CHECK(correct.call().is_ok());
        CHECK(demod.call().is_ok());
        CHECK(demap.call().is_ok());
        const std::optional<Eq> e = tap->try_recv();
        CHECK(e.has_value());
        if (e) {
            CHECK(e->csi_period == D && e->frames.frame_bytes == kSyms * sizeof(C) && same_bytes(e->frames.headers, want[i].headers));
            CHECK(starts_with(host(e->frames.data), want[i].records) && starts_with(host(e->csi), want[i].csi));
        }
        const std::optional<Out> l = sink->try_recv();
        CHECK(l.has_value());
        if (l) CHECK(l->frame_bytes == kSyms * 2 * sizeof(float) && same_bytes(l->headers, want[i].headers) && starts_with(host(l->data), want[i].llr));
    }
}

int main() {
    int32_t n_dev = 0;
    if (comms_device_count(&n_dev) != COMMS_OK || n_dev < 1) {
        std::fprintf(stderr, "no MI355X visible\n");
        return 1;
    }
    const OfdmSpec format = make_spec();
    const OfdmSyncSpec spec = OfdmSyncSpec::for_format(format, kThr, kGuard, kAdvance);

    // the transmitted frames, and the received stream: gaps, the channel, the offset from stream index 0, noise everywhere
    uint64_t seed = 0xA4093822299F31D0ull;
    std::vector<C> data(kFrames * kSyms);
    for (auto& v : data) v = C(unit(seed) < 0 ? -1.0f : 1.0f, unit(seed) < 0 ? -1.0f : 1.0f);   // digital.rs's QPSK points
    OfdmModNode mod(format);
    const auto tx = mod.run(data);
    CHECK(tx.is_ok() && tx.value().size() == kFrames * kFrame);
    if (!tx.is_ok() || tx.value().size() != kFrames * kFrame) return 1;
    size_t total = 0;
    for (size_t len : kLens) total += len;
    std::vector<Z> clean(total + 1, Z(0, 0));
    const Z tap1 = std::polar(0.9, kPi + 2 * kPi * kNull / N);
    for (size_t f = 0; f < kFrames; ++f)
        for (size_t n = 0; n < kFrame; ++n) {
            const Z v(tx.value()[f * kFrame + n].real(), tx.value()[f * kFrame + n].imag());
            clean[kStart[f] + n] += v;
            clean[kStart[f] + n + 1] += tap1 * v;
        }
    std::vector<std::vector<C>> msgs;
    size_t k = 0;
    for (size_t len : kLens) {
        std::vector<C> m(len);
        for (size_t i = 0; i < len; ++i, ++k) {
            const Z v = clean[k] * std::polar(1.0, kEps * static_cast<double>(k)) + kSigma * Z(unit(seed), unit(seed));
            m[i] = C(static_cast<float>(v.real()), static_cast<float>(v.imag()));
        }
        msgs.push_back(std::move(m));
    }

    const std::vector<Want> want = direct(format, spec, msgs);
    CHECK(want.size() == 3);
    if (want.size() != 3) return 1;
    // every frame arrives; its weights are smallest on the null's carrier (data carrier 8: bins 1 ... 6, 8 ... 10) and the signs
    // of the weighted LLRs are the transmitted bits wherever the carrier is not next to the null (positive = bit 0 = +1)
    size_t frame = 0, wrong = 0;
    for (const Want& w : want)
        for (size_t j = 0; j < w.headers.size(); ++j, ++frame) {
            const float* g = w.csi.data() + j * D;
            size_t weakest = 0;
            for (size_t d = 0; d < D; ++d) weakest = g[d] < g[weakest] ? d : weakest;
            CHECK(weakest == 8);
            CHECK(g[weakest] > 0.0f && g[weakest] < 0.02f * g[28]);
            const float* L = reinterpret_cast<const float*>(w.llr.data()) + j * kSyms * 2;
            for (size_t s = 0; s < kSyms && frame < kFrames; ++s) {
                const size_t d = s % D;
                if (d >= 6 && d <= 10) continue;
                const C sent = data[frame * kSyms + s];
                wrong += (L[2 * s] > 0) != (sent.real() > 0);
                wrong += (L[2 * s + 1] > 0) != (sent.imag() > 0);
            }
        }
    std::printf("%zu frames, %zu wrong signs away from the null\n", frame, wrong);
    CHECK(frame == kFrames && wrong == 0);

    drive<OfdmSyncNode, DeframeNode, OfdmCfoCorrectNode, OfdmDemodCsiNode, WeightedDemapNode, std::vector<C>, OfdmDemodCsiOp::Equalised,
          DeframeOp::Frames>(msgs, want, format, spec);
    {
        std::vector<DeviceBuf<C>> dmsgs;
        for (auto& m : msgs) dmsgs.push_back(DeviceBuf<C>::from_host(m));
        drive<OfdmSyncNodeDev, DeframeNodeDev, OfdmCfoCorrectNodeDev, OfdmDemodCsiNodeDev, WeightedDemapNodeDev, DeviceBuf<C>,
              OfdmDemodCsiOp::EqualisedDev, DeframeOp::FramesDev>(dmsgs, want, format, spec);
    }
    {  // records of another length, weights that do not cover the frames, and the formats the nodes refuse
        OfdmDemodCsiNode demod(format);
        DeframeOp::Frames in{std::vector<uint8_t>(kFrame * sizeof(C) - 8), std::vector<comms_deframe_header_t>(1), kFrame * sizeof(C) - 8};
        CHECK(demod.run(in).is_err());
        WeightedDemapNode demap(make_demap());
        OfdmDemodCsiOp::Equalised eq{{std::vector<uint8_t>(kSyms * sizeof(C)), std::vector<comms_deframe_header_t>(1), kSyms * sizeof(C)},
                                     std::vector<float>(D - 1), D};
        CHECK(demap.run(eq).is_err());
        eq.csi.assign(D, 1.0f);
        CHECK(demap.run(eq).is_ok());
    }
    int threw = 0;
    try {
        OfdmSpec bad = format;
        bad.n_train = 0;
        OfdmDemodCsiNode node(bad);   // nothing to estimate from
    } catch (const std::exception&) {
        ++threw;
    }
    try {
        DemapSpec bad = make_demap();
        bad.format = COMMS_SYM_BITS;
        WeightedDemapNode node(bad);
    } catch (const std::exception&) {
        ++threw;
    }
    CHECK(threw == 2);
    if (g_fail) {
        std::fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    std::puts("host GPU channel-state node tests: all passed");
    return 0;
}
