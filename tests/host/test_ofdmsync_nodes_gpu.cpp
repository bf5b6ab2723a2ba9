// GPU test of the OFDM synchroniser in a graph: source -> OfdmSyncNode -> DeframeNode (COMMS_SYM_C32) -> OfdmCfoCorrectNode ->
// sink, the source connected to both the synchroniser and the deframer and the synchroniser's two senders to the deframer and
// the correct stage, must give the detections, offsets, headers and records of the direct C calls (comms_ofdmsync_run,
// comms_deframe_run, comms_ofdmsync_correct_run) on the same messages, in the host-vector and the device-resident forms.  The
// stream carries four frames of OfdmModNode (N = 64, CP = 16, two training symbols) between gaps, turned by a carrier-frequency
// offset of 0.3 pi / 80 rad / sample, plus noise: one frame inside the first message, two whose detection and record come out
// of different messages, one inside the third message.  What comes out must be the transmitted frames up to one constant
// rotation each.
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
using Det = std::vector<comms_frame_detection_t>;

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
constexpr size_t T = 2, S = 3, kFrames = 4, D = 48, SYM = N + CP, kFrame = (T + S) * SYM;
constexpr size_t kGuard = 40, kAdvance = 8;
constexpr double kThr = 0.5, kPi = 3.14159265358979323846, kEps = 0.3 * kPi / SYM, kSigma = 0.02;
constexpr size_t kStart[kFrames] = {150, 700, 1290, 1900}, kLens[3] = {1000, 537, 1063};

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

struct Want {  // what one message emits
    OfdmSyncFound found;
    std::vector<uint8_t> data;
    std::vector<comms_deframe_header_t> headers;
};
template <class V>
static bool same_bytes(const std::vector<V>& a, const std::vector<V>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(V)) == 0);
}
static bool same(const Want& w, const std::vector<uint8_t>& data, const std::vector<comms_deframe_header_t>& headers, size_t frame_bytes) {
    const size_t bytes = headers.size() * frame_bytes;
    return same_bytes(headers, w.headers) && data.size() >= bytes && w.data.size() == bytes &&
           (bytes == 0 || std::memcmp(data.data(), w.data.data(), bytes) == 0);
}

// The C entries on the same messages; the last entry is the synchroniser's flush
static std::vector<Want> direct(const OfdmSyncSpec& spec, const std::vector<std::vector<C>>& msgs) {
    comms_ofdmsync_t* h = nullptr;
    comms_deframe_t* d = nullptr;
    CHECK(comms_ofdmsync_create(spec.lag, spec.window, spec.threshold, spec.guard, spec.advance, kFrame, 0, &h) == COMMS_OK);
    CHECK(comms_deframe_create(kFrame, 0, spec.lookback(), 2, nullptr, 0, 0, &d) == COMMS_OK);
    CHECK(comms_deframe_set_output_format(d, COMMS_SYM_C32) == COMMS_OK);
    const size_t fb = comms_deframe_frame_bytes(d);
    CHECK(fb == kFrame * sizeof(C));
    std::vector<Want> out;
    std::vector<std::pair<uint64_t, double>> known;
    for (const auto& m : msgs) {
        Want w;
        const auto* x = reinterpret_cast<const comms_c32*>(m.data());
        w.found.detections.resize(m.size());
        w.found.cfo.resize(m.size());
        size_t found = 0, cap = 0, n_frames = 0;
        CHECK(comms_ofdmsync_run(h, x, m.size(), w.found.detections.data(), w.found.cfo.data(), m.size(), &found) == COMMS_OK);
        w.found.detections.resize(found);
        w.found.cfo.resize(found);
        for (size_t i = 0; i < found; ++i) known.emplace_back(w.found.detections[i].index, w.found.cfo[i]);
        CHECK(comms_deframe_frames_ready(d, m.size(), w.found.detections.data(), found, &cap) == COMMS_OK);
        std::vector<uint8_t> raw(cap * fb);
        w.headers.resize(cap);
        CHECK(comms_deframe_run(d, x, m.size(), w.found.detections.data(), found, raw.data(), cap, w.headers.data(), &n_frames) == COMMS_OK);
        CHECK(n_frames == cap);
        std::vector<double> cfo;
        for (const auto& hd : w.headers)
            for (const auto& k : known)
                if (k.first == hd.index) cfo.push_back(k.second);
        CHECK(cfo.size() == cap);
        w.data.resize(cap * fb);
        if (cfo.size() == cap)
            CHECK(comms_ofdmsync_correct_run(h, reinterpret_cast<const comms_c32*>(raw.data()), cap, cfo.data(),
                                             reinterpret_cast<comms_c32*>(w.data.data())) == COMMS_OK);
        out.push_back(std::move(w));
    }
    Want last;
    last.found.detections.resize(8);
    last.found.cfo.resize(8);
    size_t found = 0, dropped = 7;
    CHECK(comms_ofdmsync_flush(h, last.found.detections.data(), last.found.cfo.data(), 8, &found) == COMMS_OK);
    last.found.detections.resize(found);
    last.found.cfo.resize(found);
    out.push_back(std::move(last));
    CHECK(comms_deframe_flush(d, &dropped) == COMMS_OK && dropped == 0);
    comms_ofdmsync_destroy(h);
    comms_deframe_destroy(d);
    return out;
}

static std::vector<uint8_t> bytes_of(const std::vector<uint8_t>& v) { return v; }
static std::vector<uint8_t> bytes_of(const DeviceBuf<uint8_t>& v) { return v.to_host(); }

// source -> {synchroniser, deframer}; synchroniser -> {deframer, correct stage}; deframer -> correct stage -> sink
template <class Sync, class Deframe, class Correct, class Msg, class Out>
static void drive(Sync& sync, Deframe& deframe, Correct& correct, const std::vector<Msg>& msgs, const std::vector<Want>& want) {
    NodeSender<Msg> src;
    NodeReceiver<OfdmSyncFound> tap;   // a second consumer of the synchroniser's message
    NodeReceiver<Out> sink;
    connect_nodes(src, sync.input);
    connect_nodes(src, deframe.input);                    // the same sample blocks to both
    connect_nodes(sync.detections, deframe.detections);
    connect_nodes(sync.output, correct.found);
    connect_nodes(sync.output, tap);
    connect_nodes(deframe.output, correct.input);
    connect_nodes(correct.output, sink);
    CHECK(sync.is_connected() && deframe.is_connected() && correct.is_connected());
    for (size_t i = 0; i < msgs.size(); ++i) {
        for (auto& s : src) CHECK(s.first.send(msgs[i]));
        CHECK(sync.call().is_ok());
        CHECK(deframe.call().is_ok());
        CHECK(correct.call().is_ok());
        const std::optional<OfdmSyncFound> f = tap->try_recv();
        CHECK(f.has_value());   // every block sends a message, possibly an empty one
        if (f) CHECK(same_bytes(f->detections, want[i].found.detections) && same_bytes(f->cfo, want[i].found.cfo));
        const std::optional<Out> d = sink->try_recv();
        CHECK(d.has_value());
        if (d) CHECK(d->frame_bytes == kFrame * sizeof(C) && same(want[i], bytes_of(d->data), d->headers, d->frame_bytes));
    }
    auto last = sync.flush();
    CHECK(last.is_ok());
    if (last.is_ok()) CHECK(same_bytes(last.value().detections, want.back().found.detections) && same_bytes(last.value().cfo, want.back().found.cfo));
    CHECK(deframe.flush() == 0);
    uint64_t total = 0;
    for (size_t len : kLens) total += len;
    CHECK(sync.position() == total);
}

int main() {
    int32_t n_dev = 0;
    if (comms_device_count(&n_dev) != COMMS_OK || n_dev < 1) {
        std::fprintf(stderr, "no MI355X visible\n");
        return 1;
    }
    const OfdmSpec format = make_spec();
    const OfdmSyncSpec spec = OfdmSyncSpec::for_format(format, kThr, kGuard, kAdvance);
    CHECK(spec.lag == SYM && spec.window == SYM && spec.lookback() == 2 * SYM + kGuard + kAdvance - 1);

    // the transmitted frames, and the received stream: gaps, the offset from stream index 0, noise everywhere
    uint64_t seed = 0xA4093822299F31D0ull;
    std::vector<C> data(kFrames * S * D);
    for (auto& v : data) v = C(unit(seed) < 0 ? -0.7f : 0.7f, unit(seed) < 0 ? -0.7f : 0.7f);
    OfdmModNode mod(format);
    CHECK(mod.frame_samples() == kFrame);
    const auto tx = mod.run(data);
    CHECK(tx.is_ok() && tx.value().size() == kFrames * kFrame);
    if (!tx.is_ok() || tx.value().size() != kFrames * kFrame) return 1;
    size_t total = 0;
    for (size_t len : kLens) total += len;
    CHECK(kStart[kFrames - 1] + kFrame + 2 * SYM + kGuard <= total);
    std::vector<Z> clean(total, Z(0, 0));
    for (size_t f = 0; f < kFrames; ++f)
        for (size_t n = 0; n < kFrame; ++n) clean[kStart[f] + n] = Z(tx.value()[f * kFrame + n].real(), tx.value()[f * kFrame + n].imag());
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

    const std::vector<Want> want = direct(spec, msgs);
    CHECK(want.size() == 4);
    if (want.size() != 4) return 1;
    // A frame's peak lies at its first sample and is decided by the message that brings sample start + 2 SYM + guard - 1; its
    // record is complete with sample start - advance + kFrame - 1.  Frames 0 and 1 are decided by the first message and frame 1
    // ends in the second; frame 2 is decided by the second and ends in the third; frame 3 is decided and complete in the third.
    const size_t n_found[4] = {2, 1, 1, 0}, n_records[3] = {1, 1, 2};
    size_t f_det = 0, f_rec = 0;
    for (size_t i = 0; i < 4; ++i) {
        CHECK(want[i].found.size() == n_found[i] && want[i].found.cfo.size() == n_found[i]);
        for (size_t j = 0; j < want[i].found.size() && f_det < kFrames; ++j, ++f_det) {
            const comms_frame_detection_t& d = want[i].found.detections[j];
            CHECK(d.index == kStart[f_det] - kAdvance);
            CHECK(d.metric > 0.9f && d.metric < 1.001f);
            CHECK(std::fabs(want[i].found.cfo[j] - kEps) < 0.02 * kEps);
            CHECK(want[i].found.cfo[j] == std::atan2(static_cast<double>(d.corr_im), static_cast<double>(d.corr_re)) / static_cast<double>(SYM));
        }
    }
    CHECK(f_det == kFrames);
    for (size_t i = 0; i < 3; ++i) {
        CHECK(want[i].headers.size() == n_records[i]);
        for (size_t j = 0; j < want[i].headers.size() && f_rec < kFrames; ++j, ++f_rec) {
            CHECK(want[i].headers[j].index == kStart[f_rec] - kAdvance && want[i].headers[j].start == want[i].headers[j].index);
            // the record against the transmitted frame: one constant rotation u (least squares), then the residue.  An offset
            // wrong by the 0.02 eps allowed above turns the ends of a record by +-0.05 rad against its middle, 0.13 at a peak of
            // three times the rms amplitude 0.9, and the noise adds at most 0.03: uncorrected, eps turns them by +-2.4 rad.
            const C* got = reinterpret_cast<const C*>(want[i].data.data()) + j * kFrame;
            Z u(0, 0);
            double den = 0, worst = 0;
            for (size_t n = kAdvance; n < kFrame; ++n) {
                const Z c = clean[kStart[f_rec] - kAdvance + n];
                u += std::conj(c) * Z(got[n].real(), got[n].imag());
                den += std::norm(c);
            }
            u /= den;
            CHECK(std::fabs(std::abs(u) - 1.0) < 0.02);
            for (size_t n = kAdvance; n < kFrame; ++n) {
                const double e = std::abs(Z(got[n].real(), got[n].imag()) - u * clean[kStart[f_rec] - kAdvance + n]);
                worst = e > worst ? e : worst;
            }
            std::printf("frame %zu: |u| %.4f, worst residue %.4f\n", f_rec, std::abs(u), worst);
            CHECK(worst < 0.16);
        }
    }
    CHECK(f_rec == kFrames);

    {  // host vectors
        OfdmSyncNode sync(spec);
        DeframeNode deframe(kFrame, 0, sync.lookback(), 2, COMMS_SYM_C32);
        OfdmCfoCorrectNode correct(kFrame);
        CHECK(sync.kernel(1000).find("ofdmsync_detect_kernel") != std::string::npos);
        CHECK(correct.frame_bytes() == kFrame * sizeof(C));
        drive<OfdmSyncNode, DeframeNode, OfdmCfoCorrectNode, std::vector<C>, DeframeOp::Frames>(sync, deframe, correct, msgs, want);
    }
    {  // device-resident messages
        std::vector<DeviceBuf<C>> dmsgs;
        for (auto& m : msgs) dmsgs.push_back(DeviceBuf<C>::from_host(m));
        OfdmSyncNodeDev sync(spec);
        DeframeNodeDev deframe(kFrame, 0, sync.lookback(), 2, COMMS_SYM_C32);
        OfdmCfoCorrectNodeDev correct(kFrame);
        drive<OfdmSyncNodeDev, DeframeNodeDev, OfdmCfoCorrectNodeDev, DeviceBuf<C>, DeframeOp::FramesDev>(sync, deframe, correct, dmsgs, want);
    }
    {  // a record whose detection the correct stage never saw, and records of another length
        OfdmCfoCorrectNode correct(kFrame);
        DeframeOp::Frames in{std::vector<uint8_t>(kFrame * sizeof(C)), std::vector<comms_deframe_header_t>(1), kFrame * sizeof(C)};
        in.headers[0].index = 5;
        CHECK(correct.run(in, OfdmSyncFound{}).is_err());
        OfdmSyncFound found{Det(1), {0.0}};
        found.detections[0].index = 5;
        const auto same_record = correct.run(in, found);
        CHECK(same_record.is_ok() && same_record.value().data == in.data);   // cfo = 0: the record's values
        in.frame_bytes -= sizeof(C);
        CHECK(correct.run(in, found).is_err());
    }
    int threw = 0;
    try {
        OfdmSyncSpec bad = spec;
        bad.lag = 2049;
        OfdmSyncNode node(bad);
    } catch (const std::exception&) {
        ++threw;
    }
    try {
        OfdmCfoCorrectNode node(0);   // no correct stage
    } catch (const std::exception&) {
        ++threw;
    }
    CHECK(threw == 2);
    if (g_fail) {
        std::fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    std::puts("host GPU ofdmsync node tests: all passed");
    return 0;
}
