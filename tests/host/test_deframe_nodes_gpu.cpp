// GPU test of the deframer in a graph: source -> SymbolSyncNode -> FrameSyncNode -> DeframeNode -> sink, the synchroniser's
// output connected to both the frame synchroniser and the deframer, must give the records and headers of the direct C calls
// (comms_symsync_run, comms_framesync_run, comms_deframe_run) on the same messages, in the host-vector and the
// device-resident forms, and the payload bits that were sent.  The stream carries a known word three times, rotated: one
// frame inside the first message, one whose word straddles the first boundary, one whose payload ends in the third message.
// With a one-tap matched filter the synchroniser passes every S-th sample through.
// Needs an MI355X (libcomms_hip has no CPU fallback).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../comms_rs_amd/host/comms/nodes.hpp"

using namespace comms;
using C = Complex32;
using Det = std::vector<comms_frame_detection_t>;

static int g_fail = 0;
#define CHECK(cond)                                                                       \
    do {                                                                                  \
        if (!(cond)) {                                                                    \
            std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_fail;                                                                     \
        }                                                                                 \
    } while (0)

static float noise(uint64_t& s) {  // xorshift, uniform in [-1, 1)
    s ^= s << 13;
    s ^= s >> 7;
    s ^= s << 17;
    return static_cast<float>(static_cast<double>(s >> 11) * (2.0 / 9007199254740992.0) - 1.0);
}

constexpr size_t S = 4, kGuard = 12, kWord = 13, kPayload = 64;
constexpr double kThr = 0.8;
static const float kBarker[kWord] = {1, 1, 1, 1, 1, -1, -1, 1, 1, -1, 1, -1, 1};

struct Want {  // what one message emits
    std::vector<uint8_t> data;
    std::vector<comms_deframe_header_t> headers;
};
static bool same(const Want& w, const std::vector<uint8_t>& data, const std::vector<comms_deframe_header_t>& headers, size_t frame_bytes) {
    const size_t bytes = headers.size() * frame_bytes;
    return headers.size() == w.headers.size() && data.size() >= bytes && w.data.size() == bytes &&
           (bytes == 0 || std::memcmp(data.data(), w.data.data(), bytes) == 0) &&
           (headers.empty() || std::memcmp(headers.data(), w.headers.data(), headers.size() * sizeof(comms_deframe_header_t)) == 0);
}

// The C entries on the same messages
static std::vector<Want> direct(const std::vector<float>& taps, const std::vector<C>& word, const std::vector<std::vector<C>>& msgs) {
    comms_symsync_t* h = nullptr;
    comms_framesync_t* f = nullptr;
    comms_deframe_t* d = nullptr;
    CHECK(comms_symsync_create(taps.data(), taps.size(), 1, S, 0, &h) == COMMS_OK);
    CHECK(comms_framesync_create(reinterpret_cast<const comms_c32*>(word.data()), word.size(), kThr, kGuard, 0, &f) == COMMS_OK);
    CHECK(comms_deframe_create(kPayload, kWord, kGuard - 1, 2, nullptr, 0, 0, &d) == COMMS_OK);
    CHECK(comms_deframe_set_output_format(d, COMMS_SYM_BITS) == COMMS_OK);
    const size_t fb = comms_deframe_frame_bytes(d);
    CHECK(fb == kPayload * 2 / 8);
    std::vector<Want> out;
    for (const auto& m : msgs) {
        std::vector<C> y(m.size() / S);
        CHECK(comms_symsync_run(h, reinterpret_cast<const comms_c32*>(m.data()), m.size(), y.data()) == COMMS_OK);
        Det det(y.size());
        size_t found = 0, cap = 0, n_frames = 0;
        CHECK(comms_framesync_run(f, reinterpret_cast<const comms_c32*>(y.data()), y.size(), det.data(), det.size(), &found) == COMMS_OK);
        det.resize(found);
        CHECK(comms_deframe_frames_ready(d, y.size(), det.data(), det.size(), &cap) == COMMS_OK);
        Want w;
        w.data.resize(cap * fb);
        w.headers.resize(cap);
        CHECK(comms_deframe_run(d, reinterpret_cast<const comms_c32*>(y.data()), y.size(), det.data(), det.size(), w.data.data(), cap,
                                w.headers.data(), &n_frames) == COMMS_OK);
        CHECK(n_frames == cap);
        out.push_back(std::move(w));
    }
    size_t dropped = 7;
    CHECK(comms_deframe_flush(d, &dropped) == COMMS_OK && dropped == 0);
    comms_symsync_destroy(h);
    comms_framesync_destroy(f);
    comms_deframe_destroy(d);
    return out;
}

static std::vector<uint8_t> bytes_of(const std::vector<uint8_t>& v) { return v; }
static std::vector<uint8_t> bytes_of(const DeviceBuf<uint8_t>& v) { return v.to_host(); }

// source -> synchroniser -> {frame synchroniser, deframer} -> sink; one call() of each node per message
template <class Sync, class Frame, class Deframe, class Msg, class Out>
static void drive(Sync& sync, Frame& frame, Deframe& deframe, const std::vector<Msg>& msgs, const std::vector<Want>& want) {
    NodeSender<Msg> src;
    NodeReceiver<Out> sink;
    connect_nodes(src, sync.input);
    connect_nodes(sync.output, frame.input);
    connect_nodes(sync.output, deframe.input);          // the same symbol blocks to both
    connect_nodes(frame.output, deframe.detections);
    connect_nodes(deframe.output, sink);
    CHECK(sync.is_connected() && frame.is_connected() && deframe.is_connected());
    for (size_t i = 0; i < msgs.size(); ++i) {
        for (auto& s : src) CHECK(s.first.send(msgs[i]));
        CHECK(sync.call().is_ok());
        CHECK(frame.call().is_ok());
        CHECK(deframe.call().is_ok());
        const std::optional<Out> d = sink->try_recv();
        CHECK(d.has_value());   // every block sends a message, possibly one without frames
        if (d) CHECK(same(want[i], bytes_of(d->data), d->headers, d->frame_bytes));
    }
    CHECK(deframe.flush() == 0);
}

static void test_deframe_graph() {
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    const std::vector<float> taps(1, 1.0f);
    std::vector<C> word;
    for (float b : kBarker) word.push_back(C(b, 0.0f));
    // symbols: QPSK, the word at 100, at 1019 (it straddles the boundary at 1024) and at 1490 (its payload ends behind the
    // boundary at 1537), everything rotated by 0.7 rad, plus noise
    const size_t n_sym = 1024 + 513 + 2100, at[3] = {100, 1019, 1490};
    std::vector<C> clean(n_sym), sym(n_sym);
    for (C& v : clean) v = C(noise(seed) < 0 ? -1.0f : 1.0f, noise(seed) < 0 ? -1.0f : 1.0f);
    for (size_t a : at)
        for (size_t j = 0; j < word.size(); ++j) clean[a + j] = word[j];
    const C rot(std::cos(0.7f), std::sin(0.7f));
    for (size_t i = 0; i < n_sym; ++i) sym[i] = clean[i] * rot + C(0.05f * noise(seed), 0.05f * noise(seed));
    const size_t lens[3] = {1024, 513, 2100};
    std::vector<std::vector<C>> msgs;
    size_t k = 0;
    for (size_t len : lens) {
        std::vector<C> m(len * S, C(0.0f, 0.0f));
        for (size_t i = 0; i < len; ++i, ++k) {
            m[i * S] = sym[k];                                         // what the one-tap synchroniser keeps
            for (size_t r = 1; r < S; ++r) m[i * S + r] = C(noise(seed), noise(seed));
        }
        msgs.push_back(std::move(m));
    }
    const std::vector<Want> want = direct(taps, word, msgs);
    CHECK(want.size() == 3);
    // one frame per message: the third word is reported by the second message, its payload complete in the third
    for (size_t i = 0; i < want.size() && i < 3; ++i) {
        CHECK(want[i].headers.size() == 1);
        if (want[i].headers.size() != 1) continue;
        const comms_deframe_header_t& hd = want[i].headers[0];
        CHECK(hd.index == at[i] && hd.start == at[i] + kWord && hd.gain == 1.0f);
        CHECK(std::fabs(std::atan2(-hd.rot_im, hd.rot_re) - 0.7f) < 0.05f);
        for (size_t j = 0; j < kPayload; ++j) {                        // the bits that were sent: bit 0 = re < 0, bit 1 = im < 0
            const C c = clean[hd.start + j];
            const unsigned v = (c.real() < 0 ? 1u : 0u) | (c.imag() < 0 ? 2u : 0u);
            CHECK(((want[i].data[j / 4] >> (2 * (j % 4))) & 3u) == v);
        }
    }
    {  // host vectors
        SymbolSyncNode<C> sync(taps, 1, S);
        FrameSyncNode frame(word, kThr, kGuard);
        DeframeNode deframe(kPayload, kWord, kGuard - 1);
        CHECK(deframe.kernel(3).find("deframe_kernel") != std::string::npos);
        drive<SymbolSyncNode<C>, FrameSyncNode, DeframeNode, std::vector<C>, DeframeOp::Frames>(sync, frame, deframe, msgs, want);
    }
    {  // device-resident messages
        std::vector<DeviceBuf<C>> dmsgs;
        for (auto& m : msgs) dmsgs.push_back(DeviceBuf<C>::from_host(m));
        SymbolSyncNodeDev<C> sync(taps, 1, S);
        FrameSyncNodeDev frame(word, kThr, kGuard);
        DeframeNodeDev deframe(kPayload, kWord, kGuard - 1);
        drive<SymbolSyncNodeDev<C>, FrameSyncNodeDev, DeframeNodeDev, DeviceBuf<C>, DeframeOp::FramesDev>(sync, frame, deframe, dmsgs, want);
    }
    bool threw = false;
    try {
        DeframeNode bad(0, kWord, kGuard - 1);   // no payload
    } catch (const std::exception&) {
        threw = true;
    }
    CHECK(threw);
}

int main() {
    int32_t n_dev = 0;
    if (comms_device_count(&n_dev) != COMMS_OK || n_dev < 1) {
        std::fprintf(stderr, "no MI355X visible\n");
        return 1;
    }
    test_deframe_graph();
    if (g_fail) {
        std::fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    std::puts("host GPU deframe node tests: all passed");
    return 0;
}
