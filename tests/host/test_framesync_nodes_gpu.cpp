// GPU test of the frame synchroniser in a graph: source -> SymbolSyncNode -> FrameSyncNode -> sink must give the detections
// of the direct C calls (comms_symsync_run, comms_framesync_run, comms_framesync_flush) on the same messages, in the
// host-vector and the device-resident forms.  The stream carries a known word twice -- once across a message boundary -- as
// symbols at S samples per symbol; with a one-tap matched filter the synchroniser passes every S-th sample through.
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

static bool same_bytes(const Det& a, const Det& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(comms_frame_detection_t)) == 0);
}

constexpr size_t S = 4, kGuard = 12;
constexpr double kThr = 0.8;
static const float kBarker[13] = {1, 1, 1, 1, 1, -1, -1, 1, 1, -1, 1, -1, 1};

// The C entries on the same messages; the last entry is the flush
static std::vector<Det> direct(const std::vector<float>& taps, const std::vector<C>& word, const std::vector<std::vector<C>>& msgs) {
    comms_symsync_t* h = nullptr;
    comms_framesync_t* f = nullptr;
    CHECK(comms_symsync_create(taps.data(), taps.size(), 1, S, 0, &h) == COMMS_OK);
    CHECK(comms_framesync_create(reinterpret_cast<const comms_c32*>(word.data()), word.size(), kThr, kGuard, 0, &f) == COMMS_OK);
    std::vector<Det> out;
    for (const auto& m : msgs) {
        std::vector<C> y(m.size() / S);
        CHECK(comms_symsync_run(h, reinterpret_cast<const comms_c32*>(m.data()), m.size(), y.data()) == COMMS_OK);
        Det d(y.size());
        size_t found = 0;
        CHECK(comms_framesync_run(f, reinterpret_cast<const comms_c32*>(y.data()), y.size(), d.data(), d.size(), &found) == COMMS_OK);
        d.resize(found);
        out.push_back(std::move(d));
    }
    Det d(64);
    size_t found = 0;
    CHECK(comms_framesync_flush(f, d.data(), d.size(), &found) == COMMS_OK);
    d.resize(found);
    out.push_back(std::move(d));
    comms_symsync_destroy(h);
    comms_framesync_destroy(f);
    return out;
}

// source -> synchroniser -> frame synchroniser -> sink; one call() of each node per message, then the flush
template <class Sync, class Frame, class Msg>
static void drive(Sync& sync, Frame& frame, const std::vector<Msg>& msgs, const std::vector<Det>& want) {
    NodeSender<Msg> src;
    NodeReceiver<Det> sink;
    connect_nodes(src, sync.input);
    connect_nodes(sync.output, frame.input);
    connect_nodes(frame.output, sink);
    CHECK(sync.is_connected() && frame.is_connected());
    for (size_t i = 0; i < msgs.size(); ++i) {
        for (auto& s : src) CHECK(s.first.send(msgs[i]));
        CHECK(sync.call().is_ok());
        CHECK(frame.call().is_ok());
        const std::optional<Det> d = sink->try_recv();
        CHECK(d.has_value());   // every block sends a vector, possibly an empty one
        if (d) CHECK(same_bytes(*d, want[i]));
    }
    auto last = frame.flush();
    CHECK(last.is_ok());
    if (last.is_ok()) CHECK(same_bytes(last.value(), want.back()));
}

static void test_framesync_graph() {
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    const std::vector<float> taps(1, 1.0f);
    std::vector<C> word;
    for (float b : kBarker) word.push_back(C(b, 0.0f));
    // symbols: noisy QPSK, the word rotated by 0.7 rad at symbols 100 and 1019 (the second straddles the first boundary at 1024)
    const size_t n_sym = 1024 + 513 + 2100, at[2] = {100, 1019};
    std::vector<C> sym(n_sym);
    for (C& v : sym) v = C((noise(seed) < 0 ? -1.0f : 1.0f) + 0.05f * noise(seed), (noise(seed) < 0 ? -1.0f : 1.0f) + 0.05f * noise(seed));
    const C rot(std::cos(0.7f), std::sin(0.7f));
    for (size_t a : at)
        for (size_t j = 0; j < word.size(); ++j) sym[a + j] = word[j] * rot + C(0.05f * noise(seed), 0.05f * noise(seed));
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
    const std::vector<Det> want = direct(taps, word, msgs);
    CHECK(want.size() == 4);
    // the word at 100 is decided by the first block; the one at 1019 ends at 1031, its guard window at 1043: the second block
    CHECK(want[0].size() == 1 && want[0][0].index == 100);
    CHECK(want[1].size() == 1 && want[1][0].index == 1019);
    CHECK(want[2].empty() && want[3].empty());
    if (want[1].size() == 1) {
        const comms_frame_detection_t& d = want[1][0];
        CHECK(std::fabs(std::atan2(d.corr_im, d.corr_re) - 0.7f) < 0.05f && d.metric > 0.9f && d.metric < 1.001f);
    }
    {  // host vectors
        SymbolSyncNode<C> sync(taps, 1, S);
        FrameSyncNode frame(word, kThr, kGuard);
        CHECK(frame.kernel(1024).find("framesync_kernel") != std::string::npos);
        drive<SymbolSyncNode<C>, FrameSyncNode, std::vector<C>>(sync, frame, msgs, want);
    }
    {  // device-resident messages
        std::vector<DeviceBuf<C>> dmsgs;
        for (auto& m : msgs) dmsgs.push_back(DeviceBuf<C>::from_host(m));
        SymbolSyncNodeDev<C> sync(taps, 1, S);
        FrameSyncNodeDev frame(word, kThr, kGuard);
        drive<SymbolSyncNodeDev<C>, FrameSyncNodeDev, DeviceBuf<C>>(sync, frame, dmsgs, want);
    }
    bool threw = false;
    try {
        FrameSyncNode bad(word, 1.5, kGuard);   // threshold beyond 1
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
    test_framesync_graph();
    if (g_fail) {
        std::fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    std::puts("host GPU framesync node tests: all passed");
    return 0;
}
