// GPU test of the synchronisation estimator in a graph: source -> SyncEstimatorNode -> SymbolSyncNode.update alongside
// source -> SymbolSyncNode.input must give the symbols of the direct C calls (comms_syncest_run, tau = timing + (N - 1) / (2 L)
// mod S, comms_symsync_set_timing, comms_symsync_run) on the same messages, in the host-vector and the device-resident forms.
// Needs an MI355X (libcomms_hip has no CPU fallback).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../comms_rs_amd/host/comms/nodes.hpp"

using namespace comms;
using C = Complex32;

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

template <class T>
static bool same_bytes(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

constexpr size_t L = 32, S = 4;
constexpr uint32_t kD = 8;
constexpr double kAlpha = 0.35;

struct Direct {
    std::vector<comms_sync_estimate_t> est;
    std::vector<double> tau;
    std::vector<std::vector<C>> sym;
};

// The C entries on the same messages: each block's estimate sets the timing the block itself is sampled with
static Direct direct(const std::vector<float>& taps, const std::vector<std::vector<C>>& msgs) {
    comms_syncest_t* e = nullptr;
    comms_symsync_t* h = nullptr;
    CHECK(comms_syncest_create(S, kD, kAlpha, 0, &e) == COMMS_OK);
    CHECK(comms_symsync_create(taps.data(), taps.size(), L, S, 0, &h) == COMMS_OK);
    Direct out;
    for (const auto& m : msgs) {
        comms_sync_estimate_t r{};
        CHECK(comms_syncest_run(e, reinterpret_cast<const comms_c32*>(m.data()), m.size(), &r) == COMMS_OK);
        double tau = std::fmod(r.timing + static_cast<double>(taps.size() - 1) / (2.0 * L), static_cast<double>(S));
        if (tau < 0) tau += static_cast<double>(S);
        CHECK(comms_symsync_set_timing(h, tau) == COMMS_OK);
        std::vector<C> y(m.size() / S);
        CHECK(comms_symsync_run(h, reinterpret_cast<const comms_c32*>(m.data()), m.size(), y.data()) == COMMS_OK);
        out.est.push_back(r);
        out.tau.push_back(tau);
        out.sym.push_back(std::move(y));
    }
    comms_syncest_destroy(e);
    comms_symsync_destroy(h);
    return out;
}

// source -> estimator -> synchroniser.update, source -> synchroniser.input; one call() of each node per message
template <class Est, class Sync, class Msg, class Out, class ToHost>
static void drive(Est& est, Sync& sync, const std::vector<Msg>& msgs, const Direct& want, ToHost to_host) {
    NodeSender<Msg> src;
    NodeReceiver<comms_sync_estimate_t> est_sink;
    NodeReceiver<Out> sink;
    connect_nodes(src, est.input);
    connect_nodes(src, sync.input);
    connect_nodes(est.update, sync.update);
    connect_nodes(est.output, est_sink);
    connect_nodes(sync.output, sink);
    CHECK(est.is_connected() && sync.is_connected() && src.size() == 2);
    for (size_t i = 0; i < msgs.size(); ++i) {
        for (auto& s : src) CHECK(s.first.send(msgs[i]));
        CHECK(est.call().is_ok());
        const std::optional<comms_sync_estimate_t> r = est_sink->try_recv();
        CHECK(r.has_value());
        if (r) CHECK(std::memcmp(&*r, &want.est[i], sizeof *r) == 0);
        CHECK(sync.call().is_ok());   // drains the update the estimator has just sent, then runs the block
        const std::optional<Out> y = sink->try_recv();
        CHECK(y.has_value());
        if (y) CHECK(same_bytes(to_host(*y), want.sym[i]));
    }
}

static void test_syncest_graph() {
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    std::vector<float> taps(32 * L + 1);
    for (float& t : taps) t = noise(seed);
    // a tone at the symbol rate in |x|^2 gives the estimator something to lock to: two-level amplitude at S samples per symbol
    const size_t lens[3] = {S * 4099, S * 513, S * 1024};
    std::vector<std::vector<C>> msgs;
    for (size_t k = 0; k < 3; ++k) {
        std::vector<C> m(lens[k]);
        for (size_t i = 0; i < m.size(); ++i) {
            const float a = ((i + k) % S) < S / 2 ? 1.0f : 0.25f;
            m[i] = C(a * (1.0f + 0.1f * noise(seed)), a * 0.1f * noise(seed));
        }
        msgs.push_back(std::move(m));
    }
    const Direct want = direct(taps, msgs);
    CHECK(want.tau[0] != want.tau[1]);   // the messages' timings differ: the update matters
    {  // host vectors
        SyncEstimatorNode est(S, kD, kAlpha, taps.size(), L);
        SymbolSyncNode<C> sync(taps, L, S);
        CHECK(est.kernel(lens[0]).find("syncest_kernel") != std::string::npos);
        drive<SyncEstimatorNode, SymbolSyncNode<C>, std::vector<C>, std::vector<C>>(est, sync, msgs, want, [](const std::vector<C>& y) { return y; });
    }
    {  // device-resident messages
        std::vector<DeviceBuf<C>> dmsgs;
        for (auto& m : msgs) dmsgs.push_back(DeviceBuf<C>::from_host(m));
        SyncEstimatorNodeDev est(S, kD, kAlpha, taps.size(), L);
        SymbolSyncNodeDev<C> sync(taps, L, S);
        drive<SyncEstimatorNodeDev, SymbolSyncNodeDev<C>, DeviceBuf<C>, DeviceBuf<C>>(est, sync, dmsgs, want, [](const DeviceBuf<C>& y) { return y.to_host(); });
    }
    {  // the update's fields: tau in [0, S), the phase left alone
        SyncEstimatorNode est(S, kD, kAlpha, taps.size(), L);
        auto r = est.run(msgs[0]);
        CHECK(r.is_ok());
        if (r.is_ok()) {
            const SymbolSyncUpdate u = r.value();
            CHECK(u.tau == want.tau[0] && u.tau >= 0.0 && u.tau < static_cast<double>(S) && std::isnan(u.phase));
        }
    }
    bool threw = false;
    try {
        SyncEstimatorNode bad(8, 64, 0.25, 33, 1);   // 1025 taps
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
    test_syncest_graph();
    if (g_fail) {
        std::fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    std::puts("host GPU syncest node tests: all passed");
    return 0;
}
