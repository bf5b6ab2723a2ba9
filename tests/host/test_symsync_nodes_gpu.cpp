// GPU test of the symbol synchroniser in a graph: SymbolSyncNode (host vectors; symbols and packed bits) and
// SymbolSyncNodeDev (device-resident messages) must give the bytes of the C entry (comms_symsync_run) called directly on the
// same messages with the same (tau, phase) update between them, state carried from message to message.
// Needs an MI355X (libcomms_hip has no CPU fallback).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
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
constexpr double kDphase = 0.05;
static const double kNaN = std::numeric_limits<double>::quiet_NaN();
// the update in front of message i (none in front of message 0): timing and phase, timing alone, phase alone
static const SymbolSyncUpdate kUpdates[4] = {{kNaN, kNaN}, {0.37, 1.25}, {2.5, kNaN}, {kNaN, 0.5}};

// The C entry on the same messages: out[i] as bytes (symbols, or packed bits with bits_per_sym > 0)
static std::vector<std::vector<uint8_t>> direct(const std::vector<float>& taps, const std::vector<std::vector<C>>& msgs, int bits_per_sym) {
    comms_symsync_t* h = nullptr;
    CHECK(comms_symsync_create(taps.data(), taps.size(), L, S, 0, &h) == COMMS_OK);
    CHECK(comms_symsync_set_rotation(h, kDphase, 0.0) == COMMS_OK);
    if (bits_per_sym) CHECK(comms_symsync_set_output_format(h, COMMS_SYM_BITS, bits_per_sym, nullptr) == COMMS_OK);
    std::vector<std::vector<uint8_t>> out;
    for (size_t i = 0; i < msgs.size(); ++i) {
        if (!std::isnan(kUpdates[i].tau)) CHECK(comms_symsync_set_timing(h, kUpdates[i].tau) == COMMS_OK);
        if (!std::isnan(kUpdates[i].phase)) CHECK(comms_symsync_set_rotation(h, kDphase, kUpdates[i].phase) == COMMS_OK);
        size_t m = 0;
        CHECK(comms_symsync_out_len(msgs[i].size(), S, &m) == COMMS_OK && m == msgs[i].size() / S);
        std::vector<uint8_t> y(bits_per_sym ? (m * bits_per_sym + 7) / 8 : m * sizeof(C));
        CHECK(comms_symsync_run(h, reinterpret_cast<const comms_c32*>(msgs[i].data()), msgs[i].size(), y.data()) == COMMS_OK);
        out.push_back(std::move(y));
    }
    uint32_t mu = 0;
    CHECK(comms_symsync_get_timing(h, &mu) == COMMS_OK && mu == 80);  // 2.5 * 32
    comms_symsync_destroy(h);
    return out;
}

template <class T>
static std::vector<uint8_t> bytes_of(const std::vector<T>& v) {
    std::vector<uint8_t> b(v.size() * sizeof(T));
    if (!b.empty()) std::memcpy(b.data(), v.data(), b.size());
    return b;
}

// One node on channels it is connected by: message, update, message ... in a fixed order, one call() per message -- every
// update queued when a block arrives is applied before it
template <class Node, class Msg, class Out, class ToBytes>
static void drive(Node& node, const std::vector<Msg>& msgs, const std::vector<std::vector<uint8_t>>& want, ToBytes to_bytes) {
    NodeSender<Msg> src;
    NodeSender<SymbolSyncUpdate> upd;
    NodeReceiver<Out> sink;
    connect_nodes(src, node.input);
    connect_nodes(upd, node.update);
    connect_nodes(node.output, sink);
    CHECK(node.is_connected());
    for (size_t i = 0; i < msgs.size(); ++i) {
        if (i) CHECK(upd[0].first.send(kUpdates[i]));
        CHECK(src[0].first.send(msgs[i]));
        CHECK(node.call().is_ok());
        const std::optional<Out> y = sink->try_recv();
        CHECK(y.has_value());
        if (y) CHECK(same_bytes(to_bytes(*y), want[i]));
    }
}

static void test_symsync_graph() {
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    std::vector<float> taps(32 * L + 1);
    for (float& t : taps) t = noise(seed);
    const size_t lens[4] = {S * 4099, S * 7, S * 1024, S * 333};
    std::vector<std::vector<C>> msgs;
    for (size_t n : lens) {
        std::vector<C> m(n);
        for (C& v : m) v = C(noise(seed), noise(seed));
        msgs.push_back(std::move(m));
    }
    const auto want_c = direct(taps, msgs, 0);
    const auto want_b = direct(taps, msgs, 2);
    CHECK(want_c[0].size() == 4099 * sizeof(C) && want_b[0].size() == (4099 * 2 + 7) / 8);
    {  // host vectors, symbols
        SymbolSyncNode<C> node(taps, L, S, kDphase);
        CHECK(node.kernel(lens[0]).find("symsync_kernel") != std::string::npos);
        drive<SymbolSyncNode<C>, std::vector<C>, std::vector<C>>(node, msgs, want_c, [](const std::vector<C>& y) { return bytes_of(y); });
    }
    {  // host vectors, packed bits
        SymbolSyncNode<uint8_t> node(taps, L, S, kDphase, 2);
        drive<SymbolSyncNode<uint8_t>, std::vector<C>, std::vector<uint8_t>>(node, msgs, want_b, [](const std::vector<uint8_t>& y) { return y; });
    }
    std::vector<DeviceBuf<C>> dmsgs;
    for (auto& m : msgs) dmsgs.push_back(DeviceBuf<C>::from_host(m));
    {  // device-resident messages, symbols
        SymbolSyncNodeDev<C> node(taps, L, S, kDphase);
        drive<SymbolSyncNodeDev<C>, DeviceBuf<C>, DeviceBuf<C>>(node, dmsgs, want_c, [](const DeviceBuf<C>& y) { return bytes_of(y.to_host()); });
    }
    {  // device-resident messages, packed bits
        SymbolSyncNodeDev<uint8_t> node(taps, L, S, kDphase, 2);
        drive<SymbolSyncNodeDev<uint8_t>, DeviceBuf<C>, DeviceBuf<uint8_t>>(node, dmsgs, want_b, [](const DeviceBuf<uint8_t>& y) { return y.to_host(); });
    }
    {  // without an update channel the node runs as it was set up; a message that is no multiple of S is a DataError
        SymbolSyncNode<C> node(taps, L, S, kDphase);
        CHECK(node.run(msgs[1]).is_ok());
        CHECK(node.run(std::vector<C>(S + 1)).is_err());
    }
}

int main() {
    int32_t n_dev = 0;
    if (comms_device_count(&n_dev) != COMMS_OK || n_dev < 1) {
        std::fprintf(stderr, "no MI355X visible\n");
        return 1;
    }
    test_symsync_graph();
    if (g_fail) {
        std::fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    std::puts("host GPU symsync node tests: all passed");
    return 0;
}
