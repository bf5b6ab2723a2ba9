// GPU tests of the C++ transmit source node in a graph, written like the reference's node tests
// (src/prns.rs:146-221: PrnsNode -> CheckNode): the bits that arrive downstream are compared with a plain serial
// LFSR (prns.rs:64-71), across the node's device-generated blocks, for an 8-bit and a 64-bit register.  Needs an
// MI355X (libcomms_hip has no CPU fallback).
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "../../comms_rs_amd/host/comms/nodes.hpp"

using namespace comms;

static int g_fail = 0;
#define CHECK(cond)                                                                       \
    do {                                                                                  \
        if (!(cond)) {                                                                    \
            std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_fail;                                                                     \
        }                                                                                 \
    } while (0)

template <class T>
struct Collect : DeriveNode<Collect<T>> {
    NodeReceiver<T> input;
    std::vector<T> got;
    Result<Unit> run(const T& v) {
        got.push_back(v);
        return Unit{};
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(); }
};

// PrnGen::next_byte for a W-bit register
static uint8_t serial_step(uint64_t mask, uint64_t& state, int w) {
    const uint64_t wm = w == 64 ? ~0ull : (1ull << w) - 1;
    const uint8_t out = static_cast<uint8_t>((state >> (w - 1)) & 1);
    const uint64_t fb = static_cast<uint64_t>(__builtin_popcountll(state & mask) & 1);
    state = ((state << 1) | fb) & wm;
    return out;
}

// same thread: the source's call() sends into the channel, the check node's call() receives
static void test_prns_node_in_graph(uint64_t mask, uint64_t state, int w, size_t n) {
    PrnsNode src(mask, state, w);
    Collect<uint8_t> chk;
    connect_nodes(src.output, chk.input);
    for (size_t i = 0; i < n; ++i) {
        CHECK(src.call().is_ok());
        CHECK(chk.call().is_ok());
    }
    uint64_t s = state;
    size_t bad = 0;
    CHECK(chk.got.size() == n);
    for (size_t i = 0; i < chk.got.size(); ++i)
        if (chk.got[i] != serial_step(mask, s, w)) ++bad;
    CHECK(bad == 0);
    CHECK(src.state() == s);  // the register before the next bit, although the handle runs a block ahead
}

int main() {
    int32_t ndev = 0;
    if (comms_device_count(&ndev) != COMMS_OK || ndev < 1) {
        std::fprintf(stderr, "no MI355X visible: %s\n", comms_last_error());
        return 2;
    }
    test_prns_node_in_graph(0xB8, 0x01, 8, 2 * PrnsNode::kBlock + 100);
    test_prns_node_in_graph(0xD800000000000000ull, 0x0123456789ABCDEFull, 64, PrnsNode::kBlock + 1);
    bool refused = false;
    try {
        PrnsNode bad(0x1C0, 1, 8);  // mask wider than the register
    } catch (const std::runtime_error&) {
        refused = true;
    }
    CHECK(refused);
    if (g_fail) {
        std::fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    std::puts("host GPU transmit node tests: all passed");
    return 0;
}
