// GPU test of a digital link from bits to bits in a C++ graph: PrnsNode -> (bits packed into bytes) -> PulseBitsNode (QPSK,
// RRC, mixer, i16) -> ChainBitsNode (i16, unmixing, the same RRC, keep every sps-th, hard decisions) -> check.  The bits
// that arrive are the LFSR's (src/prns.rs:64-71, stepped serially here) delayed by the combined filter's (N - 1) / sps
// symbols, with no error: the ISI of the 33-tap RRC pair at 4 samples per symbol is far below the decision margin.
// Needs an MI355X (libcomms_hip has no CPU fallback).
#include <cmath>
#include <cstdio>
#include <optional>
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

// bits (one per message) -> bytes, LSB first, kBytes per message
struct PackNode : DeriveNode<PackNode> {
    static constexpr size_t kBytes = 512;
    NodeReceiver<uint8_t> input;
    NodeSender<std::vector<uint8_t>> output;
    std::vector<uint8_t> cur;
    size_t n_bits = 0;
    Result<std::optional<std::vector<uint8_t>>> run(const uint8_t& bit) {
        if (n_bits % 8 == 0) cur.push_back(0);
        cur.back() |= static_cast<uint8_t>((bit & 1u) << (n_bits % 8));
        if (++n_bits < 8 * kBytes) return std::optional<std::vector<uint8_t>>{};
        n_bits = 0;
        std::vector<uint8_t> out;
        out.swap(cur);
        return std::optional<std::vector<uint8_t>>{std::move(out)};
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output); }
};

struct Collect : DeriveNode<Collect> {
    NodeReceiver<std::vector<uint8_t>> input;
    std::vector<uint8_t> got;
    Result<Unit> run(const std::vector<uint8_t>& v) {
        got.insert(got.end(), v.begin(), v.end());
        return Unit{};
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(); }
};

static uint8_t serial_step(uint64_t mask, uint64_t& state, int w) {
    const uint64_t wm = w == 64 ? ~0ull : (1ull << w) - 1;
    const uint8_t out = static_cast<uint8_t>((state >> (w - 1)) & 1);
    const uint64_t fb = static_cast<uint64_t>(__builtin_popcountll(state & mask) & 1);
    state = ((state << 1) | fb) & wm;
    return out;
}

static void test_qpsk_link(size_t n_msgs) {
    const size_t sps = 4, n_taps = 8 * sps + 1;
    const int k = 2;
    std::vector<Complex32> taps(n_taps);
    throw_on(comms_rrc_taps(static_cast<uint32_t>(n_taps), static_cast<double>(sps), 0.35, c32(taps.data())), "rrc_taps");
    double sum_abs = 0.0;
    for (const Complex32& t : taps) sum_abs += std::abs(t.real());
    const float scale = static_cast<float>(std::floor(32767.0 / (sum_abs * std::sqrt(2.0) * 1.01)));  // no i16 saturation
    const double dphase = 2.0 * M_PI * 0.0173;
    const uint64_t mask = 0xD04FBB5Aull, state = 0x2468ACE1ull;

    PrnsNode src(mask, state, 32);
    PackNode pack;
    PulseBitsNode tx(taps, sps, k, dphase, scale);
    ChainBitsNode rx(-dphase, 0.0, taps, sps, k, 1.0f / scale);
    Collect chk;
    connect_nodes(src.output, pack.input);
    connect_nodes(pack.output, tx.input);
    connect_nodes(tx.output, rx.input);
    connect_nodes(rx.output, chk.input);
    for (size_t m = 0; m < n_msgs; ++m) {
        for (size_t i = 0; i < 8 * PackNode::kBytes; ++i) {
            CHECK(src.call().is_ok());
            CHECK(pack.call().is_ok());
        }
        CHECK(tx.call().is_ok());
        CHECK(rx.call().is_ok());
        CHECK(chk.call().is_ok());
    }
    CHECK(rx.fused_kind() == 2);  // i16 in, 33 taps at rate 4: fir_decim_kernel, the decision in its store stage
    const size_t n_bits = n_msgs * 8 * PackNode::kBytes;
    CHECK(chk.got.size() * 8 == n_bits);
    const size_t delay_bits = (n_taps - 1) / sps * k;  // 8 symbols
    uint64_t s = state;
    size_t bad = 0;
    for (size_t i = 0; i + delay_bits < n_bits; ++i) {
        const size_t j = i + delay_bits;
        const uint8_t got = static_cast<uint8_t>((chk.got[j / 8] >> (j % 8)) & 1u);
        if (got != serial_step(mask, s, 32)) ++bad;
    }
    if (bad) std::fprintf(stderr, "%zu bit errors\n", bad);
    CHECK(bad == 0);
    // the device counter agrees
    std::vector<uint8_t> want((n_bits + 7) / 8, 0);
    s = state;
    for (size_t i = 0; i < n_bits; ++i) want[i / 8] |= static_cast<uint8_t>(serial_step(mask, s, 32) << (i % 8));
    uint64_t errors = ~0ull;
    CHECK(comms_bit_errors(chk.got.data() + delay_bits / 8, want.data(), n_bits - delay_bits, &errors, 0) == COMMS_OK);
    CHECK(errors == 0);
}

int main() {
    int32_t ndev = 0;
    if (comms_device_count(&ndev) != COMMS_OK || ndev < 1) {
        std::fprintf(stderr, "no MI355X visible: %s\n", comms_last_error());
        return 2;
    }
    test_qpsk_link(4);
    bool refused = false;
    try {
        std::vector<Complex32> taps(33, Complex32(0.1f, 0.f));
        ChainBitsNode bad(0.1, 0.0, taps, 4, 3, 1.0f);  // bits_per_sym 3
    } catch (const std::runtime_error&) {
        refused = true;
    }
    CHECK(refused);
    if (g_fail) {
        std::fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    std::puts("host GPU receive node tests: all passed");
    return 0;
}
