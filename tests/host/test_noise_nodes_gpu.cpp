// GPU test of the random source nodes and the AWGN nodes in a C++ graph (util/rand_node.rs:26-152 and its three tests):
//   * seeded NormalNode / UniformNode<float> / random_bit() messages are the values of the C entries (comms_noise_*),
//     through run() one by one and through run_block();
//   * random_bit() yields only 0 and 1, UniformNode stays in [start, end) (the reference's test_random_bit / test_uniform;
//     test_normal only checks that the node runs);
//   * without a seed two nodes differ (seeded from entropy, as the reference);
//   * BatchPulseNodeDev -> AwgnNodeDev -> ChainNodeDev gives, bit for bit, what comms_pulse_run -> comms_awgn_run ->
//     comms_chain_run give in series, and AwgnNode (host vectors) the same as comms_awgn_run.
// Needs an MI355X (libcomms_hip has no CPU fallback).
#include <cmath>
#include <cstdio>
#include <cstring>
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

struct Noise {  // a C handle, for the expected values
    comms_noise_t* h = nullptr;
    explicit Noise(uint64_t seed, uint64_t stream = 0) { throw_on(comms_noise_create(seed, stream, 0, &h), "comms_noise_create"); }
    ~Noise() { comms_noise_destroy(h); }
};

static const uint64_t kSeed = 0x5EED0123456789ABull;

static void test_sources() {
    const size_t n = 2 * 4096 + 77;  // more than two of the nodes' blocks
    // NormalNode
    {
        NormalNode node(0.5, 2.0, kSeed);
        Collect<double> chk;
        connect_nodes(node.output, chk.input);
        for (size_t i = 0; i < n; ++i) {
            CHECK(node.call().is_ok());
            CHECK(chk.call().is_ok());
        }
        auto blk = node.run_block(1000);
        CHECK(blk.is_ok() && blk.value().size() == 1000);
        Noise ref(kSeed);
        std::vector<double> want(n + 1000);
        CHECK(comms_noise_normal_f64_run(ref.h, want.size(), 0.5, 2.0, want.data()) == COMMS_OK);
        CHECK(chk.got.size() == n && std::memcmp(chk.got.data(), want.data(), n * sizeof(double)) == 0);
        CHECK(blk.is_ok() && std::memcmp(blk.value().data(), want.data() + n, 1000 * sizeof(double)) == 0);
        double sum = 0.0, sq = 0.0;
        for (double v : chk.got) sum += v, sq += (v - 0.5) * (v - 0.5);
        CHECK(std::fabs(sum / n - 0.5) < 0.2 && std::fabs(std::sqrt(sq / n) - 2.0) < 0.2);
    }
    // UniformNode<float>: the reference's test_uniform range [1, 2)
    {
        UniformNode<float> node(1.0f, 2.0f, kSeed);
        Collect<float> chk;
        connect_nodes(node.output, chk.input);
        for (size_t i = 0; i < n; ++i) {
            CHECK(node.call().is_ok());
            CHECK(chk.call().is_ok());
        }
        auto blk = node.run_block(5000);  // longer than what is left of the node's block
        Noise ref(kSeed);
        std::vector<float> want(n + 5000);
        CHECK(comms_noise_uniform_run(ref.h, want.size(), 1.0f, 2.0f, want.data()) == COMMS_OK);
        CHECK(chk.got.size() == n && std::memcmp(chk.got.data(), want.data(), n * sizeof(float)) == 0);
        CHECK(blk.is_ok() && blk.value().size() == 5000 && std::memcmp(blk.value().data(), want.data() + n, 5000 * sizeof(float)) == 0);
        bool in_range = true;
        for (float v : chk.got) in_range = in_range && v >= 1.0f && v < 2.0f;
        CHECK(in_range);
    }
    // random_bit()
    {
        auto node = random_bit(kSeed);
        Collect<uint8_t> chk;
        connect_nodes(node.output, chk.input);
        for (size_t i = 0; i < n; ++i) {
            CHECK(node.call().is_ok());
            CHECK(chk.call().is_ok());
        }
        auto blk = node.run_block(4100);
        Noise ref(kSeed);
        std::vector<uint8_t> want(3 * 4096 + 4096);
        CHECK(comms_noise_bits_run(ref.h, want.size(), COMMS_BITS_U8, want.data()) == COMMS_OK);
        CHECK(chk.got.size() == n && std::memcmp(chk.got.data(), want.data(), n) == 0);
        CHECK(blk.is_ok() && blk.value().size() == 4100 && std::memcmp(blk.value().data(), want.data() + n, 4100) == 0);
        bool only_bits = true;
        size_t ones = 0;
        for (uint8_t v : chk.got) only_bits = only_bits && (v == 0 || v == 1), ones += v;
        CHECK(only_bits);
        CHECK(ones > n / 2 - n / 10 && ones < n / 2 + n / 10);
    }
    // unseeded nodes draw their seed from entropy
    {
        NormalNode a(0.0, 1.0), b(0.0, 1.0);
        CHECK(a.seed() != b.seed());
        auto va = a.run(), vb = b.run();
        CHECK(va.is_ok() && vb.is_ok() && va.value() != vb.value());
    }
    // what Uniform::new / Normal::new panic on
    bool refused = false;
    try {
        UniformNode<float> bad(2.0f, 1.0f, kSeed);
    } catch (const std::runtime_error&) {
        refused = true;
    }
    CHECK(refused);
    refused = false;
    try {
        NormalNode bad(0.0, -1.0, kSeed);
    } catch (const std::runtime_error&) {
        refused = true;
    }
    CHECK(refused);
}

static void test_awgn_nodes() {
    const size_t sps = 8, n_taps = 8 * sps + 1, n_sym = 4096, n_msgs = 3;
    const float sigma = 1.5f;  // the matched filter's output is 8 +- 1.5 sqrt(8): about 3 % of the decisions are wrong
    std::vector<Complex32> taps(n_taps);
    throw_on(comms_rrc_taps(static_cast<uint32_t>(n_taps), static_cast<double>(sps), 0.35, c32(taps.data())), "rrc_taps");
    // QPSK symbols from the source's own bits
    std::vector<std::vector<Complex32>> syms(n_msgs, std::vector<Complex32>(n_sym));
    {
        auto bits = random_bit(kSeed + 1);
        for (auto& msg : syms) {
            auto b = bits.run_block(2 * n_sym);
            CHECK(b.is_ok());
            for (size_t i = 0; i < n_sym; ++i) msg[i] = Complex32(1.0f - 2.0f * b.value()[2 * i], 1.0f - 2.0f * b.value()[2 * i + 1]);
        }
    }
    // the graph, device-resident messages
    BatchPulseNodeDev tx(taps, sps);
    AwgnNodeDev chan(sigma, kSeed, 3);
    ChainNodeDev<Complex32> rx(0.0, 0.0, taps, sps);
    struct Sink : DeriveNode<Sink> {
        NodeReceiver<DeviceBuf<Complex32>> input;
        std::vector<Complex32> got;
        Result<Unit> run(const DeviceBuf<Complex32>& b) {
            auto v = b.to_host();
            got.insert(got.end(), v.begin(), v.end());
            return Unit{};
        }
        auto receivers() { return std::tie(input); }
        auto senders() { return std::tie(); }
    } sink;
    struct Src : DeriveNode<Src> {
        NodeSender<DeviceBuf<Complex32>> output;
        const std::vector<std::vector<Complex32>>* msgs = nullptr;
        size_t next = 0;
        Result<DeviceBuf<Complex32>> run() {
            return DeviceBuf<Complex32>::from_host((*msgs)[next++]);  // the upload is synchronous
        }
        auto receivers() { return std::tie(); }
        auto senders() { return std::tie(output); }
    } src;
    src.msgs = &syms;
    connect_nodes(src.output, tx.input);
    connect_nodes(tx.output, chan.input);
    connect_nodes(chan.output, rx.input);
    connect_nodes(rx.output, sink.input);
    for (size_t m = 0; m < n_msgs; ++m) {
        CHECK(src.call().is_ok());
        CHECK(tx.call().is_ok());
        CHECK(chan.call().is_ok());
        CHECK(rx.call().is_ok());
        CHECK(sink.call().is_ok());
    }
    // the C calls in series, host pointers
    comms_pulse_t* p = nullptr;
    comms_chain_t* ch = nullptr;
    Noise nz(kSeed, 3);
    throw_on(comms_pulse_create(c32(taps.data()), n_taps, sps, 0, &p), "comms_pulse_create");
    throw_on(comms_chain_create(0.0, 0.0, c32(taps.data()), n_taps, sps, 0, 0, &ch), "comms_chain_create");
    std::vector<Complex32> want, host_node;
    AwgnNode host_chan(sigma, kSeed, 3);
    for (size_t m = 0; m < n_msgs; ++m) {
        std::vector<Complex32> a(n_sym * sps), b(n_sym * sps), d(n_sym);
        CHECK(comms_pulse_run(p, c32(syms[m].data()), n_sym, c32(a.data())) == COMMS_OK);
        CHECK(comms_awgn_run(nz.h, a.data(), a.size(), sigma, c32(b.data())) == COMMS_OK);
        CHECK(comms_chain_run(ch, c32(b.data()), b.size(), d.data()) == COMMS_OK);
        want.insert(want.end(), d.begin(), d.end());
        auto r = host_chan.run(a);
        CHECK(r.is_ok() && r.value().size() == b.size() && std::memcmp(r.value().data(), b.data(), b.size() * sizeof(Complex32)) == 0);
    }
    comms_pulse_destroy(p);
    comms_chain_destroy(ch);
    CHECK(sink.got.size() == want.size() && want.size() == n_msgs * n_sym);
    CHECK(sink.got.size() == want.size() && std::memcmp(sink.got.data(), want.data(), want.size() * sizeof(Complex32)) == 0);
    // the noise is there: the decided bits differ from the sent ones now and then, but rarely
    size_t bad = 0, cnt = 0;
    const size_t delay = (n_taps - 1) / sps;
    for (size_t j = delay; j < n_sym; ++j, ++cnt) bad += (sink.got[j].real() < 0) != (syms[0][j - delay].real() < 0);
    CHECK(bad > 0 && bad < cnt / 10);
}

int main() {
    int32_t ndev = 0;
    if (comms_device_count(&ndev) != COMMS_OK || ndev < 1) {
        std::fprintf(stderr, "no MI355X visible: %s\n", comms_last_error());
        return 2;
    }
    test_sources();
    test_awgn_nodes();
    if (g_fail) {
        std::fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    std::puts("host GPU noise node tests: all passed");
    return 0;
}
