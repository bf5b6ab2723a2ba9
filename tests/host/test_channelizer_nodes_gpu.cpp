// GPU test of the polyphase channelizer in a graph: a source feeds ChannelizerNode, whose one sender feeds M sinks, sink k
// keeping channel k of every message; the values must be those the Python helper (tests/channelizer_ref.py, float64) wrote
// to the case file given as argv[1], within the bound written there, and ChannelizerNodeDev (device-resident messages) and
// the frame-major layout must hold the bits of the host node.  State is carried across ragged messages.
// Needs an MI355X (libcomms_hip has no CPU fallback).
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
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

struct Replay : DeriveNode<Replay> {
    std::vector<std::vector<C>> items;
    size_t i = 0;
    NodeSender<std::vector<C>> output;
    explicit Replay(std::vector<std::vector<C>> v) : items(std::move(v)) {}
    Result<std::vector<C>> run() {
        if (i >= items.size()) {
            output.clear();  // a Graph keeps its nodes alive: dropping the sender is what ends the channelizer's loop
            return NodeError::DataEnd;
        }
        return items[i++];
    }
    auto receivers() { return std::tie(); }
    auto senders() { return std::tie(output); }
};
// Sink k: channel k of each channel-major message.  A Graph keeps its nodes alive, so a sink ends itself after the
// expected number of messages.
struct ChannelSink : DeriveNode<ChannelSink> {
    NodeReceiver<std::vector<C>> input;
    size_t k, channels, left;
    std::vector<std::vector<C>> got;
    ChannelSink(size_t k_, size_t channels_, size_t expect) : k(k_), channels(channels_), left(expect) {}
    Result<Unit> run(const std::vector<C>& v) {
        const size_t frames = v.size() / channels;
        got.emplace_back(v.begin() + k * frames, v.begin() + (k + 1) * frames);
        if (--left == 0) return NodeError::DataEnd;
        return Unit{};
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(); }
};

struct Case {
    uint64_t M = 0, D = 0, N = 0, calls = 0;
    std::vector<float> taps;
    double bound = 0;
    std::vector<std::vector<C>> in;
    std::vector<std::vector<std::complex<double>>> want;  // [call][k frames + j]
    std::vector<uint64_t> frames;
};

static bool rd(std::FILE* f, void* p, size_t bytes) { return std::fread(p, 1, bytes, f) == bytes; }

static bool load(const char* path, Case& c) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    uint64_t head[4];
    bool ok = rd(f, head, sizeof head);
    c.M = head[0], c.D = head[1], c.N = head[2], c.calls = head[3];
    ok = ok && c.M >= 1 && c.M <= 1024 && c.N >= 1 && c.N <= (1u << 20) && c.calls <= 64;
    if (ok) {
        c.taps.resize(c.N);
        ok = rd(f, c.taps.data(), c.N * sizeof(float)) && rd(f, &c.bound, sizeof(double));
    }
    for (uint64_t i = 0; ok && i < c.calls; ++i) {
        uint64_t nf[2];
        ok = rd(f, nf, sizeof nf) && nf[0] <= (1u << 24) && nf[1] <= (1u << 24);
        if (!ok) break;
        c.in.emplace_back(nf[0]);
        c.want.emplace_back(nf[1] * c.M);
        c.frames.push_back(nf[1]);
        ok = rd(f, c.in.back().data(), nf[0] * sizeof(C)) && rd(f, c.want.back().data(), nf[1] * c.M * sizeof(std::complex<double>));
    }
    std::fclose(f);
    return ok;
}

static bool same_bytes(const std::vector<C>& a, const std::vector<C>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(C)) == 0);
}

static void test_channelizer_graph(const Case& c) {
    std::vector<std::shared_ptr<ChannelSink>> sinks;
    {  // host vectors through a Graph: one sender, M receivers
        auto src = std::make_shared<Replay>(c.in);
        auto ch = std::make_shared<ChannelizerNode>(c.taps, c.M, c.D);
        CHECK(ch->kernel(c.in[0].size()).find("channelizer_kernel") != std::string::npos);
        CHECK(ch->channels() == c.M);
        Graph g;
        g.connect_nodes(src->output, ch->input);
        std::vector<std::shared_ptr<Node>> nodes{src, ch};
        for (size_t k = 0; k < c.M; ++k) {
            sinks.push_back(std::make_shared<ChannelSink>(k, c.M, c.calls));
            g.connect_nodes(ch->output, sinks.back()->input);
            nodes.push_back(sinks.back());
        }
        g.add_nodes(nodes);
        CHECK(g.is_connected());
        g.run_graph();
        g.join();  // the sinks end themselves, the channelizer with its input
        for (size_t k = 0; k < c.M; ++k) {
            CHECK(sinks[k]->got.size() == c.calls);
            for (size_t b = 0; b < sinks[k]->got.size(); ++b) {
                const auto& y = sinks[k]->got[b];
                CHECK(y.size() == c.frames[b]);
                double worst = 0;
                for (size_t j = 0; j < y.size() && j < c.frames[b]; ++j) {
                    const std::complex<double> d = std::complex<double>(y[j].real(), y[j].imag()) - c.want[b][k * c.frames[b] + j];
                    worst = std::max(worst, std::abs(d));
                }
                CHECK(worst <= c.bound);
            }
        }
    }
    // the same messages through the C entry, the device node and the frame-major layout: the bits of the host node
    ChannelizerNodeDev dev(c.taps, c.M, c.D);
    ChannelizerNode frm(c.taps, c.M, c.D, COMMS_CHANNELIZER_FRAME_MAJOR);
    for (size_t b = 0; b < c.calls; ++b) {
        const std::vector<C> y = dev.run(DeviceBuf<C>::from_host(c.in[b])).value().to_host();
        const std::vector<C> z = frm.run(c.in[b]).value();
        const size_t frames = c.frames[b];
        CHECK(y.size() == frames * c.M && z.size() == frames * c.M);
        for (size_t k = 0; k < c.M && y.size() == frames * c.M; ++k) {
            CHECK(same_bytes(std::vector<C>(y.begin() + k * frames, y.begin() + (k + 1) * frames), sinks[k]->got[b]));
            for (size_t j = 0; j < frames && z.size() == frames * c.M; ++j)
                if (std::memcmp(&z[j * c.M + k], &y[k * frames + j], sizeof(C)) != 0) {
                    CHECK(!"frame-major differs from channel-major");
                    break;
                }
        }
    }
    {  // beyond the kernel's range the node is the series of chains: same interface
        ChannelizerNode series(std::vector<float>(25, 0.04f), 12, 5);
        CHECK(series.kernel(100).find("series") != std::string::npos);
        const auto y = series.run(std::vector<C>(101, C(1.0f, 0.0f)));
        CHECK(y.is_ok() && y.value().size() == 21 * 12);
        // a constant input: channel 0 settles at the filter's DC gain, 25 * 0.04 = 1
        if (y.is_ok() && y.value().size() == 21 * 12) CHECK(std::abs(y.value()[20] - C(1.0f, 0.0f)) < 1e-4f);
    }
}

int main(int argc, char** argv) {
    int32_t n_dev = 0;
    if (comms_device_count(&n_dev) != COMMS_OK || n_dev < 1) {
        std::fprintf(stderr, "no MI355X visible\n");
        return 1;
    }
    Case c;
    if (argc < 2 || !load(argv[1], c)) {
        std::fprintf(stderr, "usage: test_channelizer_nodes_gpu <case file written by tests/test_gpu_channelizer.py>\n");
        return 1;
    }
    test_channelizer_graph(c);
    if (g_fail) {
        std::fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    std::puts("host GPU channelizer node tests: all passed");
    return 0;
}
