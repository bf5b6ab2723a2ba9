// GPU test of the rational resampler in a graph: ResampleNode<float> (host vectors) and ResampleNodeDev<Complex32>
// (device-resident messages) must give the bytes of the C entry (comms_resample_run) called directly on the same
// batches, state carried from batch to batch, and the lengths of the reference's three nodes in series.
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

template <class T>
struct Replay : DeriveNode<Replay<T>> {
    std::vector<T> items;
    size_t i = 0;
    NodeSender<T> output;
    explicit Replay(std::vector<T> v) : items(std::move(v)) {}
    Result<T> run() {
        if (i >= items.size()) return NodeError::DataEnd;
        return items[i++];
    }
    auto receivers() { return std::tie(); }
    auto senders() { return std::tie(output); }
};
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

// windowed sinc, `per` taps for each of the `up` phases, cutoff at the narrower of the two Nyquist bands, DC gain `up`
static std::vector<float> lowpass(size_t up, size_t down, size_t per) {
    const size_t n = up * per;
    const double fc = 0.5 / static_cast<double>(up > down ? up : down);
    std::vector<float> h(n);
    for (size_t k = 0; k < n; ++k) {
        const double t = static_cast<double>(k) - 0.5 * static_cast<double>(n - 1);
        const double s = t == 0.0 ? 1.0 : std::sin(2.0 * M_PI * fc * t) / (2.0 * M_PI * fc * t);
        const double w = 0.54 - 0.46 * std::cos(2.0 * M_PI * static_cast<double>(k) / static_cast<double>(n - 1));
        h[k] = static_cast<float>(static_cast<double>(up) * 2.0 * fc * s * w);
    }
    return h;
}

static float noise(uint64_t& s) {  // xorshift, uniform in [-1, 1)
    s ^= s << 13;
    s ^= s >> 7;
    s ^= s << 17;
    return static_cast<float>(static_cast<double>(s >> 11) * (2.0 / 9007199254740992.0) - 1.0);
}

template <class T>
static std::vector<std::vector<T>> direct(const std::vector<float>& taps, size_t up, size_t down, const std::vector<std::vector<T>>& batches) {
    comms_resample_t* h = nullptr;
    CHECK(comms_resample_create(taps.data(), taps.size(), up, down, ResampleElem<T>::value, 0, &h) == COMMS_OK);
    std::vector<std::vector<T>> out;
    for (const auto& b : batches) {
        size_t m = 0;
        CHECK(comms_resample_out_len(b.size(), up, down, &m) == COMMS_OK);
        CHECK(m == (b.size() * up + down - 1) / down);
        std::vector<T> y(m);
        CHECK(comms_resample_run(h, b.data(), b.size(), y.data()) == COMMS_OK);
        out.push_back(std::move(y));
    }
    comms_resample_destroy(h);
    return out;
}

template <class T>
static bool same_bytes(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

static void test_resample_graph() {
    const size_t up = 147, down = 152;
    const std::vector<float> taps = lowpass(up, down, 24);
    const size_t lens[4] = {45600, 4561, 152, 30001};  // ragged: the decimator restarts with every message
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    std::vector<std::vector<float>> fb;
    std::vector<std::vector<C>> cb;
    for (size_t n : lens) {
        std::vector<float> f(n);
        std::vector<C> c(n);
        for (size_t i = 0; i < n; ++i) {
            f[i] = noise(seed);
            c[i] = C(noise(seed), noise(seed));
        }
        fb.push_back(std::move(f));
        cb.push_back(std::move(c));
    }
    const auto want_f = direct<float>(taps, up, down, fb);
    const auto want_c = direct<C>(taps, up, down, cb);
    // a resampled constant settles at the filter's DC gain per phase, about 1: the C entry itself computes something
    {
        std::vector<std::vector<float>> ones(1, std::vector<float>(4096, 1.0f));
        const auto y = direct<float>(taps, up, down, ones);
        CHECK(y[0].size() == (4096 * up + down - 1) / down && std::fabs(y[0].back() - 1.0f) < 0.01f);
    }
    {  // host vectors through a graph
        Replay<std::vector<float>> src(fb);
        ResampleNode<float> rs(taps, up, down);
        CHECK(rs.kernel(lens[0]).find("resample_kernel") != std::string::npos);
        Collect<std::vector<float>> sink;
        connect_nodes(src.output, rs.input);
        connect_nodes(rs.output, sink.input);
        start_nodes(std::move(src), std::move(rs));
        while (sink.call().is_ok()) {
        }
        CHECK(sink.got.size() == fb.size());
        for (size_t b = 0; b < sink.got.size() && b < want_f.size(); ++b) CHECK(same_bytes(sink.got[b], want_f[b]));
    }
    {  // device-resident messages through a graph
        std::vector<DeviceBuf<C>> msgs;
        for (auto& c : cb) msgs.push_back(DeviceBuf<C>::from_host(c));
        Replay<DeviceBuf<C>> src(msgs);
        ResampleNodeDev<C> rs(taps, up, down);
        Collect<DeviceBuf<C>> sink;
        connect_nodes(src.output, rs.input);
        connect_nodes(rs.output, sink.input);
        start_nodes(std::move(src), std::move(rs));
        while (sink.call().is_ok()) {
        }
        CHECK(sink.got.size() == cb.size());
        for (size_t b = 0; b < sink.got.size() && b < want_c.size(); ++b) CHECK(same_bytes(sink.got[b].to_host(), want_c[b]));
    }
    {  // the other two pairings, on the series form as well (up = 300 is beyond the kernel's range)
        const std::vector<float> t2 = lowpass(300, 7, 4);
        ResampleNode<C> host(t2, 300, 7);
        CHECK(host.kernel(100).find("series") != std::string::npos);
        std::vector<std::vector<C>> small;
        for (size_t n : {100u, 7u, 33u}) small.emplace_back(cb[0].begin(), cb[0].begin() + n);
        const auto want = direct<C>(t2, 300, 7, small);
        for (size_t b = 0; b < small.size(); ++b) CHECK(same_bytes(host.run(small[b]).value(), want[b]));
        ResampleNodeDev<float> dev(taps, up, down);
        for (size_t b = 0; b < fb.size(); ++b) CHECK(same_bytes(dev.run(DeviceBuf<float>::from_host(fb[b])).value().to_host(), want_f[b]));
    }
}

int main() {
    int32_t n_dev = 0;
    if (comms_device_count(&n_dev) != COMMS_OK || n_dev < 1) {
        std::fprintf(stderr, "no MI355X visible\n");
        return 1;
    }
    test_resample_graph();
    if (g_fail) {
        std::fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    std::puts("host GPU resample node tests: all passed");
    return 0;
}
