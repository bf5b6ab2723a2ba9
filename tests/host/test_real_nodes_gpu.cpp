// GPU test of RealFirDecimNode in a graph: examples/fm_radio.rs:144-164 wired as TWO nodes -- the chain front end
// (radio bytes -> 63 taps -> /5 -> FM demod, one launch) -> RealFirDecimNode (63 taps, /5, one launch) -- against the
// example's own nine nodes called one by one (the graph of test_fm_radio_literal_graph, tests/host/test_nodes_gpu.cpp).
// Needs an MI355X (libcomms_hip has no CPU fallback).
#include <cmath>
#include <cstdio>
#include <cstdlib>
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

// The 63 taps examples/fm_radio.rs:30-52 ships, read from the fixture (tests/golden/reference_kats.json)
static std::vector<float> fm_radio_taps() {
    std::vector<float> taps;
    for (const char* path : {"tests/golden/reference_kats.json", "../../tests/golden/reference_kats.json"}) {
        std::FILE* f = std::fopen(path, "rb");
        if (!f) continue;
        std::string txt;
        char buf[4096];
        size_t got;
        while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) txt.append(buf, got);
        std::fclose(f);
        size_t p = txt.find("\"fm_radio_taps\"");
        if (p == std::string::npos) break;
        p = txt.find("\"taps_re\"", p);
        p = txt.find('[', p);
        const size_t end = txt.find(']', p);
        const char* q = txt.c_str() + p + 1;
        while (q < txt.c_str() + end) {
            char* e = nullptr;
            const double v = std::strtod(q, &e);
            if (e == q) break;
            taps.push_back(static_cast<float>(v));
            q = e;
            while (q < txt.c_str() + end && (*q == ',' || *q == ' ' || *q == '\n')) ++q;
        }
        break;
    }
    return taps;
}

// bytes -> (x - 127.5) / 127.5 -> FIR -> /rate -> FM demod as one launch (comms_chain_*, u8 load stage)
struct FrontChainU8 : DeriveNode<FrontChainU8> {
    NodeReceiver<std::vector<uint8_t>> input;
    NodeSender<std::vector<float>> output;
    FrontChainU8(const std::vector<C>& taps, size_t rate) : rate_(rate) {
        throw_on(comms_chain_create_ex(0.0, 0.0, c32(taps.data()), taps.size(), rate, COMMS_CHAIN_FM_DEMOD, 0, &h_), "FrontChainU8::new");
        throw_on(comms_chain_set_input_format(h_, COMMS_IQ_U8, 1.0f), "FrontChainU8::new");
    }
    FrontChainU8(FrontChainU8&& o) noexcept : input(std::move(o.input)), output(std::move(o.output)), h_(o.h_), rate_(o.rate_) { o.h_ = nullptr; }
    ~FrontChainU8() { comms_chain_destroy(h_); }
    Result<std::vector<float>> run(const std::vector<uint8_t>& b) {
        const size_t n = b.size() / 2;
        if (n % rate_) return NodeError::DataError;
        std::vector<float> out(n / rate_);
        if (comms_chain_run(h_, reinterpret_cast<const comms_c32*>(b.data()), n, out.data()) != COMMS_OK) return NodeError::PermanentError;
        return out;
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output); }

private:
    comms_chain_t* h_ = nullptr;
    size_t rate_;
};

static std::vector<C> convert_u8(const std::vector<uint8_t>& b) {  // fm_radio.rs:62-91
    std::vector<C> out(b.size() / 2);
    for (size_t i = 0; i < out.size(); ++i) out[i] = C((b[2 * i] - 127.5f) / 127.5f, (b[2 * i + 1] - 127.5f) / 127.5f);
    return out;
}

static void test_fm_radio_graph_as_two_nodes() {
    const std::vector<float> t32 = fm_radio_taps();
    CHECK(t32.size() == 63);
    if (t32.size() != 63) return;
    std::vector<C> taps;
    double sum_abs = 0.0;
    for (float v : t32) {
        taps.push_back(C(v, 0.f));
        sum_abs += std::fabs(v);
    }
    // four radio blocks of an FM tone on a carrier offset, quantised to the radio's bytes; 131070 samples each (the chain
    // front end takes whole decimation periods; RealFirDecimNode takes the 26214 angles of a block, not a multiple of 5)
    const size_t blk = 131070, nblk = 4;
    std::vector<std::vector<uint8_t>> blocks(nblk, std::vector<uint8_t>(2 * blk));
    for (size_t b = 0; b < nblk; ++b)
        for (size_t i = 0; i < blk; ++i) {
            const double n = static_cast<double>(b * blk + i);
            const double ph = 2.0 * M_PI * 0.02 * n + 4.0 * std::cos(2.0 * M_PI * n / 5000.0);
            blocks[b][2 * i] = static_cast<uint8_t>(std::lround(127.5 + 100.0 * std::cos(ph)));
            blocks[b][2 * i + 1] = static_cast<uint8_t>(std::lround(127.5 + 100.0 * std::sin(ph)));
        }
    // the example's nodes one by one, state carried across the blocks
    BatchFirNode f1(taps), f2(taps);
    FMDemodNode fmd;
    std::vector<std::vector<float>> angles, want;
    for (size_t b = 0; b < nblk; ++b) {
        const auto a = fmd.run(DecimateNode<C>(5).run(f1.run(convert_u8(blocks[b])).value()).value()).value();
        std::vector<C> ac(a.size());
        for (size_t i = 0; i < a.size(); ++i) ac[i] = C(a[i], 0.f);        // Convert2Node
        const auto y = f2.run(ac).value();
        std::vector<float> re(y.size());
        for (size_t i = 0; i < y.size(); ++i) re[i] = y[i].real();          // Convert3Node
        angles.push_back(a);
        want.push_back(DecimateNode<float>(5).run(re).value());
    }
    // (1) the audio stage alone on the SAME angles: the four nodes against the one, to the f32 FIR bound of the project,
    //     1e-5 sum|taps| max|x| with |x| <= pi
    {
        RealFirDecimNode audio(t32, 5);
        CHECK(audio.kernel(blk / 5).find("rfir_decim") != std::string::npos);
        double worst = 0.0;
        for (size_t b = 0; b < nblk; ++b) {
            const auto got = audio.run(angles[b]).value();
            CHECK(got.size() == want[b].size() && got.size() == (blk / 5 + 4) / 5);
            for (size_t i = 0; i < got.size() && i < want[b].size(); ++i)
                worst = std::fmax(worst, std::fabs(static_cast<double>(got[i]) - want[b][i]));
        }
        CHECK(worst <= 1e-5 * sum_abs * M_PI);
    }
    // (2) the graph as two nodes.  The front end's angles agree with the three nodes' within 2e-3 rad behind the first
    //     filter's start-up (the bound test_fm_radio_literal_graph holds it to), so the audio outputs agree within
    //     sum|taps| x that; the first outputs of block 0 filter start-up angles (|y| runs through zero there) and are left out
    {
        Replay<std::vector<uint8_t>> sdr(blocks);
        FrontChainU8 front(taps, 5);
        RealFirDecimNode audio(t32, 5);
        Collect<std::vector<float>> sink;
        connect_nodes(sdr.output, front.input);
        connect_nodes(front.output, audio.input);
        connect_nodes(audio.output, sink.input);
        start_nodes(std::move(sdr), std::move(front), std::move(audio));
        while (sink.call().is_ok()) {
        }
        CHECK(sink.got.size() == nblk);
        double worst = 0.0;
        for (size_t b = 0; b < nblk && b < sink.got.size(); ++b) {
            CHECK(sink.got[b].size() == want[b].size());
            for (size_t i = (b == 0 ? (63 / 5 + 1 + 63) / 5 + 1 : 0); i < want[b].size() && i < sink.got[b].size(); ++i)
                worst = std::fmax(worst, std::fabs(static_cast<double>(sink.got[b][i]) - want[b][i]));
        }
        CHECK(worst <= sum_abs * 2e-3);
        // what comes out is the instantaneous frequency per decimated sample times the filter's DC gain
        if (!sink.got.empty() && sink.got.back().size() > 1000) {
            double mean = 0.0;
            const auto& v = sink.got.back();
            for (size_t i = 200; i < v.size(); ++i) mean += v[i];
            mean /= static_cast<double>(v.size() - 200);
            CHECK(std::fabs(mean - 2.0 * M_PI * 0.02 * 5.0 * 1.0363602) < 0.02);
        }
    }
    // (3) the device-message form: the angles as DeviceBuf messages, equal to the host-vector node bit for bit
    {
        std::vector<DeviceBuf<float>> msgs;
        for (auto& a : angles) msgs.push_back(DeviceBuf<float>::from_host(a));
        Replay<DeviceBuf<float>> src(msgs);
        RealFirDecimNodeDev dev(t32, 5);
        Collect<DeviceBuf<float>> sink;
        connect_nodes(src.output, dev.input);
        connect_nodes(dev.output, sink.input);
        start_nodes(std::move(src), std::move(dev));
        while (sink.call().is_ok()) {
        }
        CHECK(sink.got.size() == nblk);
        RealFirDecimNode host(t32, 5);
        for (size_t b = 0; b < nblk && b < sink.got.size(); ++b) CHECK(sink.got[b].to_host() == host.run(angles[b]).value());
    }
}

int main() {
    int32_t n_dev = 0;
    if (comms_device_count(&n_dev) != COMMS_OK || n_dev < 1) {
        std::fprintf(stderr, "no MI355X visible\n");
        return 1;
    }
    test_fm_radio_graph_as_two_nodes();
    if (g_fail) {
        std::fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    std::puts("host GPU real-stream node tests: all passed");
    return 0;
}
