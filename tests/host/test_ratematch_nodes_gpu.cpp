// GPU test of the rate-matching nodes in graphs, at rate 3/4 with 17 interleaver columns and a scrambling sequence.
//   1. source -> ConvEncoderNode -> RateMatchNode -> PulseBitsNode -> sink: the transmitted records go into the bit-input
//      modulator as they stand, and the symbols are the QPSK points of bits selected, permuted and whitened here one by one
//      (write rows, read columns, skip).
//   2. sources -> DeframeNode (COMMS_SYM_LLR) -> RateDematchNode -> ViterbiNode -> sink, host vectors and device-resident
//      messages: punctured QPSK symbols with two sign errors per frame come back as the information bits that were sent.
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

static uint64_t next(uint64_t& s) {  // xorshift
    s ^= s << 13;
    s ^= s >> 7;
    s ^= s << 17;
    return s;
}

constexpr int K = 7;
constexpr uint32_t kGens[2] = {0171, 0133};
constexpr size_t T = 100, kSteps = T + K - 1, kCoded = 2 * kSteps, kFrames = 3, kCols = 17;
static const std::vector<uint8_t> kPattern = {1, 1, 0, 1, 1, 0};

// the register of include/comms_hip.h, one bit at a time
static std::vector<uint8_t> encode(const std::vector<uint8_t>& info) {
    std::vector<uint8_t> coded;
    unsigned s = 0;
    for (size_t t = 0; t < kSteps; ++t) {
        const unsigned r = ((t < T ? info[t] : 0u) << (K - 1)) | s;
        for (uint32_t g : kGens) coded.push_back(static_cast<uint8_t>(__builtin_popcount(r & g) & 1));
        s = r >> 1;
    }
    return coded;
}
// src by the definition: the kept positions written into rows of kCols cells, the columns read, cells past the end skipped
static std::vector<uint32_t> source_map() {
    std::vector<uint32_t> kept, src;
    for (size_t i = 0; i < kCoded; ++i)
        if (kPattern[i % kPattern.size()]) kept.push_back(static_cast<uint32_t>(i));
    const size_t rows = (kept.size() + kCols - 1) / kCols;
    for (size_t c = 0; c < kCols; ++c)
        for (size_t r = 0; r < rows; ++r)
            if (r * kCols + c < kept.size()) src.push_back(kept[r * kCols + c]);
    return src;
}
static std::vector<uint8_t> pack(const std::vector<uint8_t>& bits, size_t record) {
    std::vector<uint8_t> out(record, 0);
    for (size_t i = 0; i < bits.size(); ++i) out[i / 8] = static_cast<uint8_t>(out[i / 8] | (bits[i] << (i % 8)));
    return out;
}
static std::vector<std::vector<uint8_t>> random_frames(uint64_t& seed) {
    std::vector<std::vector<uint8_t>> f(kFrames, std::vector<uint8_t>(T));
    for (auto& frame : f)
        for (auto& b : frame) b = static_cast<uint8_t>(next(seed) >> 40 & 1);
    return f;
}

struct Format {
    std::vector<uint32_t> src = source_map();
    std::vector<uint8_t> scramble;   // 0 / 1 per transmitted bit
    RateMatchSpec spec{kCoded, kPattern, kCols, {}, {}};
    Format() {
        uint64_t seed = 0xA4093822299F31D0ull;
        for (size_t k = 0; k < src.size(); ++k) scramble.push_back(static_cast<uint8_t>(next(seed) >> 33 & 1));
        spec.scramble = pack(scramble, (src.size() + 7) / 8);
    }
    std::vector<uint8_t> transmit(const std::vector<uint8_t>& coded) const {
        std::vector<uint8_t> tx;
        for (size_t k = 0; k < src.size(); ++k) tx.push_back(static_cast<uint8_t>(coded[src[k]] ^ scramble[k]));
        return tx;
    }
};

static void test_rate_match_feeds_the_modulator(const Format& fmt) {
    uint64_t seed = 0x243F6A8885A308D3ull;
    const size_t E = fmt.src.size();
    const ConvCodeSpec code{T};
    ConvEncoderNode enc(code);
    RateMatchNode match(fmt.spec);
    const size_t fin = enc.in_frame_bytes(), fout = match.out_frame_bytes();
    CHECK(E == 142 && match.n_tx_bits() == E && match.in_frame_bytes() == enc.out_frame_bytes() && fout == 20);
    CHECK(match.map() == fmt.src);
    CHECK(match.kernel(kFrames).find("ratematch_tx_kernel") != std::string::npos && match.kernel(kFrames).find("table=lds") != std::string::npos);
    PulseBitsNode mod(std::vector<C>(1, C(1.0f, 0.0f)), 1, 2, 0.0, 100.0f);
    NodeSender<std::vector<uint8_t>> src;
    NodeReceiver<std::vector<Complex16>> sink;
    connect_nodes(src, enc.input);
    connect_nodes(enc.output, match.input);
    connect_nodes(match.output, mod.input);
    connect_nodes(mod.output, sink);
    CHECK(enc.is_connected() && match.is_connected() && mod.is_connected());
    const auto frames = random_frames(seed);
    std::vector<uint8_t> msg;
    for (const auto& f : frames) {
        const auto rec = pack(f, fin);
        msg.insert(msg.end(), rec.begin(), rec.end());
    }
    for (auto& s : src) CHECK(s.first.send(msg));
    CHECK(enc.call().is_ok());
    CHECK(match.call().is_ok());
    CHECK(mod.call().is_ok());
    const auto got = sink->try_recv();
    CHECK(got.has_value() && got->size() == kFrames * fout * 4);
    if (got && got->size() == kFrames * fout * 4) {
        for (size_t f = 0; f < kFrames; ++f) {
            const auto tx = fmt.transmit(encode(frames[f]));
            for (size_t j = 0; j < fout * 4; ++j) {      // symbol j of the record: transmitted bits 2j (re) and 2j + 1 (im); padding is 0
                const int b0 = 2 * j < E ? tx[2 * j] : 0, b1 = 2 * j + 1 < E ? tx[2 * j + 1] : 0;
                const Complex16 v = (*got)[f * fout * 4 + j];
                CHECK(v.real() == (b0 ? -100 : 100) && v.imag() == (b1 ? -100 : 100));
            }
        }
    }
    // device-resident messages give the same records as the host-vector node
    const auto coded = ConvEncoderNode(code).run(msg);
    CHECK(coded.is_ok());
    if (coded.is_ok()) {
        RateMatchNodeDev dev(fmt.spec);
        const auto out = dev.run(DeviceBuf<uint8_t>::from_host(coded.value()));
        const auto host = RateMatchNode(fmt.spec).run(coded.value());
        CHECK(out.is_ok() && host.is_ok());
        if (out.is_ok() && host.is_ok()) CHECK(out.value().to_host() == host.value());
    }
    CHECK(RateMatchNode(fmt.spec).run(std::vector<uint8_t>(match.in_frame_bytes() + 1)).is_err());   // not whole records
    bool threw = false;
    try {
        RateMatchNode bad(RateMatchSpec{kCoded, kPattern, E + 1, {}, {}});   // more columns than transmitted bits
    } catch (const std::exception&) {
        threw = true;
    }
    CHECK(threw);
}

static std::vector<uint8_t> bytes_of(const std::vector<uint8_t>& v) { return v; }
static std::vector<uint8_t> bytes_of(const DeviceBuf<uint8_t>& v) { return v.to_host(); }

template <class Deframe, class Dematch, class Decode, class Msg, class Out>
static void drive(Deframe& deframe, Dematch& dematch, Decode& decode, const std::vector<Msg>& msgs, const std::vector<Det>& dets,
                  const std::vector<std::vector<std::vector<uint8_t>>>& sent) {
    NodeSender<Msg> src;
    NodeSender<Det> det_src;
    NodeReceiver<Out> sink;
    connect_nodes(src, deframe.input);
    connect_nodes(det_src, deframe.detections);
    connect_nodes(deframe.output, dematch.input);
    connect_nodes(dematch.output, decode.input);
    connect_nodes(decode.output, sink);
    CHECK(deframe.is_connected() && dematch.is_connected() && decode.is_connected());
    for (size_t i = 0; i < msgs.size(); ++i) {
        for (auto& s : src) CHECK(s.first.send(msgs[i]));
        for (auto& s : det_src) CHECK(s.first.send(dets[i]));
        CHECK(deframe.call().is_ok());
        CHECK(dematch.call().is_ok());
        CHECK(decode.call().is_ok());
        const std::optional<Out> d = sink->try_recv();
        CHECK(d.has_value());
        if (!d) continue;
        CHECK(d->size() == kFrames && d->frame_bytes == 16);
        const auto data = bytes_of(d->data);
        CHECK(data.size() >= d->size() * d->frame_bytes);
        for (size_t f = 0; f < d->size() && data.size() >= d->size() * d->frame_bytes; ++f) {
            CHECK(d->headers[f].index == dets[i][f].index);
            const auto want = pack(sent[i][f], 16);
            CHECK(std::memcmp(data.data() + f * 16, want.data(), 16) == 0);
        }
    }
}

static void test_rate_dematch_feeds_the_decoder(const Format& fmt) {
    uint64_t seed = 0x13198A2E03707344ull;
    const size_t E = fmt.src.size(), kPay = E / 2, kGap = 5, kMsgs = 2;
    std::vector<std::vector<C>> msgs;
    std::vector<Det> dets;
    std::vector<std::vector<std::vector<uint8_t>>> sent;
    uint64_t index = 0;
    for (size_t m = 0; m < kMsgs; ++m) {
        std::vector<C> y;
        Det det;
        sent.push_back(random_frames(seed));
        for (size_t f = 0; f < kFrames; ++f) {
            const auto tx = fmt.transmit(encode(sent[m][f]));
            det.push_back(comms_frame_detection_t{index + y.size(), 1.0f, 0.0f, 1.0f, 1.0f});
            for (size_t j = 0; j < kPay; ++j) y.push_back(C(tx[2 * j] ? -1.0f : 1.0f, tx[2 * j + 1] ? -1.0f : 1.0f));
            for (size_t e = 0; e < 2; ++e) {             // two transmitted bits wrong: d_free = 5 at rate 3/4 corrects them
                C& v = y[y.size() - kPay + 12 + 40 * e];
                v = C(-v.real(), v.imag());
            }
            for (size_t j = 0; j < kGap; ++j) y.push_back(C(0.3f, -0.7f));
        }
        index += y.size();
        msgs.push_back(std::move(y));
        dets.push_back(std::move(det));
    }
    const ConvCodeSpec code{T, K, {kGens[0], kGens[1]}};
    {  // host vectors
        DeframeNode deframe(kPay, 0, 0, 2, COMMS_SYM_LLR);
        RateDematchNode dematch(fmt.spec);
        ViterbiNode decode(code, 0, 8.0f);
        CHECK(dematch.in_frame_bytes() == deframe.frame_bytes() && dematch.out_frame_bytes() == decode.in_frame_bytes());
        CHECK(dematch.kernel(kFrames).find("ratematch_rx_kernel") != std::string::npos);
        drive<DeframeNode, RateDematchNode, ViterbiNode, std::vector<C>, ViterbiOp::Frames>(deframe, dematch, decode, msgs, dets, sent);
        // the dematched records by themselves: zeros exactly at the punctured positions, the descrambled signs elsewhere
        DeframeNode again(kPay, 0, 0, 2, COMMS_SYM_LLR);
        const auto rec = again.run(msgs[0], dets[0]);
        CHECK(rec.is_ok());
        if (rec.is_ok()) {
            const auto out = RateDematchNode(fmt.spec).run(rec.value());
            CHECK(out.is_ok());
            if (out.is_ok()) {
                CHECK(out.value().frame_bytes == 4 * kCoded && out.value().size() == kFrames);
                std::vector<float> v(kCoded);
                std::memcpy(v.data(), out.value().data.data(), 4 * kCoded);
                std::vector<int> fed(kCoded, -1);
                for (size_t k = 0; k < E; ++k) fed[fmt.src[k]] = static_cast<int>(k);
                const auto coded = encode(sent[0][0]);
                size_t wrong = 0;
                for (size_t i = 0; i < kCoded; ++i) {
                    if (fed[i] < 0) CHECK(v[i] == 0.0f && !std::signbit(v[i]));
                    else wrong += (v[i] < 0.0f) != (coded[i] == 1);
                }
                CHECK(wrong == 2);   // the hard decisions are wrong where the channel was: the decoder did the work
            }
        }
        RateDematchOp::Frames other{std::vector<uint8_t>(8), {}, 8};   // records of another size
        CHECK(RateDematchNode(fmt.spec).run(other).is_err());
    }
    {  // device-resident messages
        std::vector<DeviceBuf<C>> dmsgs;
        for (auto& m : msgs) dmsgs.push_back(DeviceBuf<C>::from_host(m));
        DeframeNodeDev deframe(kPay, 0, 0, 2, COMMS_SYM_LLR);
        RateDematchNodeDev dematch(fmt.spec);
        ViterbiNodeDev decode(code, 0, 8.0f);
        drive<DeframeNodeDev, RateDematchNodeDev, ViterbiNodeDev, DeviceBuf<C>, ViterbiOp::FramesDev>(deframe, dematch, decode, dmsgs, dets, sent);
    }
    bool threw = false;
    try {
        RateDematchNode bad(fmt.spec, 3);   // fewer values per record than transmitted bits
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
    const Format fmt;
    test_rate_match_feeds_the_modulator(fmt);
    test_rate_dematch_feeds_the_decoder(fmt);
    if (g_fail) {
        std::fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    std::puts("host GPU rate matching node tests: all passed");
    return 0;
}
