// GPU test of the convolutional FEC nodes in graphs.
//   1. source -> ConvEncoderNode -> PulseBitsNode -> sink: the coded records go into the bit-input modulator as they stand, and
//      the symbols are the QPSK points of the coded bits of a register stepped here bit by bit.
//   2. sources -> DeframeNode (COMMS_SYM_LLR) -> ViterbiNode -> sink, host vectors and device-resident messages: coded QPSK
//      symbols with three sign errors per frame come back as the information bits that were sent, under the deframer's headers.
// Needs an MI355X (libcomms_hip has no CPU fallback).
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
constexpr size_t T = 100, kSteps = T + K - 1, kCoded = 2 * kSteps, kFrames = 3;

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

static void test_encoder_feeds_the_modulator() {
    uint64_t seed = 0x243F6A8885A308D3ull;
    const ConvCodeSpec code{T};
    ConvEncoderNode enc(code);
    const size_t fin = enc.in_frame_bytes(), fout = enc.out_frame_bytes();
    CHECK(fin == 16 && fout == 28);
    CHECK(enc.kernel(kFrames).find("conv_encode_kernel") != std::string::npos);
    PulseBitsNode mod(std::vector<C>(1, C(1.0f, 0.0f)), 1, 2, 0.0, 100.0f);
    NodeSender<std::vector<uint8_t>> src;
    NodeReceiver<std::vector<Complex16>> sink;
    connect_nodes(src, enc.input);
    connect_nodes(enc.output, mod.input);
    connect_nodes(mod.output, sink);
    CHECK(enc.is_connected() && mod.is_connected());
    const auto frames = random_frames(seed);
    std::vector<uint8_t> msg;
    for (const auto& f : frames) {
        const auto rec = pack(f, fin);
        msg.insert(msg.end(), rec.begin(), rec.end());
    }
    for (auto& s : src) CHECK(s.first.send(msg));
    CHECK(enc.call().is_ok());
    CHECK(mod.call().is_ok());
    const auto got = sink->try_recv();
    CHECK(got.has_value() && got->size() == kFrames * fout * 4);
    if (got && got->size() == kFrames * fout * 4) {
        for (size_t f = 0; f < kFrames; ++f) {
            const auto coded = encode(frames[f]);
            for (size_t j = 0; j < fout * 4; ++j) {      // symbol j of the record: coded bits 2j (re) and 2j + 1 (im); padding is 0
                const int b0 = 2 * j < kCoded ? coded[2 * j] : 0, b1 = 2 * j + 1 < kCoded ? coded[2 * j + 1] : 0;
                const Complex16 v = (*got)[f * fout * 4 + j];
                CHECK(v.real() == (b0 ? -100 : 100) && v.imag() == (b1 ? -100 : 100));
            }
        }
    }
    // device-resident messages give the same records as the host-vector node
    ConvEncoderNodeDev dev(code);
    const auto out = dev.run(DeviceBuf<uint8_t>::from_host(msg));
    const auto host = ConvEncoderNode(code).run(msg);
    CHECK(out.is_ok() && host.is_ok());
    if (out.is_ok() && host.is_ok()) CHECK(out.value().to_host() == host.value());
    CHECK(ConvEncoderNode(code).run(std::vector<uint8_t>(fin + 1)).is_err());   // not whole records
    bool threw = false;
    try {
        ConvEncoderNode bad(ConvCodeSpec{T, 8});
    } catch (const std::exception&) {
        threw = true;
    }
    CHECK(threw);
}

static std::vector<uint8_t> bytes_of(const std::vector<uint8_t>& v) { return v; }
static std::vector<uint8_t> bytes_of(const DeviceBuf<uint8_t>& v) { return v.to_host(); }

template <class Deframe, class Decode, class Msg, class Out>
static void drive(Deframe& deframe, Decode& decode, const std::vector<Msg>& msgs, const std::vector<Det>& dets,
                  const std::vector<std::vector<std::vector<uint8_t>>>& sent) {
    NodeSender<Msg> src;
    NodeSender<Det> det_src;
    NodeReceiver<Out> sink;
    connect_nodes(src, deframe.input);
    connect_nodes(det_src, deframe.detections);
    connect_nodes(deframe.output, decode.input);
    connect_nodes(decode.output, sink);
    CHECK(deframe.is_connected() && decode.is_connected());
    for (size_t i = 0; i < msgs.size(); ++i) {
        for (auto& s : src) CHECK(s.first.send(msgs[i]));
        for (auto& s : det_src) CHECK(s.first.send(dets[i]));
        CHECK(deframe.call().is_ok());
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

static void test_deframer_feeds_the_decoder() {
    uint64_t seed = 0x13198A2E03707344ull;
    constexpr size_t kPay = kCoded / 2, kGap = 5, kMsgs = 2;
    std::vector<std::vector<C>> msgs;
    std::vector<Det> dets;
    std::vector<std::vector<std::vector<uint8_t>>> sent;
    uint64_t index = 0;
    for (size_t m = 0; m < kMsgs; ++m) {
        std::vector<C> y;
        Det det;
        sent.push_back(random_frames(seed));
        for (size_t f = 0; f < kFrames; ++f) {
            const auto coded = encode(sent[m][f]);
            det.push_back(comms_frame_detection_t{index + y.size(), 1.0f, 0.0f, 1.0f, 1.0f});
            for (size_t j = 0; j < kPay; ++j) y.push_back(C(coded[2 * j] ? -1.0f : 1.0f, coded[2 * j + 1] ? -1.0f : 1.0f));
            for (size_t e = 0; e < 3; ++e) {             // three coded bits wrong, far apart: d_free = 10 corrects them
                C& v = y[y.size() - kPay + 10 + 30 * e];
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
        ViterbiNode decode(code, 0, 8.0f);
        CHECK(decode.in_frame_bytes() == deframe.frame_bytes() && decode.out_frame_bytes() == 16);
        CHECK(decode.kernel(kFrames).find("viterbi_kernel<2,lds>") != std::string::npos);
        drive<DeframeNode, ViterbiNode, std::vector<C>, ViterbiOp::Frames>(deframe, decode, msgs, dets, sent);
        // the hard decisions of the same records are wrong: the decoder did the work
        DeframeNode hard(kPay, 0, 0, 2, COMMS_SYM_BITS);
        const auto rec = hard.run(msgs[0], dets[0]);
        CHECK(rec.is_ok());
        if (rec.is_ok()) CHECK(std::memcmp(rec.value().data.data(), pack(encode(sent[0][0]), rec.value().frame_bytes).data(), rec.value().frame_bytes) != 0);
        ViterbiOp::Frames wrong{std::vector<uint8_t>(8), {}, 8};   // records of another size
        CHECK(ViterbiNode(code).run(wrong).is_err());
    }
    {  // device-resident messages
        std::vector<DeviceBuf<C>> dmsgs;
        for (auto& m : msgs) dmsgs.push_back(DeviceBuf<C>::from_host(m));
        DeframeNodeDev deframe(kPay, 0, 0, 2, COMMS_SYM_LLR);
        ViterbiNodeDev decode(code, 0, 8.0f);
        drive<DeframeNodeDev, ViterbiNodeDev, DeviceBuf<C>, ViterbiOp::FramesDev>(deframe, decode, dmsgs, dets, sent);
    }
    bool threw = false;
    try {
        ViterbiNode bad(code, 3);   // fewer values per record than n * steps
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
    test_encoder_feeds_the_modulator();
    test_deframer_feeds_the_decoder();
    if (g_fail) {
        std::fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    std::puts("host GPU viterbi node tests: all passed");
    return 0;
}
