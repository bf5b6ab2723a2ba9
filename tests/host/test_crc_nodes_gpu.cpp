// GPU test of the frame-check nodes in the graphs of test_viterbi_nodes_gpu.cpp.
//   1. source -> CrcAttachNode -> ConvEncoderNode -> PulseBitsNode -> sink: the attached records go into the encoder as they stand,
//      and the symbols are the QPSK points of the coded bits of payload + CRC, both registers stepped here bit by bit.
//   2. sources -> DeframeNode (COMMS_SYM_LLR) -> ViterbiNode -> CrcCheckNode -> sink, host vectors and device-resident messages:
//      coded QPSK symbols with three sign errors per frame come back as the payload that was sent with pass = 1, and the frame of
//      every message that was sent with one CRC bit wrong comes back with pass = 0 -- under the deframer's headers.
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
constexpr int W = 24;
constexpr uint32_t kPoly = 0x864CFB;                      // 3GPP CRC24A, init 0, xorout 0
constexpr size_t kPayload = 76, T = kPayload + W, kSteps = T + K - 1, kCoded = 2 * kSteps, kFrames = 3;
constexpr size_t kBadFrame = 1;                           // the frame of every message that is sent with a wrong CRC bit
static const CrcSpec kCrc{W, kPoly, 0, 0, kPayload};

// the registers of include/comms_hip.h, one bit at a time
static std::vector<uint8_t> attach(const std::vector<uint8_t>& payload) {
    uint32_t reg = 0;
    for (uint8_t b : payload) {
        const uint32_t top = ((reg >> (W - 1)) & 1u) ^ b;
        reg = (reg << 1) & ((1u << W) - 1u);
        if (top) reg ^= kPoly;
    }
    std::vector<uint8_t> frame = payload;
    for (int i = 0; i < W; ++i) frame.push_back(static_cast<uint8_t>((reg >> (W - 1 - i)) & 1u));
    return frame;
}
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
static std::vector<std::vector<uint8_t>> random_payloads(uint64_t& seed) {
    std::vector<std::vector<uint8_t>> f(kFrames, std::vector<uint8_t>(kPayload));
    for (auto& frame : f)
        for (auto& b : frame) b = static_cast<uint8_t>(next(seed) >> 40 & 1);
    return f;
}

static void test_attach_feeds_the_encoder() {
    uint64_t seed = 0x243F6A8885A308D3ull;
    const ConvCodeSpec code{T};
    CrcAttachNode att(kCrc);
    ConvEncoderNode enc(code);
    const size_t fin = att.in_frame_bytes(), fout = enc.out_frame_bytes();
    CHECK(fin == 12 && att.out_frame_bytes() == 16 && enc.in_frame_bytes() == 16 && fout == 28);
    CHECK(att.kernel(kFrames).find("crc_attach_kernel") != std::string::npos && att.kernel(kFrames).find("group=4") != std::string::npos);
    PulseBitsNode mod(std::vector<C>(1, C(1.0f, 0.0f)), 1, 2, 0.0, 100.0f);
    NodeSender<std::vector<uint8_t>> src;
    NodeReceiver<std::vector<Complex16>> sink;
    connect_nodes(src, att.input);
    connect_nodes(att.output, enc.input);
    connect_nodes(enc.output, mod.input);
    connect_nodes(mod.output, sink);
    CHECK(att.is_connected() && enc.is_connected() && mod.is_connected());
    const auto payloads = random_payloads(seed);
    std::vector<uint8_t> msg;
    for (const auto& f : payloads) {
        auto rec = pack(f, fin);
        rec[fin - 1] |= 0xF0;                                  // bits 92 ... 95, behind the 76 payload bits: ignored
        rec[fin - 2] |= 0xF0;                                  // bits 84 ... 87 too
        msg.insert(msg.end(), rec.begin(), rec.end());
    }
    for (auto& s : src) CHECK(s.first.send(msg));
    CHECK(att.call().is_ok());
    CHECK(enc.call().is_ok());
    CHECK(mod.call().is_ok());
    const auto got = sink->try_recv();
    CHECK(got.has_value() && got->size() == kFrames * fout * 4);
    if (got && got->size() == kFrames * fout * 4) {
        for (size_t f = 0; f < kFrames; ++f) {
            const auto coded = encode(attach(payloads[f]));
            for (size_t j = 0; j < fout * 4; ++j) {      // symbol j of the record: coded bits 2j (re) and 2j + 1 (im); padding is 0
                const int b0 = 2 * j < kCoded ? coded[2 * j] : 0, b1 = 2 * j + 1 < kCoded ? coded[2 * j + 1] : 0;
                const Complex16 v = (*got)[f * fout * 4 + j];
                CHECK(v.real() == (b0 ? -100 : 100) && v.imag() == (b1 ? -100 : 100));
            }
        }
    }
    // the records themselves, and device-resident messages give the same records as the host-vector node
    const auto host = CrcAttachNode(kCrc).run(msg);
    CHECK(host.is_ok());
    if (host.is_ok())
        for (size_t f = 0; f < kFrames; ++f) CHECK(std::memcmp(host.value().data() + 16 * f, pack(attach(payloads[f]), 16).data(), 16) == 0);
    CrcAttachNodeDev dev(kCrc);
    const auto out = dev.run(DeviceBuf<uint8_t>::from_host(msg));
    CHECK(out.is_ok());
    if (out.is_ok() && host.is_ok()) CHECK(out.value().to_host() == host.value());
    CHECK(CrcAttachNode(kCrc).run(std::vector<uint8_t>(fin + 1)).is_err());   // not whole records
    bool threw = false;
    try {
        CrcAttachNode bad(CrcSpec{33, kPoly, 0, 0, kPayload});
    } catch (const std::exception&) {
        threw = true;
    }
    CHECK(threw);
}

static std::vector<uint8_t> bytes_of(const std::vector<uint8_t>& v) { return v; }
static std::vector<uint8_t> bytes_of(const DeviceBuf<uint8_t>& v) { return v.to_host(); }
static std::vector<int32_t> flags_of(const std::vector<int32_t>& v) { return v; }
static std::vector<int32_t> flags_of(const DeviceBuf<int32_t>& v) { return v.to_host(); }

template <class Deframe, class Decode, class Check, class Msg, class Out>
static void drive(Deframe& deframe, Decode& decode, Check& check, const std::vector<Msg>& msgs, const std::vector<Det>& dets,
                  const std::vector<std::vector<std::vector<uint8_t>>>& sent) {
    NodeSender<Msg> src;
    NodeSender<Det> det_src;
    NodeReceiver<Out> sink;
    connect_nodes(src, deframe.input);
    connect_nodes(det_src, deframe.detections);
    connect_nodes(deframe.output, decode.input);
    connect_nodes(decode.output, check.input);
    connect_nodes(check.output, sink);
    CHECK(deframe.is_connected() && decode.is_connected() && check.is_connected());
    for (size_t i = 0; i < msgs.size(); ++i) {
        for (auto& s : src) CHECK(s.first.send(msgs[i]));
        for (auto& s : det_src) CHECK(s.first.send(dets[i]));
        CHECK(deframe.call().is_ok());
        CHECK(decode.call().is_ok());
        CHECK(check.call().is_ok());
        const std::optional<Out> d = sink->try_recv();
        CHECK(d.has_value());
        if (!d) continue;
        CHECK(d->size() == kFrames && d->frames.frame_bytes == 12);
        const auto data = bytes_of(d->frames.data);
        const auto passed = flags_of(d->passed);
        CHECK(data.size() >= kFrames * 12 && passed.size() >= kFrames);
        for (size_t f = 0; f < kFrames && data.size() >= kFrames * 12 && passed.size() >= kFrames; ++f) {
            CHECK(d->frames.headers[f].index == dets[i][f].index);
            CHECK(passed[f] == (f == kBadFrame ? 0 : 1));
            const auto want = pack(sent[i][f], 12);           // the payload comes back stripped, good frame or bad
            CHECK(std::memcmp(data.data() + f * 12, want.data(), 12) == 0);
        }
    }
}

static void test_decoder_feeds_the_check() {
    uint64_t seed = 0x13198A2E03707344ull;
    constexpr size_t kPay = kCoded / 2, kGap = 5, kMsgs = 2;
    std::vector<std::vector<C>> msgs;
    std::vector<Det> dets;
    std::vector<std::vector<std::vector<uint8_t>>> sent;
    uint64_t index = 0;
    for (size_t m = 0; m < kMsgs; ++m) {
        std::vector<C> y;
        Det det;
        sent.push_back(random_payloads(seed));
        for (size_t f = 0; f < kFrames; ++f) {
            auto frame = attach(sent[m][f]);
            if (f == kBadFrame) frame[kPayload + 5 + m] ^= 1;    // a frame that was sent with a wrong CRC bit: decodes, and fails
            const auto coded = encode(frame);
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
        CrcCheckNode check(kCrc);
        CHECK(check.in_frame_bytes() == decode.out_frame_bytes() && check.out_frame_bytes() == 12);
        CHECK(check.kernel(kFrames).find("crc_check_kernel") != std::string::npos && check.kernel(kFrames).find("width=24") != std::string::npos);
        drive<DeframeNode, ViterbiNode, CrcCheckNode, std::vector<C>, CrcCheckOp::Checked>(deframe, decode, check, msgs, dets, sent);
        CrcCheckOp::Frames wrong{std::vector<uint8_t>(8), {}, 8};   // records of another size
        CHECK(CrcCheckNode(kCrc).run(wrong).is_err());
        CrcCheckOp::Frames none{{}, {}, check.in_frame_bytes()};    // no frames: passes through empty
        const auto empty = CrcCheckNode(kCrc).run(none);
        CHECK(empty.is_ok() && empty.value().size() == 0 && empty.value().passed.empty());
    }
    {  // device-resident messages
        std::vector<DeviceBuf<C>> dmsgs;
        for (auto& m : msgs) dmsgs.push_back(DeviceBuf<C>::from_host(m));
        DeframeNodeDev deframe(kPay, 0, 0, 2, COMMS_SYM_LLR);
        ViterbiNodeDev decode(code, 0, 8.0f);
        CrcCheckNodeDev check(kCrc);
        drive<DeframeNodeDev, ViterbiNodeDev, CrcCheckNodeDev, DeviceBuf<C>, CrcCheckOp::CheckedDev>(deframe, decode, check, dmsgs, dets, sent);
    }
    bool threw = false;
    try {
        CrcCheckNode bad(CrcSpec{8, 0x107, 0, 0, kPayload});   // poly does not fit the width
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
    test_attach_feeds_the_encoder();
    test_decoder_feeds_the_check();
    if (g_fail) {
        std::fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    std::puts("host GPU crc node tests: all passed");
    return 0;
}
