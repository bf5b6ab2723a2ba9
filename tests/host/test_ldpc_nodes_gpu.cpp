// GPU test of the LDPC nodes in graphs.
//   1. source -> LdpcEncoderNode -> PulseBitsNode -> sink: the coded records go into the bit-input modulator as they stand, and
//      the symbols are the QPSK points of the coded bits of the header's rule worked out here bit by bit; every codeword
//      satisfies every check of the base matrix.
//   2. sources -> DeframeNode (COMMS_SYM_LLR) -> LdpcDecoderNode -> sink, host vectors and device-resident messages: coded QPSK
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

// a (4, 8, 16) code of the encoder's form: three entries per information column, s = 5 in rows 0 and 3, t = 9 in row r = 2
constexpr int kMb = 4, kNb = 8, kZ = 16, kKb = kNb - kMb, kR = 2, kS = 5, kT = 9;
constexpr size_t T = kKb * kZ, kCoded = kNb * kZ, kFrames = 3;   // 64 information bits, 128 coded bits: 64 QPSK symbols

static LdpcCodeSpec code_spec() {
    std::vector<int16_t> b(kMb * kNb, -1);
    for (int j = 0; j < kKb; ++j)
        for (int k = 0; k < 3; ++k) {
            const int i = (j + k) % kMb;
            b[i * kNb + j] = static_cast<int16_t>((3 * j + 5 * i + 1) % kZ);
        }
    b[0 * kNb + kKb] = b[(kMb - 1) * kNb + kKb] = kS;
    b[kR * kNb + kKb] = kT;
    for (int i = 0; i + 1 < kMb; ++i) b[i * kNb + kKb + 1 + i] = b[(i + 1) * kNb + kKb + 1 + i] = 0;
    return LdpcCodeSpec{kMb, kNb, kZ, b};
}

// the encoding rule of include/comms_hip.h, one bit at a time
static std::vector<uint8_t> encode(const std::vector<uint8_t>& u) {
    const auto base = code_spec().base;
    uint8_t lam[kMb][kZ] = {}, p[kMb][kZ] = {};
    for (int i = 0; i < kMb; ++i)
        for (int z = 0; z < kZ; ++z)
            for (int j = 0; j < kKb; ++j)
                if (base[i * kNb + j] >= 0) lam[i][z] ^= u[j * kZ + (z + base[i * kNb + j]) % kZ];
    for (int z = 0; z < kZ; ++z)
        for (int i = 0; i < kMb; ++i) p[0][(z + kT) % kZ] ^= lam[i][z];
    for (int z = 0; z < kZ; ++z) p[1][z] = lam[0][z] ^ p[0][(z + kS) % kZ];
    for (int i = 1; i + 1 < kMb; ++i)
        for (int z = 0; z < kZ; ++z) p[i + 1][z] = lam[i][z] ^ p[i][z] ^ (i == kR ? p[0][(z + kT) % kZ] : 0);
    std::vector<uint8_t> coded(u);
    for (int i = 0; i < kMb; ++i) coded.insert(coded.end(), p[i], p[i] + kZ);
    return coded;
}
// every check of the base matrix on a coded frame
static bool checks_hold(const std::vector<uint8_t>& c) {
    const auto base = code_spec().base;
    for (int i = 0; i < kMb; ++i)
        for (int z = 0; z < kZ; ++z) {
            int sum = 0;
            for (int j = 0; j < kNb; ++j)
                if (base[i * kNb + j] >= 0) sum ^= c[j * kZ + (z + base[i * kNb + j]) % kZ];
            if (sum) return false;
        }
    return true;
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
    const LdpcCodeSpec code = code_spec();
    LdpcEncoderNode enc(code);
    const size_t fin = enc.in_frame_bytes(), fout = enc.out_frame_bytes();
    CHECK(fin == 8 && fout == 16);
    CHECK(enc.kernel(kFrames).find("ldpc_encode_kernel") != std::string::npos);
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
            CHECK(coded.size() == kCoded && checks_hold(coded));
            for (size_t j = 0; j < fout * 4; ++j) {      // symbol j of the record: coded bits 2j (re) and 2j + 1 (im)
                const Complex16 v = (*got)[f * fout * 4 + j];
                CHECK(v.real() == (coded[2 * j] ? -100 : 100) && v.imag() == (coded[2 * j + 1] ? -100 : 100));
            }
        }
    }
    // device-resident messages give the same records as the host-vector node
    LdpcEncoderNodeDev dev(code);
    const auto out = dev.run(DeviceBuf<uint8_t>::from_host(msg));
    const auto host = LdpcEncoderNode(code).run(msg);
    CHECK(out.is_ok() && host.is_ok());
    if (out.is_ok() && host.is_ok()) CHECK(out.value().to_host() == host.value());
    CHECK(LdpcEncoderNode(code).run(std::vector<uint8_t>(fin + 1)).is_err());   // not whole records
    bool threw = false;
    try {
        LdpcCodeSpec bad = code;
        bad.base[0 * kNb + kKb + 1] = 1;             // a shift on the double diagonal
        LdpcEncoderNode node(bad);
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
        CHECK(d->size() == kFrames && d->frame_bytes == 8);
        const auto data = bytes_of(d->data);
        CHECK(data.size() >= d->size() * d->frame_bytes);
        for (size_t f = 0; f < d->size() && data.size() >= d->size() * d->frame_bytes; ++f) {
            CHECK(d->headers[f].index == dets[i][f].index);
            const auto want = pack(sent[i][f], 8);
            CHECK(std::memcmp(data.data() + f * 8, want.data(), 8) == 0);
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
            for (size_t e = 0; e < 3; ++e) {             // coded bits 10, 50 and 90 wrong: one iteration corrects them
                C& v = y[y.size() - kPay + 5 + 20 * e];
                v = C(-v.real(), v.imag());
            }
            for (size_t j = 0; j < kGap; ++j) y.push_back(C(0.3f, -0.7f));
        }
        index += y.size();
        msgs.push_back(std::move(y));
        dets.push_back(std::move(det));
    }
    const LdpcCodeSpec code = code_spec();
    LdpcDecSpec dec;
    dec.qscale = 8.0f;
    {  // host vectors
        DeframeNode deframe(kPay, 0, 0, 2, COMMS_SYM_LLR);
        LdpcDecoderNode decode(code, dec);
        CHECK(decode.in_frame_bytes() == deframe.frame_bytes() && decode.out_frame_bytes() == 8);
        CHECK(decode.kernel(kFrames).find("ldpc_decode_kernel") != std::string::npos);
        CHECK(decode.kernel(kFrames).find("Z=16") != std::string::npos);
        drive<DeframeNode, LdpcDecoderNode, std::vector<C>, LdpcDecOp::Frames>(deframe, decode, msgs, dets, sent);
        // the hard decisions of the same records are wrong: the decoder did the work
        DeframeNode hard(kPay, 0, 0, 2, COMMS_SYM_BITS);
        const auto rec = hard.run(msgs[0], dets[0]);
        CHECK(rec.is_ok());
        if (rec.is_ok()) CHECK(std::memcmp(rec.value().data.data(), pack(encode(sent[0][0]), rec.value().frame_bytes).data(), rec.value().frame_bytes) != 0);
        LdpcDecOp::Frames wrong{std::vector<uint8_t>(8), {}, 8};   // records of another size
        CHECK(LdpcDecoderNode(code).run(wrong).is_err());
    }
    {  // device-resident messages
        std::vector<DeviceBuf<C>> dmsgs;
        for (auto& m : msgs) dmsgs.push_back(DeviceBuf<C>::from_host(m));
        DeframeNodeDev deframe(kPay, 0, 0, 2, COMMS_SYM_LLR);
        LdpcDecoderNodeDev decode(code, dec);
        drive<DeframeNodeDev, LdpcDecoderNodeDev, DeviceBuf<C>, LdpcDecOp::FramesDev>(deframe, decode, dmsgs, dets, sent);
    }
    bool threw = false;
    try {
        LdpcDecSpec bad;
        bad.record_llrs = 3;                             // fewer values per record than N
        LdpcDecoderNode node(code, bad);
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
    std::puts("host GPU ldpc node tests: all passed");
    return 0;
}
