// GPU test of the symbol mapper and soft demapper nodes, both through the host-vector and the device-resident shells, against a
// bit-serial restatement of include/comms_hip.h's definitions in this file.
//   1. source -> SymbolMapNode -> sink over 64-QAM (6-bit fields straddle the 32-bit words) with a word and a gap, dirty padding
//      bits in the records; SymbolMapNodeDev gives the same symbols.
//   2. DemapNode / DemapNodeDev on frame messages as DeframeNode sends them (COMMS_SYM_C32 records under headers): hard bits
//      and max-log LLRs equal the brute force over all 64 points, float for float, for the per-axis form and the forced table
//      form; the mapper's own symbols come back as the bits that went in.
// Needs an MI355X (libcomms_hip has no CPU fallback).
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

static uint64_t next(uint64_t& s) {  // xorshift
    s ^= s << 13;
    s ^= s >> 7;
    s ^= s << 17;
    return s;
}

constexpr int M = 6;
constexpr size_t kBits = 100, kPay = (kBits + M - 1) / M, kGap = 2, kFrames = 3;   // 17 payload symbols, the last holds 4 bits
static const std::vector<C> kWord = {C(7.0f, 0.0f), C(-7.0f, 0.0f), C(0.0f, 7.0f)};
constexpr size_t kRec = 3 + kPay + kGap;

// the table of include/comms_hip.h: Gray rank per axis, level = (2^k - 1 - 2 rank) * scale
static unsigned gray_rank(unsigned g) {
    unsigned r = 0;
    for (; g; g >>= 1) r ^= g;
    return r;
}
static std::vector<C> table64() {
    std::vector<C> t(64);
    for (unsigned v = 0; v < 64; ++v) t[v] = C(7.0f - 2.0f * gray_rank(v & 7u), 7.0f - 2.0f * gray_rank(v >> 3));
    return t;
}
static std::vector<uint8_t> pack(const std::vector<uint8_t>& bits, size_t record) {
    std::vector<uint8_t> out(record, 0);
    for (size_t i = 0; i < bits.size(); ++i) out[i / 8] = static_cast<uint8_t>(out[i / 8] | (bits[i] << (i % 8)));
    return out;
}
// d_i of the definition: every operation rounded on its own
static float dist(C z, C c) {
    volatile float dx = z.real() - c.real(), dy = z.imag() - c.imag();
    volatile float xx = dx * dx, yy = dy * dy;
    return xx + yy;
}
static unsigned decide(C z, const std::vector<C>& t) {
    unsigned v = 0;
    float best = dist(z, t[0]);
    for (unsigned i = 1; i < t.size(); ++i) {
        const float d = dist(z, t[i]);
        if (d < best) {
            best = d;
            v = i;
        }
    }
    return v;
}
static float llr(C z, const std::vector<C>& t, int b, float s) {
    float d0 = 0, d1 = 0;
    bool h0 = false, h1 = false;
    for (unsigned i = 0; i < t.size(); ++i) {
        const float d = dist(z, t[i]);
        if ((i >> b) & 1u) {
            if (!h1 || d < d1) d1 = d;
            h1 = true;
        } else {
            if (!h0 || d < d0) d0 = d;
            h0 = true;
        }
    }
    volatile float diff = d1 - d0;
    return s * diff;
}

static std::vector<uint8_t> bytes_of(const std::vector<uint8_t>& v) { return v; }
static std::vector<uint8_t> bytes_of(const DeviceBuf<uint8_t>& v) { return v.to_host(); }

static std::vector<std::vector<uint8_t>> g_bits;   // what test 1 mapped
static std::vector<C> g_syms;                      // its output

static void test_mapper() {
    uint64_t seed = 0x243F6A8885A308D3ull;
    const SymbolMapSpec spec{M, qam_table(M), kBits, kWord, kGap};
    const auto table = table64();
    CHECK(spec.constellation == table);
    CHECK(psk_table(2, std::sqrt(2.0)) == (std::vector<C>{C(1, 1), C(-1, 1), C(1, -1), C(-1, -1)}));
    SymbolMapNode map(spec);
    const size_t fin = map.in_frame_bytes();
    CHECK(fin == 16 && map.out_frame_syms() == kRec);
    CHECK(map.kernel(kFrames).find("symmap_kernel") != std::string::npos && map.kernel(kFrames).find("bits=6") != std::string::npos);
    NodeSender<std::vector<uint8_t>> src;
    NodeReceiver<std::vector<C>> sink;
    connect_nodes(src, map.input);
    connect_nodes(map.output, sink);
    CHECK(map.is_connected());
    std::vector<uint8_t> msg;
    for (size_t f = 0; f < kFrames; ++f) {
        std::vector<uint8_t> bits(kBits);
        for (auto& b : bits) b = static_cast<uint8_t>(next(seed) >> 40 & 1);
        auto rec = pack(bits, fin);
        rec[fin - 1] |= 0xFF;                                  // bits 120 ... 127, behind the 100 bits of the record: ignored
        rec[12] |= 0xF0;                                       // bits 100 ... 103 too
        msg.insert(msg.end(), rec.begin(), rec.end());
        g_bits.push_back(bits);
    }
    for (auto& s : src) CHECK(s.first.send(msg));
    CHECK(map.call().is_ok());
    const auto got = sink->try_recv();
    CHECK(got.has_value() && got->size() == kFrames * kRec);
    if (!got || got->size() != kFrames * kRec) return;
    for (size_t f = 0; f < kFrames; ++f) {
        const C* rec = got->data() + f * kRec;
        for (size_t j = 0; j < 3; ++j) CHECK(rec[j] == kWord[j]);
        for (size_t j = 0; j < kPay; ++j) {
            unsigned v = 0;
            for (int b = 0; b < M; ++b)
                if (j * M + b < kBits) v |= static_cast<unsigned>(g_bits[f][j * M + b]) << b;
            CHECK(rec[3 + j] == table[v]);
        }
        for (size_t j = 0; j < kGap; ++j) CHECK(rec[3 + kPay + j] == C(0.0f, 0.0f));
    }
    g_syms = *got;
    SymbolMapNodeDev dev(spec);
    const auto out = dev.run(DeviceBuf<uint8_t>::from_host(msg));
    CHECK(out.is_ok());
    if (out.is_ok()) CHECK(out.value().to_host() == *got);
    CHECK(SymbolMapNode(spec).run(std::vector<uint8_t>(fin + 1)).is_err());   // not whole records
    bool threw = false;
    try {
        SymbolMapNode bad(SymbolMapSpec{3, {}, kBits});                      // no default table at 3 bits
    } catch (const std::exception&) {
        threw = true;
    }
    CHECK(threw);
}

template <class Node, class Msg>
static void check_demap(Node& node, const Msg& in, const std::vector<C>& z, int32_t format, float scale) {
    const auto table = table64();
    const auto out = node.run(in);
    CHECK(out.is_ok());
    if (!out.is_ok()) return;
    const auto& d = out.value();
    const size_t fb = format == COMMS_SYM_BITS ? (kPay * M + 31) / 32 * 4 : kPay * M * 4;
    CHECK(d.size() == kFrames && d.frame_bytes == fb && node.out_frame_bytes() == fb);
    const auto data = bytes_of(d.data);
    CHECK(data.size() >= kFrames * fb);
    if (data.size() < kFrames * fb) return;
    for (size_t f = 0; f < kFrames; ++f) {
        CHECK(d.headers[f].index == 1000 * f);
        if (format == COMMS_SYM_BITS) {
            std::vector<uint8_t> bits;
            for (size_t j = 0; j < kPay; ++j)
                for (int b = 0; b < M; ++b) bits.push_back(static_cast<uint8_t>((decide(z[f * kPay + j], table) >> b) & 1u));
            CHECK(std::memcmp(data.data() + f * fb, pack(bits, fb).data(), fb) == 0);
        } else {
            for (size_t j = 0; j < kPay; ++j)
                for (int b = 0; b < M; ++b) {
                    float got, want = llr(z[f * kPay + j], table, b, scale);
                    std::memcpy(&got, data.data() + f * fb + 4 * (j * M + b), 4);
                    CHECK(std::memcmp(&got, &want, 4) == 0);
                }
        }
    }
}

static void test_demapper() {
    uint64_t seed = 0x13198A2E03707344ull;
    const auto table = table64();
    // the mapper's payload symbols, then the same with noise and a few ties (midpoints between points)
    std::vector<C> clean, noisy;
    for (size_t f = 0; f < kFrames; ++f)
        for (size_t j = 0; j < kPay; ++j) {
            const C s = g_syms.size() == kFrames * kRec ? g_syms[f * kRec + 3 + j] : C(0, 0);
            clean.push_back(s);
            const float nr = static_cast<float>(static_cast<int64_t>(next(seed) >> 40) - (1 << 23)) / (1 << 23);
            const float ni = static_cast<float>(static_cast<int64_t>(next(seed) >> 40) - (1 << 23)) / (1 << 23);
            noisy.push_back(j % 5 == 0 ? C(s.real() + 1.0f, s.imag() - 1.0f) : C(s.real() + 1.5f * nr, s.imag() + 1.5f * ni));
        }
    std::vector<comms_deframe_header_t> headers(kFrames);
    for (size_t f = 0; f < kFrames; ++f) headers[f] = comms_deframe_header_t{1000 * f, 1000 * f + 3, 1.0f, 0.0f, 1.0f, 1.0f};
    auto frames_of = [&](const std::vector<C>& z) {
        std::vector<uint8_t> raw(z.size() * sizeof(C));
        std::memcpy(raw.data(), z.data(), raw.size());
        return DemapOp::Frames{raw, headers, kPay * sizeof(C)};
    };
    for (const bool force : {false, true}) {
        for (const int32_t format : {COMMS_SYM_LLR, COMMS_SYM_BITS}) {
            const DemapSpec spec{M, table, kPay, format, 0.75f, force};
            DemapNode host(spec);
            CHECK(host.in_frame_bytes() == kPay * 8);
            CHECK(host.kernel(kFrames).find(force ? "form=table" : "form=axis") != std::string::npos);
            for (const auto* z : {&clean, &noisy}) {
                const auto in = frames_of(*z);
                check_demap(host, in, *z, format, 0.75f);
                DemapNodeDev dev(spec);
                const DemapOp::FramesDev din{DeviceBuf<uint8_t>::from_host(in.data), headers, in.frame_bytes};
                check_demap(dev, din, *z, format, 0.75f);
            }
        }
    }
    // the round trip: the hard bits of the mapper's symbols are the bits that went in, padding zero
    DemapNode back(DemapSpec{M, table, kPay, COMMS_SYM_BITS});
    const auto out = back.run(frames_of(clean));
    CHECK(out.is_ok());
    if (out.is_ok() && g_bits.size() == kFrames)
        for (size_t f = 0; f < kFrames; ++f) CHECK(std::memcmp(out.value().data.data() + f * 16, pack(g_bits[f], 16).data(), 16) == 0);
    DemapOp::Frames wrong{std::vector<uint8_t>(8), {}, 8};   // records of another size
    CHECK(DemapNode(DemapSpec{M, table, kPay}).run(wrong).is_err());
    DemapOp::Frames none{{}, {}, kPay * 8};                  // no frames: passes through empty
    const auto empty = DemapNode(DemapSpec{M, table, kPay}).run(none);
    CHECK(empty.is_ok() && empty.value().size() == 0);
    bool threw = false;
    try {
        DemapNode bad(DemapSpec{9, {}, kPay});
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
    test_mapper();
    test_demapper();
    if (g_fail) {
        std::fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    std::puts("host GPU symmap node tests: all passed");
    return 0;
}
