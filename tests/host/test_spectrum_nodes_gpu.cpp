// GPU test of the spectrum estimator nodes, through the host-vector and the device-resident shells, against a direct O(N^2)
// DFT in double precision that restates include/comms_hip.h's definition in this file, at N = 64.
//   1. source -> SpectrumNode -> sink as a graph over messages of uneven lengths: a message that completes no row sends
//      nothing, the others carry their rows; all rows together within the bound of the definition (the f32 transform's 1e-5,
//      on the power: 2 B + B^2, plus the f32 sums).
//   2. SpectrumNodeDev over the same messages gives the same bytes.
//   3. K = 33 (two launches) in the centred order against the same definition.
// Needs an MI355X (libcomms_hip has no CPU fallback).
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../comms_rs_amd/host/comms/nodes.hpp"

using namespace comms;
using C = Complex32;
using Z = std::complex<double>;

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
static float unit(uint64_t& s) { return static_cast<float>(static_cast<int64_t>(next(s) >> 40) - (1 << 23)) / (1 << 23); }

constexpr int N = 64;
constexpr double kPi = 3.14159265358979323846, kB = 1e-5;

// rows of the whole stream by the definition: scale * sum over the row's K segments of |DFT(w x[s H .. s H + N))|^2
static std::vector<double> rows_of(const std::vector<C>& x, const std::vector<float>& w, size_t H, size_t K, double scale, bool centred) {
    const size_t segs = x.size() >= N ? (x.size() - N) / H + 1 : 0, rows = segs / K;
    std::vector<double> out(rows * N, 0.0);
    for (size_t s = 0; s < rows * K; ++s)
        for (int k = 0; k < N; ++k) {
            Z a = 0;
            for (int n = 0; n < N; ++n) {
                const C v = x[s * H + n];
                a += static_cast<double>(w[n]) * Z(v.real(), v.imag()) * std::polar(1.0, -2.0 * kPi * ((k * n) % N) / N);
            }
            out[(s / K) * N + (centred ? (k + N / 2) % N : k)] += scale * std::norm(a);
        }
    return out;
}

// the row bound of the contract: sum_k |got - P| <= (2 B + B^2 + e) sum_k P, e = (32 + ceil(K / 32) + 3) 2^-24
static void check_rows(const std::vector<float>& got, const std::vector<double>& want, size_t K, const char* what) {
    CHECK(got.size() == want.size());
    if (got.size() != want.size()) return;
    const double e = (32.0 + static_cast<double>((K + 31) / 32) + 3.0) * std::ldexp(1.0, -24);
    double worst = 0;
    for (size_t r = 0; r < want.size() / N; ++r) {
        double num = 0, den = 0;
        for (int k = 0; k < N; ++k) {
            num += std::fabs(static_cast<double>(got[r * N + k]) - want[r * N + k]);
            den += want[r * N + k];
        }
        const double share = num / ((2 * kB + kB * kB + e) * den);
        worst = share > worst ? share : worst;
        CHECK(share <= 1.0);
    }
    std::printf("%s: %zu rows, worst row error / bound %.3f\n", what, want.size() / N, worst);
}

int main() {
    int32_t n_dev = 0;
    if (comms_device_count(&n_dev) != COMMS_OK || n_dev < 1) {
        std::fprintf(stderr, "no MI355X visible\n");
        return 1;
    }
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    const size_t H = 24, K = 3, kLen = N + 40 * H + 11;
    std::vector<C> x(kLen);
    for (size_t t = 0; t < kLen; ++t) {
        const Z tone = 2.0 * std::polar(1.0, 2.0 * kPi * 9.0 / 64.0 * static_cast<double>(t));
        x[t] = C(unit(seed) + static_cast<float>(tone.real()), unit(seed) + static_cast<float>(tone.imag()));
    }
    const std::vector<float> w = SpectrumOp::window(COMMS_WINDOW_HANN, N);
    double e2 = 0;
    for (float v : w) e2 += static_cast<double>(v) * v;
    const double scale = static_cast<double>(static_cast<float>(1.0 / (K * e2)));

    // 1. the vector shell in a graph; the messages: shorter than a segment, inside a row, several rows, the rest
    const size_t cuts[] = {0, 30, 30 + N + 2 * H, 30 + N + 20 * H + 5, kLen};
    SpectrumNode node(N, w, H, K);
    CHECK(node.n_fft() == N);
    CHECK(node.kernel(kLen).find("spectrum_kernel<64,") == 0 && node.kernel(kLen).find("spectrum_rows_kernel") == std::string::npos);
    NodeSender<std::vector<C>> src;
    NodeReceiver<std::vector<float>> sink;
    connect_nodes(src, node.input);
    connect_nodes(node.output, sink);
    CHECK(node.is_connected());
    std::vector<float> all;
    size_t messages = 0;
    for (size_t i = 0; i + 1 < sizeof cuts / sizeof *cuts; ++i) {
        const std::vector<C> part(x.begin() + cuts[i], x.begin() + cuts[i + 1]);
        for (auto& s : src) CHECK(s.first.send(part));
        CHECK(node.call().is_ok());
        const auto got = sink->try_recv();
        if (i == 0) CHECK(!got.has_value());   // 30 samples complete no row: no message
        if (got) {
            CHECK(!got->empty() && got->size() % N == 0);
            all.insert(all.end(), got->begin(), got->end());
            ++messages;
        }
    }
    CHECK(messages == 3);
    const std::vector<double> want = rows_of(x, w, H, K, scale, false);
    CHECK(want.size() == 13 * N);
    check_rows(all, want, K, "SpectrumNode, cut into messages");
    const auto whole = SpectrumNode(N, w, H, K).run(x);
    CHECK(whole.is_ok() && whole.value().has_value() && *whole.value() == all);

    // 2. the device shell: the same bytes
    SpectrumNodeDev dev(N, w, H, K);
    std::vector<float> all_dev;
    for (size_t i = 0; i + 1 < sizeof cuts / sizeof *cuts; ++i) {
        const std::vector<C> part(x.begin() + cuts[i], x.begin() + cuts[i + 1]);
        const auto got = dev.run(DeviceBuf<C>::from_host(part));
        CHECK(got.is_ok());
        if (!got.is_ok()) return 1;
        if (i == 0) CHECK(!got.value().has_value());
        if (got.value()) {
            const std::vector<float> rows = got.value()->to_host();
            all_dev.insert(all_dev.end(), rows.begin(), rows.end());
        }
    }
    CHECK(all_dev.size() == all.size() && std::memcmp(all_dev.data(), all.data(), all.size() * sizeof(float)) == 0);

    // 3. two launches, centred
    const size_t K2 = 33;
    SpectrumNode psd(N, w, 1, K2, 0.0f, COMMS_SPECTRUM_CENTRED);
    CHECK(psd.kernel(kLen).find(" + spectrum_rows_kernel") != std::string::npos);
    const auto rows2 = psd.run(x);
    CHECK(rows2.is_ok() && rows2.value().has_value());
    if (rows2.is_ok() && rows2.value())
        check_rows(*rows2.value(), rows_of(x, w, 1, K2, static_cast<double>(static_cast<float>(1.0 / (K2 * e2))), true), K2, "SpectrumNode, K = 33, centred");

    bool threw = false;
    try {
        SpectrumNode bad(96, std::vector<float>(96, 1.0f), 48);
    } catch (const std::exception&) {
        threw = true;
    }
    CHECK(threw);
    if (g_fail) {
        std::fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    std::puts("host GPU spectrum node tests: all passed");
    return 0;
}
