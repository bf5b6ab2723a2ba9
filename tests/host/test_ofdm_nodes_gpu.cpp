// GPU test of the OFDM modulator and demodulator nodes, through the host-vector and the device-resident shells, against a
// direct O(N^2) DFT in double precision that restates include/comms_hip.h's definition in this file.
//   1. OfdmModNode over an 802.11a-like format (N = 64, CP = 16, 48 data carriers, 4 pilots with a polarity sequence, 2 training
//      symbols, 3 data symbols, 3 frames): every symbol within 1e-5 of the definition in the 2-norm, the prefix a copy of the
//      symbol's tail; OfdmModNodeDev gives the same bytes.
//   2. source -> OfdmModNode -> OfdmDemodNode -> sink as a graph: the data values come back within the same bound (the training
//      symbols see a flat channel, so H_k = N tx_scale); OfdmDemodNodeDev gives the same bytes.
//   3. the two training symbols of every frame multiplied by different gains: H_k is their mean, so the data values come back
//      divided by the mean gain -- which a sum that takes one training symbol twice does not give.
// Needs an MI355X (libcomms_hip has no CPU fallback).
#include <algorithm>
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

constexpr int N = 64, CP = 16;
constexpr size_t T = 2, S = 3, kFrames = 3, D = 48, SYM = N + CP, kFrame = (T + S) * SYM;
constexpr double kBound = 1e-5, kPi = 3.14159265358979323846;
static const float kPol[2] = {1.0f, -1.0f};

static OfdmSpec make_spec() {
    OfdmSpec f{N, CP, std::vector<uint8_t>(N, COMMS_OFDM_NULL)};
    for (int k = -26; k <= 26; ++k)
        if (k) f.carrier_kind[(k + N) % N] = (k == 7 || k == -7 || k == 21 || k == -21) ? COMMS_OFDM_PILOT : COMMS_OFDM_DATA;
    f.pilots = {C(1, 0), C(0, 1), C(-1, 0), C(0, -1)};
    f.polarity = {kPol[0], kPol[1]};
    f.train.resize(N);
    for (int k = 0; k < N; ++k) f.train[k] = C(k % 2 ? 1.0f : -1.0f, 0.0f);
    f.n_train = T;
    f.n_syms = S;
    return f;
}

// x[n] = scale * sum_k X_k e^{+2 pi i k n / N}, the prefix in front
static std::vector<Z> symbol_of(const std::vector<Z>& X, double scale) {
    std::vector<Z> x(SYM);
    for (int n = 0; n < N; ++n) {
        Z a = 0;
        for (int k = 0; k < N; ++k) a += X[k] * std::polar(1.0, 2.0 * kPi * ((k * n) % N) / N);
        x[CP + n] = scale * a;
    }
    for (int n = 0; n < CP; ++n) x[n] = x[N + n];
    return x;
}

static double rel_err(const C* got, const std::vector<Z>& want) {
    double num = 0, den = 0;
    for (size_t i = 0; i < want.size(); ++i) {
        num += std::norm(Z(got[i].real(), got[i].imag()) - want[i]);
        den += std::norm(want[i]);
    }
    return std::sqrt(num / den);
}

int main() {
    int32_t n_dev = 0;
    if (comms_device_count(&n_dev) != COMMS_OK || n_dev < 1) {
        std::fprintf(stderr, "no MI355X visible\n");
        return 1;
    }
    const OfdmSpec spec = make_spec();
    const double scale = static_cast<double>(static_cast<float>(1.0 / std::sqrt(static_cast<double>(N))));
    uint64_t seed = 0xA4093822299F31D0ull;
    std::vector<C> data(kFrames * S * D);
    for (auto& v : data) v = C(unit(seed), unit(seed));

    // 1. the modulator
    OfdmModNode mod(spec);
    CHECK(mod.data_syms() == S * D && mod.frame_samples() == kFrame);
    CHECK(mod.kernel(kFrames).find("ofdm_mod_kernel<64>") != std::string::npos);
    OfdmDemodNode dem(spec);
    CHECK(dem.kernel(kFrames).find("ofdm_demod_kernel<64>") != std::string::npos);
    NodeSender<std::vector<C>> src;
    NodeReceiver<std::vector<C>> sink;
    connect_nodes(src, mod.input);
    connect_nodes(mod.output, dem.input);
    connect_nodes(dem.output, sink);
    CHECK(mod.is_connected() && dem.is_connected());
    for (auto& s : src) CHECK(s.first.send(data));
    CHECK(mod.call().is_ok());
    const auto tx_run = OfdmModNode(spec).run(data);
    CHECK(tx_run.is_ok() && tx_run.value().size() == kFrames * kFrame);
    if (!tx_run.is_ok() || tx_run.value().size() != kFrames * kFrame) return 1;
    const std::vector<C>* tx = &tx_run.value();
    double worst = 0;
    for (size_t f = 0; f < kFrames; ++f)
        for (size_t s = 0; s < T + S; ++s) {
            std::vector<Z> X(N, Z(0, 0));
            size_t d = 0, q = 0;
            for (int k = 0; k < N; ++k) {
                if (s < T)
                    X[k] = Z(spec.train[k].real(), spec.train[k].imag());
                else if (spec.carrier_kind[k] == COMMS_OFDM_DATA) {
                    const C v = data[(f * S + (s - T)) * D + d++];
                    X[k] = Z(v.real(), v.imag());
                } else if (spec.carrier_kind[k] == COMMS_OFDM_PILOT) {
                    const C v = spec.pilots[q++];
                    X[k] = Z(v.real(), v.imag()) * static_cast<double>(kPol[(s - T) % 2]);
                }
            }
            const C* got = tx->data() + (f * (T + S) + s) * SYM;
            const double e = rel_err(got, symbol_of(X, scale));
            worst = e > worst ? e : worst;
            CHECK(e <= kBound);
            CHECK(std::memcmp(got, got + N, CP * sizeof(C)) == 0);
        }
    std::printf("modulator: worst symbol %.3e\n", worst);
    OfdmModNodeDev mod_dev(spec);
    const auto tx_dev = mod_dev.run(DeviceBuf<C>::from_host(data));
    CHECK(tx_dev.is_ok());
    if (tx_dev.is_ok()) CHECK(tx_dev.value().to_host() == *tx);

    // 2. the demodulator behind it
    CHECK(dem.call().is_ok());
    const auto back = sink->try_recv();
    CHECK(back.has_value() && back->size() == data.size());
    if (!back || back->size() != data.size()) return 1;
    worst = 0;
    for (size_t i = 0; i < kFrames * S; ++i) {
        std::vector<Z> want(D);
        for (size_t d = 0; d < D; ++d) want[d] = Z(data[i * D + d].real(), data[i * D + d].imag());
        const double e = rel_err(back->data() + i * D, want);
        worst = e > worst ? e : worst;
        CHECK(e <= kBound);
    }
    std::printf("mod -> demod: worst symbol %.3e\n", worst);
    OfdmDemodNodeDev dem_dev(spec);
    if (tx_dev.is_ok()) {
        const auto back_dev = dem_dev.run(tx_dev.value());
        CHECK(back_dev.is_ok());
        if (back_dev.is_ok()) CHECK(back_dev.value().to_host() == *back);
    }
    // 3. training symbols that differ: symbol t of every frame times g_t, so H_k = N tx_scale (g_0 + g_1) / 2 and the data values
    //    come back divided by the mean gain (a sum that takes one of the two symbols twice gives 1 / g_0 or 1 / g_1 instead)
    const Z gain[T] = {Z(1.3, 0.0), Z(1.0, 0.0) + 0.3 * std::polar(1.0, 2.4)};
    std::vector<C> rx = *tx;
    for (size_t f = 0; f < kFrames; ++f)
        for (size_t t = 0; t < T; ++t)
            for (size_t n = 0; n < SYM; ++n) {
                C& v = rx[(f * (T + S) + t) * SYM + n];
                const Z w = Z(v.real(), v.imag()) * gain[t];
                v = C(static_cast<float>(w.real()), static_cast<float>(w.imag()));
            }
    const auto eq = OfdmDemodNode(spec).run(rx);
    CHECK(eq.is_ok() && eq.value().size() == data.size());
    if (!eq.is_ok() || eq.value().size() != data.size()) return 1;
    const Z mean = (gain[0] + gain[1]) / 2.0;
    worst = 0;
    double twice = 1e9;   // how far the answer of a sum that takes one symbol twice would be
    for (size_t i = 0; i < kFrames * S; ++i) {
        std::vector<Z> want(D), w0(D), w1(D);
        for (size_t d = 0; d < D; ++d) {
            const Z v(data[i * D + d].real(), data[i * D + d].imag());
            want[d] = v / mean;
            w0[d] = v / gain[0];
            w1[d] = v / gain[1];
        }
        const double e = rel_err(eq.value().data() + i * D, want);
        worst = e > worst ? e : worst;
        CHECK(e <= kBound);
        twice = std::min(twice, std::min(rel_err(eq.value().data() + i * D, w0), rel_err(eq.value().data() + i * D, w1)));
    }
    std::printf("distinct training symbols: worst symbol %.3e (one symbol taken twice: %.3e)\n", worst, twice);
    CHECK(twice >= 1e4 * kBound);
    CHECK(OfdmModNode(spec).run(std::vector<C>(S * D + 1)).is_err());   // not whole records
    bool threw = false;
    try {
        OfdmSpec bad = spec;
        bad.n_cp = N + 1;
        OfdmModNode node(bad);
    } catch (const std::exception&) {
        threw = true;
    }
    CHECK(threw);
    if (g_fail) {
        std::fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    std::puts("host GPU ofdm node tests: all passed");
    return 0;
}
