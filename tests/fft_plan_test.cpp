// Stand-alone run of the FFT node's kernel-selection rule (comms_rs_amd/csrc/fft_plan.hpp) and of the twiddle-table
// builder (comms_rs_amd/csrc/roots.hpp), the only project headers included: built and run by tests/test_fft_cases.py
// under AddressSanitizer and UBSan, no GPU.  usage: fft_plan_test NUM_CU
//
// stdout, tab-separated:
//   const <name> <value>            the rule's batching constants
//   form <section> <n> <label>      the kernels length n runs on; <section> is "default" or "<SELECTOR>=<value>" for each
//                                   selector of the diagnostic build; every n in 1 ... 70000 and 2^k - 1, 2^k, 2^k + 1 up to 2^25
//   roots <checks> <failures>       (each failure on stderr)
// The labels are those of tests/fft_cases.py: family_f32(n) under default knobs.  Exit status 0 = every root check holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "fft_plan.hpp"
#include "roots.hpp"

namespace {

using namespace comms;

struct F2 {
    float x, y;
};

std::string fmt(const char* f, size_t v) {
    char b[64];
    std::snprintf(b, sizeof(b), f, v);
    return b;
}

// "tiny", "rx<N>", "rx32k", "<form>_2p<log>"
std::string pow2_label(size_t n, const FftKnobs& k) {
    const size_t log = static_cast<size_t>(ilog2(n));
    switch (pow2_form(n, k).form) {
        case Pow2Form::Tiny: return "tiny";
        case Pow2Form::Rx: return fmt("rx%zu", n);
        case Pow2Form::Rx32k: return "rx32k";
        case Pow2Form::Cols: return fmt("cols_2p%zu", log);
        case Pow2Form::Fast20: return fmt("fast_2p%zu", log);
        case Pow2Form::Gather: return fmt("gather_2p%zu", log);
        case Pow2Form::Three: return fmt("three_2p%zu", log);
        case Pow2Form::Tile: return fmt("tile_2p%zu", log);
    }
    return "?";
}

std::string label(size_t n, const FftKnobs& k) {
    const FftChoice c = fft_form(n, k);
    switch (c.kind) {
        case FftKind::Refused: return std::string("refused: ") + c.why;
        case FftKind::Copy: return "pow2_copy";
        case FftKind::Pow2: return "pow2_" + pow2_label(n, k);
        case FftKind::DirectSmall: return "direct";
        case FftKind::Direct: return "direct_large";
        case FftKind::BluFused: return fmt("blu_fused_M%zu", c.M);
        case FftKind::BluUnfused: {
            const Pow2Form f = pow2_form(c.M, k).form;
            if (f == Pow2Form::Rx32k) return "blu_rx32k";
            if (f == Pow2Form::Tiny || f == Pow2Form::Rx) return fmt("blu_unfused_rx_M%zu", c.M);
            const std::string p = pow2_label(c.M, k);  // "<form>_2p<log>" -> "blu_<form>_M2p<log>"
            const size_t cut = p.find('_');
            return "blu_" + p.substr(0, cut) + "_M" + p.substr(cut + 1);
        }
    }
    return "?";
}

void print_forms(const char* section, const FftKnobs& k, const std::set<size_t>& lengths) {
    for (size_t n : lengths) std::printf("form\t%s\t%zu\t%s\n", section, n, label(n, k).c_str());
}

// ---- roots ----------------------------------------------------------------------------------------------------------
size_t checks = 0, failures = 0;

void expect(bool ok, const char* what, unsigned long long e, unsigned long long denom) {
    ++checks;
    if (ok) return;
    ++failures;
    std::fprintf(stderr, "FAIL %s: e %llu denom %llu\n", what, e, denom);
}

bool same_bits(F2 a, F2 b) { return std::memcmp(&a, &b, sizeof(F2)) == 0; }

// A component against the long-double value: within one f32 ulp at that value, plus 4e-15 for the f64 angle the table is
// built from (three roundings of at most 2^-53 relative on an angle below 2 pi move it by less than 2.1e-15, and the
// component by no more; at W^{denom/2} that is all there is of the sine).
bool within_ulp(float got, long double want) {
    const float w = std::fabs(static_cast<float>(want));
    const long double ulp = static_cast<long double>(std::nextafterf(w, INFINITY)) - static_cast<long double>(w);
    return std::fabs(static_cast<long double>(got) - want) <= ulp + 4e-15L;
}

void check_roots() {
    const long double pi = 3.14159265358979323846264338327950288L;
    // every exponent of the 1024-, 64-, 256- and 4096-point stage tables (a table holds W^{r c mod denom}: all residues)
    for (unsigned long long denom : {1024ull, 64ull, 256ull, 4096ull})
        for (unsigned long long e = 0; e < denom; ++e) {
            const long double a = -2.0L * pi * static_cast<long double>(e) / static_cast<long double>(denom);
            const F2 w = root<F2>(e, denom);
            expect(within_ulp(w.x, cosl(a)) && within_ulp(w.y, sinl(a)), "root against cosl / sinl", e, denom);
            // e mod denom: the products r * c of a table run far past denom
            for (unsigned long long turns : {1ull, 15ull, 4095ull, 1ull << 40})
                expect(same_bits(root<F2>(e + turns * denom, denom), w), "periodicity", e + turns * denom, denom);
        }
    // e^{+2 pi i e / denom} written with the positive angle (as the rate-8 polyphase tables were) against root_conj, and that
    // angle with the sine negated against root: the same bits, signed zeros included
    for (unsigned long long denom : {64ull, 128ull, 256ull, 1024ull, 4096ull, 16384ull})
        for (unsigned long long e = 0; e < denom; ++e) {
            const double a = 2.0 * 3.14159265358979323846264338327950288 * static_cast<double>(e) / static_cast<double>(denom);
            const F2 plus{static_cast<float>(std::cos(a)), static_cast<float>(+1 * std::sin(a))};
            const F2 minus{static_cast<float>(std::cos(a)), static_cast<float>(-1 * std::sin(a))};
            expect(same_bits(root_conj<F2>(e, denom), plus), "positive angle = conjugate", e, denom);
            expect(same_bits(root<F2>(e, denom), minus), "positive angle, sine negated = root", e, denom);
        }
    // the table builders: entry by entry root(), ones behind
    const std::vector<F2> line = roots<F2>(5, 4096, 64, 8), grid = root_grid<F2>(3, 4, 128, 2, 16);
    expect(line.size() == 8 && grid.size() == 16, "table sizes", 0, 0);
    for (size_t m = 0; m < line.size(); ++m) expect(same_bits(line[m], m < 5 ? root<F2>(m * 64, 4096) : F2{1.f, 0.f}), "roots()", m, 4096);
    for (size_t i = 0; i < grid.size(); ++i)
        expect(same_bits(grid[i], i < 12 ? root<F2>((i / 4) * (i % 4) * 2, 128) : F2{1.f, 0.f}), "root_grid()", i, 128);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: fft_plan_test NUM_CU\n");
        return 2;
    }
    const size_t num_cu = std::strtoul(argv[1], nullptr, 10);
    const FftKnobs dflt;
    std::printf("const\ttile_points\t%zu\n", kRxTilePoints);
    std::printf("const\tblu_chunk_points\t%zu\n", kBluChunkPoints);
    std::printf("const\tblu_max_n\t%zu\n", kBluMaxN);
    std::printf("const\tsmall_dft_grid_cap\t%zu\n", small_dft_grid_cap(num_cu));
    std::printf("const\tsmall_dft_lanes\t%zu\n", kSmallDftLanes);
    std::printf("const\tsmall_dft_max\t%zu\n", kSmallDftMax);
    std::printf("const\tdirect_max\t%zu\n", dflt.direct_max);
    std::printf("const\tdirect_max_cap\t%zu\n", kDirectMaxCap);

    std::set<size_t> lengths;
    for (size_t n = 1; n <= 70000; ++n) lengths.insert(n);
    for (size_t p = 2; p <= (static_cast<size_t>(1) << 25); p <<= 1)
        for (size_t n : {p - 1, p, p + 1}) lengths.insert(n);

    print_forms("default", dflt, lengths);
    FftKnobs k;
    k.no_rx = true;
    print_forms("COMMS_FFT_NO_RX=1", k, lengths);
    k = dflt;
    k.no_rx32k = true;
    print_forms("COMMS_FFT_NO_RX32K=1", k, lengths);
    k = dflt;
    k.no_cols = true;
    print_forms("COMMS_FFT_NO_COLS=1", k, lengths);
    k = dflt;
    k.blu_unfused = true;
    print_forms("COMMS_FFT_BLU_UNFUSED=1", k, lengths);
    k = dflt;
    k.direct_max = 4096;
    print_forms("COMMS_FFT_DIRECT_MAX=4096", k, lengths);

    check_roots();
    std::printf("roots\t%zu\t%zu\n", checks, failures);
    return failures ? 1 : 0;
}
