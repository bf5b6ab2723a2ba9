// roots.hpp -- the twiddle tables of the FFT and overlap-save nodes: roots of unity computed in f64 on the host and
// rounded once to f32.  Host code without HIP headers (tests/fft_plan_test.cpp builds it with g++): `C` is any
// {float x, y} pair -- float2 in the library.
#pragma once

#include <cmath>
#include <cstddef>
#include <vector>

namespace comms {

// e^{-2 pi i e / denom}: the forward sign.  The angle is taken of e mod denom, so it stays below one turn however
// large the exponent product is.
template <class C>
inline C root(unsigned long long e, unsigned long long denom) {
    const double a = -2.0 * 3.14159265358979323846264338327950288 * static_cast<double>(e % denom) / static_cast<double>(denom);
    return C{static_cast<float>(std::cos(a)), static_cast<float>(std::sin(a))};
}
// e^{+2 pi i e / denom}: the conjugate, bit for bit what the positive angle gives (cos is even, sin is odd)
template <class C>
inline C root_conj(unsigned long long e, unsigned long long denom) {
    const C w = root<C>(e, denom);
    return C{w.x, -w.y};
}

// table[m] = W_denom^{m * mult}, m < count; padded with ones up to `size` entries where the kernel's table is longer
template <class C>
inline std::vector<C> roots(size_t count, size_t denom, size_t mult = 1, size_t size = 0) {
    std::vector<C> t(size > count ? size : count, C{1.f, 0.f});
    for (size_t m = 0; m < count; ++m) t[m] = root<C>(static_cast<unsigned long long>(m) * mult, denom);
    return t;
}
// table[r * cols + c] = W_denom^{r * c * scale}: a stage's twiddles by (butterfly output, lane); padded like roots()
template <class C>
inline std::vector<C> root_grid(size_t rows, size_t cols, size_t denom, size_t scale = 1, size_t size = 0) {
    std::vector<C> t(size > rows * cols ? size : rows * cols, C{1.f, 0.f});
    for (size_t r = 0; r < rows; ++r)
        for (size_t c = 0; c < cols; ++c) t[r * cols + c] = root<C>(static_cast<unsigned long long>(r) * c * scale, denom);
    return t;
}

}  // namespace comms
