// zpow.hpp -- Complex<f64> product and integer power of the block estimators (estimators.hip, syncest.hip).
#pragma once

#include <hip/hip_runtime.h>

namespace comms {

__device__ __forceinline__ double2 zmul(double2 a, double2 b) {
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
// Complex::powi(exp >= 0): exponentiation by squaring in num_traits::pow's operation order
__device__ __forceinline__ double2 zpowi(double2 base, unsigned exp) {
    if (exp == 0) return make_double2(1.0, 0.0);
    while ((exp & 1) == 0) {
        base = zmul(base, base);
        exp >>= 1;
    }
    if (exp == 1) return base;
    double2 acc = base;
    while (exp > 1) {
        exp >>= 1;
        base = zmul(base, base);
        if (exp & 1) acc = zmul(acc, base);
    }
    return acc;
}

}  // namespace comms
