// devmath.hpp -- two small device functions that several kernel files need, one definition each: the finite test and the
// bisection in an ascending array.  (The reduction orders are wave.hpp's.)
#pragma once
#include <cfloat>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace beatamd {

// finite: false for +-inf and for NaN
__device__ __forceinline__ bool is_finite(double x) { return fabs(x) <= DBL_MAX; }

// first index with s[i] >= x (right: s[i] > x) in the ascending s [n]
__device__ __forceinline__ int64_t sorted_bound(const double *s, int64_t n, double x, bool right)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t m = lo + ((hi - lo) >> 1);
        const double v = s[m];
        if (right ? v <= x : v < x) lo = m + 1;
        else hi = m;
    }
    return lo;
}

}  // namespace beatamd
