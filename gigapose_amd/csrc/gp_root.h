// The correctly rounded float64 square root of the side libraries, written ONCE: distance/gpd_dist.hip (ADD / ADD-S distances)
// shade/gpl_shade.hip (vertex normals, Lambert's cosine), label/gpa_label.hip and appear/gpp_appear.hip (LayerNorm, the descriptor's norm) include it.  include/gigapose_dist.h states the construction and why
// it is exact: the compiler's root, its two neighbours, and two explicit fma() calls -- which stay fused under
// -ffp-contract=off and are the one fused operation of each library.  numpy.sqrt returns the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace {

__device__ __forceinline__ double root(double x)
{
    if (!(x > 0.0 && x < (double)INFINITY)) return sqrt(x);
    const bool small = x < 0x1p-500;
    const double xs = small ? x * 0x1p512 : x;
    double r = sqrt(xs);
    const double lo = __longlong_as_double(__double_as_longlong(r) - 1), hi = __longlong_as_double(__double_as_longlong(r) + 1);
    if (fma(lo, r, -xs) >= 0.0) r = lo;
    else if (fma(r, hi, -xs) < 0.0) r = hi;
    return small ? r * 0x1p-256 : r;
}

}  // namespace
