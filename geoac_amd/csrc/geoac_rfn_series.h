// geoac_rfn_series.h - the elementary functions of include/geoac_refine.h, which is normative for this arithmetic: SIN, COS, SINCOSD, ASIN and
// DIST as series in plain double operations, so that a host restatement gives the same bits (tests/refine_reference.py).  Defined once, for
// geoac_refine.hip (station refinement) and geoac_level_refine.hip (level refinement).  Every product is rounded before it is added, so
// contraction is off from here on in whatever file includes this.
#ifndef GEOAC_RFN_SERIES_H_
#define GEOAC_RFN_SERIES_H_

#include <hip/hip_runtime.h>
#include <math.h>

#include "geoac_tri_rule.h"

#pragma clang fp contract(off)

namespace {

const double kRfnPi = 3.141592653589793238462643;

__device__ inline double rfn_sin(double x){
    const double x2 = x * x;
    double t = x, s = x;
    for(int k = 1; k <= 14; k++){ t = -(t * x2) / (double)((2 * k) * (2 * k + 1)); s = s + t; }
    return s;
}
__device__ inline double rfn_cos(double x){
    const double x2 = x * x;
    double t = 1.0, s = 1.0;
    for(int k = 1; k <= 14; k++){ t = -(t * x2) / (double)((2 * k - 1) * (2 * k)); s = s + t; }
    return s;
}
__device__ inline void rfn_sincosd(double a, double* sn, double* cs){
    const double q = floor(a / 90.0 + 0.5);
    const double r = (a - 90.0 * q) * kRfnPi / 180.0;
    const double n = q - 4.0 * floor(q / 4.0);
    const double s = rfn_sin(r), c = rfn_cos(r);
    if(n == 0.0){ *sn = s; *cs = c; }
    else if(n == 1.0){ *sn = c; *cs = -s; }
    else if(n == 2.0){ *sn = -s; *cs = -c; }
    else { *sn = -c; *cs = s; }
}
__device__ inline double rfn_asin(double s){
    const bool low = s <= 0.5;
    const double u = low ? s : sqrt((1.0 - s) / 2.0);
    const double x2 = u * u;
    double t = u, a = u;
    for(int k = 1; k <= 30; k++){ t = ((t * x2) * (double)((2 * k - 1) * (2 * k - 1))) / (double)((2 * k) * (2 * k + 1)); a = a + t; }
    return low ? a : kRfnPi / 2.0 - 2.0 * a;
}
__device__ inline double rfn_dist(double lat1, double lon1, double lat2, double lon2, double R){
    const double a = rfn_sin(((lat2 - lat1) * kRfnPi / 180.0) / 2.0), b = rfn_sin((wrap180(lon2 - lon1) * kRfnPi / 180.0) / 2.0);
    double h = a * a + (rfn_cos(lat1 * kRfnPi / 180.0) * rfn_cos(lat2 * kRfnPi / 180.0)) * (b * b);
    if(h > 1.0) h = 1.0;
    return (2.0 * R) * rfn_asin(sqrt(h));
}
__device__ inline bool rfn_finite(double v){ return v - v == 0.0; }

// EXP of include/geoac_lampmap.h, which is normative for it (restated in tests/lampmap_reference.py): reduction by multiples of ln 2 with a split
// constant (q * kRfnLn2Hi is exact: 31 significant bits times at most 11), a Horner sum of 14 Taylor terms on |r| <= 0.347, and an exact power of two.
// Below -700 it returns 0.0, so that no result is subnormal (exp(-700) = 9.8e-305); above 700 +inf.
const double kRfnLn2 = 0.693147180559945309417, kRfnLn2Hi = 6.93147180369123816490e-01, kRfnLn2Lo = 1.90821492927058770002e-10;
__device__ inline double rfn_exp(double x){
    if(x != x) return x;
    if(x < -700.0) return 0.0;
    if(x > 700.0) return (double)INFINITY;
    const double q = floor(x / kRfnLn2 + 0.5);                  // |q| <= 1010
    const double r = (x - q * kRfnLn2Hi) - q * kRfnLn2Lo;
    double s = 1.0;
    for(int k = 14; k >= 1; k--) s = 1.0 + (r * s) / (double)k;
    return s * __longlong_as_double((long long)((int)q + 1023) << 52);          // biased exponent 13 .. 2033: a normal power of two
}

}  // namespace

#endif
