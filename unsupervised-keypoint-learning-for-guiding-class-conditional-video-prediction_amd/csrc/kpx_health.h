// One lane's running statistics of gradient values: the ONE definition shared by the health pass over a whole bucket (guard.hip) and the
// per-variable pass (grad_stats.hip), whose sums are compared with each other.
#pragma once
#include "kpx_common.h"

struct HealthAcc {
    double s;
    float mx;
    unsigned bad;
};
__device__ __forceinline__ void health_add(HealthAcc& a, float x) {
    if ((__float_as_uint(x) & 0x7f800000u) == 0x7f800000u) {     // exponent all ones: NaN or +-Inf
        a.bad += 1u;
    } else {
        const double d = (double)x;                               // exact; d*d is exact in fp64 (24-bit significand): the addition alone rounds
        a.s = fma(d, d, a.s);
        a.mx = fmaxf(a.mx, fabsf(x));
    }
}
