// mbb_rwsteps.hip.h -- the two pieces of step logic importance reweighting adds to mbb_psis.hip.h's, for the device
// and the host (include/mbb_hip.h: "a chain reweighted under another density").  Small functions on plain values so
// that the kernels (mbb_reweight.hip.h) and tests/_reweight_host.cpp run the same text:
//   rw_quantise      u = floor(exp(lw) 2^32 + 1/2) in [0, 2^32]: the integer weight of a log weight lw <= 0
//   rw_target        t = ceil((p / 100) U) clamped to [1, U]: the cumulative weight the quantile at percent p reaches
// With at most MBB_PW_MAX_WINDOW = 1 864 135 entries U = sum u < 2^53 (1 864 135 * 2^32 = 8.006e15 < 9.007e15): U is
// exact as an integer and as a double, and every accumulation of weights is an integer one.
#pragma once
#include "mbb_psis.hip.h"

namespace mbbrws {

constexpr double kTwo32 = 4294967296.0;
constexpr unsigned long long kUnit = 1ull << 32;      // the weight of lw = 0

// the integer weight of a log weight: 0 for -inf and for a NaN, 2^32 from lw = 0 up
PS_HD unsigned long long rw_quantise(double lw)
{
    const double v = floor(exp(lw) * kTwo32 + 0.5);
    if (!(v >= 1.0)) return 0ull;
    return v >= kTwo32 ? kUnit : (unsigned long long)v;
}

// the target of the weighted quantile at percent p of a column of total weight U (0 for U = 0: nothing to select).
// (double) U is exact; the product and the quotient are one rounding each, as the restatement in tests/_reweight_ref.py.
PS_HD unsigned long long rw_target(double p, unsigned long long U)
{
    if (U == 0ull) return 0ull;
    const double t = ceil((p / 100.0) * (double)U);
    if (!(t >= 1.0)) return 1ull;
    return t >= (double)U ? U : (unsigned long long)t;
}

}   // namespace mbbrws
