// estimate_math.h — the QBER estimator of the reconciliation stage, written
// once for the solve kernel (estimate.hip) and the host entry
// (qldpc_qber_from_weight): the method-of-moments root of
//
//     g(q) = sum over classes c of  N_c * (1 - (1 - 2 q)^d_c) / 2
//
// against a syndrome weight (include/qkd_ldpc_hip.h, "Error estimation at the
// reconciliation stage").
//
// Rules for this file, as in exact_math.h: every operation is a plain IEEE-754
// binary64 add, subtract, multiply or compare (compile with -ffp-contract=off),
// and the evaluation order below is load-bearing: tests/estimate_ref.py restates
// it in Python floats and the results are compared bit for bit.  The one
// division, of log_p, is a true division; log1p is exact_math.h's.
#pragma once

#include "exact_math.h"

namespace ql_exact {

// The degree classes of a graph's informative rows: degree[] ascending and
// distinct, rows[] the row counts.
struct EstClasses {
    int32_t count;
    const int32_t *degree;
    const int32_t *rows;
};

// g(q).  The power (1 - 2 q)^d is carried from class to class by repeated
// multiplication, starting from 1.0; the class terms N_c * (0.5 * (1 - power))
// are added in ascending class order into an accumulator that starts at 0.0.
QL_HD double est_expected_weight(const EstClasses &cl, double q) {
    const double t = 1.0 - 2.0 * q;
    double pw = 1.0, acc = 0.0;
    int32_t d = 0;
    for (int32_t c = 0; c < cl.count; ++c) {
        for (const int32_t dc = cl.degree[c]; d < dc; ++d) pw = pw * t;
        acc = acc + (double)cl.rows[c] * (0.5 * (1.0 - pw));
    }
    return acc;
}

// The q in [q_min, q_max] at which frames * g(q) meets `weight` (frames == 1:
// one frame's weight; F: a sum over F frames).  g rises with q, so the root is
// unique: the clamps first, then a bisection that ends when the midpoint is
// one of its ends, or after 64 steps.  0 < q_min <= q_max < 0.5 and
// frames >= 1 are the caller's to check.
QL_HD double est_qber(const EstClasses &cl, int64_t weight, int64_t frames, double q_min, double q_max) {
    const double k = (double)weight, f = (double)frames;
    if (f * est_expected_weight(cl, q_min) >= k) return q_min;
    if (f * est_expected_weight(cl, q_max) <= k) return q_max;
    double lo = q_min, hi = q_max;
    for (int step = 0; step < 64; ++step) {
        const double mid = 0.5 * (lo + hi);
        if (mid == lo || mid == hi) break;
        if (f * est_expected_weight(cl, mid) < k) lo = mid;
        else hi = mid;
    }
    return 0.5 * (lo + hi);
}

// log((1 - q) / q) as log1p((1 - 2 q) / q): finite and positive for q in (0, 0.5).
QL_HD double est_log_p(double q) { return log1p_exact((1.0 - 2.0 * q) / q); }

}  // namespace ql_exact
