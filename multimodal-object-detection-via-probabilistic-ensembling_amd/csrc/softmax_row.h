// The float64 softmax of one row of K+1 float32 logits at a temperature: the one definition behind the pack kernel (csrc/pack.hip) and the
// flat softmax (csrc/calibrate.hip), so a row gets the same bits from either.
//
// z_k = (double)logit_k / T, m = max_k z_k, e_k = exp(z_k - m), p_k = e_k / sum_j e_j.  For K+1 <= 64 a row is held by a power-of-two
// group of lanes, one column per lane, and max and sum are xor-butterflies over the group: every lane of the group ends with the same
// bits (a + b == b + a at every level), the logits of the group's rows are read coalesced and 64 / G rows are in flight per wavefront.
// Above 64 columns a lane walks its row serially.  Nothing is clamped: a NaN or +inf logit (or a row of -inf) gives NaN probabilities
// like the float64 NumPy expression.  Both users are built with -ffp-contract=off.
// The log-posterior (LOGP) reuses z, m and the sum s of the same call: log p_k = (z_k - m) - log(s), finite for every finite logit
// (s is in [1, K+1]), where log(p_k) is -inf once p_k underflows and log(1 - sum p) is NaN on a saturated row.
#pragma once
#include "common.h"

namespace pe {

constexpr double kNegInf = -__builtin_huge_val();

__host__ __device__ __forceinline__ int group_width(int k1) {   // smallest power of two >= k1 (k1 <= 64)
    int g = 1;
    while (g < k1) g <<= 1;
    return g;
}

// One column of one row per lane; `row` = the row's K+1 logits (ignored when !live), col = lane % G.  Every lane of the wavefront
// calls this (the shuffles are wave-wide).  Returns p_col (0 on the padding lanes col >= k1); LOGP: *lp = log p_col.
template <bool LOGP = false>
__device__ __forceinline__ double softmax_group(const float* row, bool live, int col, int k1, int G, double T, double* lp = nullptr) {
    const bool real = live && col < k1;
    const double z = real ? (double)row[col] / T : kNegInf;
    double m = z;
    for (int o = G >> 1; o > 0; o >>= 1) {
        const double v = __shfl_xor(m, o);
        m = (v > m || v != v) ? v : m;          // NaN wins, like np.max
    }
    const double e = real ? exp(z - m) : 0.0;
    double s = e;
    for (int o = G >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (LOGP) *lp = (z - m) - log(s);
    return e / s;
}

// K+1 > 64: the lane owns the row.  Sum in column order; out[k] for k < n_store, returns p_want (want < 0: nothing).
// out_lp (optional): log p_k for all k1 columns.
__device__ __forceinline__ double softmax_serial(const float* row, int k1, double T, double* out, int n_store, int want,
                                                 double* out_lp = nullptr) {
    double m = kNegInf;
    for (int k = 0; k < k1; ++k) {
        const double z = (double)row[k] / T;
        m = (z > m || z != z) ? z : m;
    }
    double s = 0.0;
    for (int k = 0; k < k1; ++k) s += exp((double)row[k] / T - m);
    double pw = 0.0;
    for (int k = 0; k < k1; ++k) {
        const double p = exp((double)row[k] / T - m) / s;
        if (k < n_store) out[k] = p;
        if (k == want) pw = p;
    }
    if (out_lp) {
        const double ls = log(s);
        for (int k = 0; k < k1; ++k) out_lp[k] = ((double)row[k] / T - m) - ls;
    }
    return pw;
}

}  // namespace pe
