// The box-delta residual of a detection against its ground-truth box, shared by pe_variance_stats (csrc/variance.hip) and
// pe_box_pair_stats (csrc/boxcorr.hip): the same expressions, so a row gets the same bits from either.
#pragma once
#include "common.h"

namespace pe {

// Box2BoxTransform.get_deltas(s, t) of the source box s against the target t (XYXY): w[:2] * (tc - sc) / swh, w[2:] * log(twh / swh).
// false, and res untouched, when a width or a height of either box is not > 0 (NaN included).
__device__ __forceinline__ bool box_residual(const double* s, const double* t, const double (&w)[4], double (&res)[4]) {
    const double sw = s[2] - s[0], sh = s[3] - s[1];
    const double tw = t[2] - t[0], th = t[3] - t[1];
    if (!(sw > 0.0 && sh > 0.0 && tw > 0.0 && th > 0.0)) return false;
    const double scx = s[0] + 0.5 * sw, scy = s[1] + 0.5 * sh;
    const double tcx = t[0] + 0.5 * tw, tcy = t[1] + 0.5 * th;
    res[0] = w[0] * (tcx - scx) / sw;
    res[1] = w[1] * (tcy - scy) / sh;
    res[2] = w[2] * log(tw / sw);
    res[3] = w[3] * log(th / sh);
    return true;
}

// bbox_reg_weights_host (null: cfg.MODEL.ROI_BOX_HEAD.BBOX_REG_WEIGHTS' default) -> w, every entry finite and > 0
inline int bbox_reg_weights(const float* host, double (&w)[4], const char* what) {
    static const float kDefaultWeights[4] = {10.f, 10.f, 5.f, 5.f};
    const float* src = host ? host : kDefaultWeights;
    for (int c = 0; c < 4; ++c) {
        PE_CHECK_ARG(src[c] == src[c] && src[c] > 0.f && src[c] < __builtin_huge_valf(), "%s: bbox_reg_weights[%d] %g is not finite and > 0", what,
                     c, (double)src[c]);
        w[c] = (double)src[c];
    }
    return PE_OK;
}

}  // namespace pe
