// Fused input build of the FLIR early / middle fusion detectors (gfx950).
//   pe_fusion_input_pack : uint8 thermal + uint8 RGB frame batches -> the detector's normalised, zero-padded NHWC4 fp16 input
//
// The reference builds the 4- / 6-channel input on the host (demo/FLIR/demo_FLIR_save_predictions.py:98-121): the RGB frame is
// resized to the thermal frame's size with OpenCV's 8-bit INTER_LINEAR (proben_amd.data.cv2_linear_resize_u8), stacked with the
// thermal channels (early: B,G,R,T0; middle: B,G,R,T0,T1,T2) as floating point, and the model's ResizeShortestEdge resizes that
// with the float INTER_LINEAR rule (misc.hip preprocess_pack_kernel, src_kind 1).  The intermediate values are integers, so this
// kernel computes them from the uint8 frames and applies the float rule in the same order: the output is bit for bit the output of
// the host build + float32 upload + pe_preprocess_pack_batch route.  Built with -ffp-contract=off (the float rule must not fuse).
#include <hip/hip_fp16.h>

#include "common.h"

namespace {
typedef _Float16 half4 __attribute__((ext_vector_type(4)));

struct FuseArgs {
    const unsigned char* th;   // [N, th_h, th_w, 3] BGR
    const unsigned char* rgb;  // [N, rgb_h, rgb_w, 3] BGR (null when no output channel is an RGB one)
    int th_h, th_w, rgb_h, rgb_w;
    int ch0, nch;              // stacked channels [ch0, ch0 + nch) of B,G,R,T0,T1,T2 -> output channels 0..nch-1
    int dst_h, dst_w, pad_h, pad_w;
    float mean[4], inv_std[4];
    _Float16* dst;             // [N, pad_h, pad_w, 4]
};

// one axis of OpenCV's 8-bit INTER_LINEAR (data.cv2_linear_resize_u8 taps): half-pixel source coordinate in double, the fraction
// cast to float, border taps collapsed onto the edge, 11-bit coefficients rounded half to even
struct CvTap { int i0, i1, c0, c1; };

__device__ __forceinline__ CvTap cv_tap(int i, int n_in, int n_out) {
    const double f = ((double)i + 0.5) * ((double)n_in / (double)n_out) - 0.5;
    const double fl = floor(f);
    int i0 = (int)fl;
    float a = (float)(f - fl);
    if (i0 < 0) { a = 0.f; i0 = 0; }
    if (i0 >= n_in - 1) { a = 0.f; i0 = n_in - 1; }
    CvTap t;
    t.i0 = i0;
    t.i1 = min(i0 + 1, n_in - 1);
    t.c1 = (int)rint((double)a * 2048.0);
    t.c0 = (int)rint((double)(1.f - a) * 2048.0);
    return t;
}

// the group's nch channels of the thermal-size stacked frame at (ty, tx), one byte each
__device__ __forceinline__ unsigned mid_px(const FuseArgs& a, const unsigned char* th, const unsigned char* rgb, int ty, int tx) {
    unsigned out = 0;
    const bool same = a.rgb_h == a.th_h && a.rgb_w == a.th_w;
    CvTap X = {tx, tx, 2048, 0}, Y = {ty, ty, 2048, 0};
    if (a.ch0 < 3 && !same) {
        X = cv_tap(tx, a.rgb_w, a.th_w);
        Y = cv_tap(ty, a.rgb_h, a.th_h);
    }
    for (int c = 0; c < a.nch; ++c) {
        const int s = a.ch0 + c;
        int v;
        if (s >= 3) {
            v = th[((size_t)ty * a.th_w + tx) * 3 + (s - 3)];
        } else if (same) {
            v = rgb[((size_t)ty * a.rgb_w + tx) * 3 + s];
        } else {
            const unsigned char* r0 = rgb + (size_t)Y.i0 * a.rgb_w * 3 + s;
            const unsigned char* r1 = rgb + (size_t)Y.i1 * a.rgb_w * 3 + s;
            const int h0 = ((int)r0[X.i0 * 3] * X.c0 + (int)r0[X.i1 * 3] * X.c1) >> 4;
            const int h1 = ((int)r1[X.i0 * 3] * X.c0 + (int)r1[X.i1 * 3] * X.c1) >> 4;
            v = (((Y.c0 * h0) >> 16) + ((Y.c1 * h1) >> 16) + 2) >> 2;
            v = v < 0 ? 0 : (v > 255 ? 255 : v);
        }
        out |= (unsigned)v << (8 * c);
    }
    return out;
}

// the float INTER_LINEAR taps of preprocess_pack_kernel (misc.hip) for output coordinate i of a src -> dst resize
struct FTap { int i0, i1; float s; };

__device__ __forceinline__ FTap f_tap(int i, int n_src, int n_dst) {
    const double f = ((double)i + 0.5) * ((double)n_src / (double)n_dst) - 0.5;
    float s = (float)f;
    int i0 = (int)floorf(s);
    s -= (float)i0;
    if (i0 < 0) { i0 = 0; s = 0.f; }
    if (i0 >= n_src - 1) { i0 = n_src - 1; s = 0.f; }
    FTap t;
    t.i0 = i0;
    t.i1 = min(i0 + 1, n_src - 1);
    t.s = s;
    return t;
}

__device__ __forceinline__ half4 blend(const FuseArgs& a, unsigned p00, unsigned p01, unsigned p10, unsigned p11, float sx, float sy) {
    half4 o = {0, 0, 0, 0};
    for (int c = 0; c < a.nch; ++c) {
        const float v00 = (float)((p00 >> (8 * c)) & 255u), v01 = (float)((p01 >> (8 * c)) & 255u);
        const float v10 = (float)((p10 >> (8 * c)) & 255u), v11 = (float)((p11 >> (8 * c)) & 255u);
        const double top = (double)v00 * (double)(1.f - sx) + (double)v01 * (double)sx;
        const double bot = (double)v10 * (double)(1.f - sx) + (double)v11 * (double)sx;
        const float v = (float)(top * (double)(1.f - sy) + bot * (double)sy);
        o[c] = (_Float16)((v - a.mean[c]) * a.inv_std[c]);
    }
    return o;
}

__device__ __forceinline__ half4 normalise(const FuseArgs& a, unsigned p) {
    half4 o = {0, 0, 0, 0};
    for (int c = 0; c < a.nch; ++c) o[c] = (_Float16)(((float)((p >> (8 * c)) & 255u) - a.mean[c]) * a.inv_std[c]);
    return o;
}

// A workgroup makes a 256-column x 16-row tile of one image's output.  The thermal-size stacked pixels the tile's taps reach form
// one rectangle (the taps are monotone in the output coordinate); it is computed once into LDS - 16 RGB bytes + the 8-bit rule per
// pixel - and the float pass reads its 2 x 2 taps from there.  A rectangle larger than the LDS buffer (output well below the
// thermal size) takes the per-pixel form, same arithmetic.
constexpr int FI_TX = 256, FI_TY = 16, FI_LDS = 8192;

__global__ __launch_bounds__(FI_TX) void fusion_input_kernel(FuseArgs a) {
    __shared__ unsigned win[FI_LDS];
    const size_t z = blockIdx.z;
    const unsigned char* th = a.th + z * a.th_h * a.th_w * 3;
    const unsigned char* rgb = a.rgb ? a.rgb + z * a.rgb_h * a.rgb_w * 3 : nullptr;
    _Float16* dst = a.dst + z * a.pad_h * a.pad_w * 4;
    const int tid = threadIdx.x;
    const int xs = blockIdx.x * FI_TX;
    const int x = xs + tid;
    const int y0 = blockIdx.y * FI_TY;
    const int rows = min(FI_TY, a.pad_h - y0);
    const bool resize = a.dst_h != a.th_h || a.dst_w != a.th_w;
    const bool live = y0 < a.dst_h && xs < a.dst_w;             // the tile has image pixels
    int wx0 = 0, wy0 = 0, ww = 0, wh = 0;
    if (live) {
        const int xe = min(xs + FI_TX, a.dst_w) - 1, ye = min(y0 + FI_TY, a.dst_h) - 1;
        if (resize) {
            wx0 = f_tap(xs, a.th_w, a.dst_w).i0;
            wy0 = f_tap(y0, a.th_h, a.dst_h).i0;
            ww = f_tap(xe, a.th_w, a.dst_w).i1 - wx0 + 1;
            wh = f_tap(ye, a.th_h, a.dst_h).i1 - wy0 + 1;
        } else {
            wx0 = xs; wy0 = y0; ww = xe - xs + 1; wh = ye - y0 + 1;
        }
    }
    const bool tiled = live && ww * wh <= FI_LDS;                // workgroup-uniform
    if (tiled) {
        for (int k = tid; k < ww * wh; k += FI_TX) {
            const int r = k / ww;
            win[k] = mid_px(a, th, rgb, wy0 + r, wx0 + (k - r * ww));
        }
        __syncthreads();
    }
    if (x >= a.pad_w) return;
    const bool col_live = x < a.dst_w;
    FTap X = {x, x, 0.f};
    if (col_live && resize) X = f_tap(x, a.th_w, a.dst_w);
    for (int yy = 0; yy < rows; ++yy) {
        const int y = y0 + yy;
        half4 o = {0, 0, 0, 0};
        if (y < a.dst_h && col_live) {
            if (!resize) {
                o = normalise(a, tiled ? win[yy * ww + tid] : mid_px(a, th, rgb, y, x));
            } else {
                const FTap Y = f_tap(y, a.th_h, a.dst_h);
                unsigned p00, p01, p10, p11;
                if (tiled) {
                    const unsigned* r0 = win + (Y.i0 - wy0) * ww - wx0;
                    const unsigned* r1 = win + (Y.i1 - wy0) * ww - wx0;
                    p00 = r0[X.i0]; p01 = r0[X.i1]; p10 = r1[X.i0]; p11 = r1[X.i1];
                } else {
                    p00 = mid_px(a, th, rgb, Y.i0, X.i0); p01 = mid_px(a, th, rgb, Y.i0, X.i1);
                    p10 = mid_px(a, th, rgb, Y.i1, X.i0); p11 = mid_px(a, th, rgb, Y.i1, X.i1);
                }
                o = blend(a, p00, p01, p10, p11, X.s, Y.s);
            }
        }
        *reinterpret_cast<half4*>(dst + ((size_t)y * a.pad_w + x) * 4) = o;
    }
}
}  // namespace

extern "C" int pe_fusion_input_pack(const void* thermal, const void* rgb, int32_t num_images, int32_t th_h, int32_t th_w,
                                    int32_t rgb_h, int32_t rgb_w, int32_t ch0, int32_t nch, int32_t dst_h, int32_t dst_w,
                                    int32_t pad_h, int32_t pad_w, int32_t pad_multiple, const float* mean_host,
                                    const float* std_host, void* dst, void* stream) {
    PE_CHECK_ARG(thermal && dst && mean_host && std_host, "pe_fusion_input_pack: null pointer");
    PE_CHECK_ARG(nch >= 1 && nch <= 4 && ch0 >= 0 && ch0 + nch <= 6,
                 "pe_fusion_input_pack: channel window [%d,%d) of the 6 stacked channels B,G,R,T0,T1,T2", ch0, ch0 + nch);
    PE_CHECK_ARG(ch0 >= 3 || rgb, "pe_fusion_input_pack: null pointer (channels [%d,%d) read the RGB batch)", ch0, ch0 + nch);
    PE_CHECK_ARG(num_images >= 1 && num_images <= 65535, "pe_fusion_input_pack: num_images %d", num_images);
    PE_CHECK_ARG(th_h > 0 && th_w > 0 && (ch0 >= 3 || (rgb_h > 0 && rgb_w > 0)),
                 "pe_fusion_input_pack: bad frame sizes (thermal %dx%d, rgb %dx%d)", th_h, th_w, rgb_h, rgb_w);
    PE_CHECK_ARG(dst_h > 0 && dst_w > 0 && dst_h <= pad_h && dst_w <= pad_w,
                 "pe_fusion_input_pack: bad sizes (resized %dx%d, padded %dx%d)", dst_h, dst_w, pad_h, pad_w);
    PE_CHECK_ARG(pad_multiple >= 1 && pad_h % pad_multiple == 0 && pad_w % pad_multiple == 0 && pad_h - dst_h < pad_multiple &&
                     pad_w - dst_w < pad_multiple,
                 "pe_fusion_input_pack: padded size %dx%d is not the resized size %dx%d rounded up to a multiple of %d", pad_h, pad_w,
                 dst_h, dst_w, pad_multiple);
    FuseArgs a{};
    a.th = (const unsigned char*)thermal; a.rgb = ch0 < 3 ? (const unsigned char*)rgb : nullptr;
    a.th_h = th_h; a.th_w = th_w; a.rgb_h = rgb_h; a.rgb_w = rgb_w; a.ch0 = ch0; a.nch = nch;
    a.dst_h = dst_h; a.dst_w = dst_w; a.pad_h = pad_h; a.pad_w = pad_w; a.dst = (_Float16*)dst;
    for (int c = 0; c < 4; ++c) {
        a.mean[c] = c < nch ? mean_host[c] : 0.f;
        a.inv_std[c] = c < nch ? 1.f / std_host[c] : 0.f;
    }
    const dim3 grid(pe::ceil_div(pad_w, FI_TX), pe::ceil_div(pad_h, FI_TY), num_images);
    hipLaunchKernelGGL(fusion_input_kernel, grid, dim3(FI_TX), 0, (hipStream_t)stream, a);
    PE_CHECK_LAUNCH("pe_fusion_input_pack");
    return PE_OK;
}
