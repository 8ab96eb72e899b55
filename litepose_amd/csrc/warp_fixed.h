// cv2.warpAffine's 8-bit fixed-point bilinear scheme for ONE destination pixel (the published algorithm of
// opencv/modules/imgproc/src/imgwarp.cpp, warpAffine + remapBilinear), shared by every kernel that warps: the three-channel
// image kernels of ae_kernels.hip and the one-channel mask kernel of target_kernels.hip compute their source position, their
// weights and their rounding here, so they agree bit for bit by construction.
//   source position in 1/1024 px:  X = round(M[0]*x*1024) + round((M[1]*y+M[2])*1024) + 16   (likewise Y)
//   integer pixel X>>10, 5 fractional bits fx = (X>>5)&31, weights (32-fx)(32-fy)*32 .. fx*fy*32
//   (sum 32768), value = (sum w*p + 16384) >> 15, taps outside the image contribute 0.
// The matrix is the INVERTED (dst->src) one, in fp64.  Compile without FMA contraction.
#pragma once
#include <hip/hip_runtime.h>

namespace lp {

__device__ __forceinline__ int sat_int_rint(double v) {
    const double r = rint(v);
    return r >= 2147483647.0 ? 2147483647 : (r <= -2147483648.0 ? (int)-2147483648LL : (int)r);
}

struct WarpTaps {
    int sx, sy;                 // top-left source pixel (may lie outside the image)
    int w00, w01, w10, w11;     // 15-bit weights of (sy, sx), (sy, sx+1), (sy+1, sx), (sy+1, sx+1)
    bool x0, x1, y0, y1;        // column sx / sx+1 and row sy / sy+1 inside the H x W source
};

__device__ __forceinline__ WarpTaps warp_taps(int H, int W, int x, int y, double m0, double m1, double m2, double m3,
                                              double m4, double m5) {
    const int adelta = sat_int_rint(m0 * (double)x * 1024.0), bdelta = sat_int_rint(m3 * (double)x * 1024.0);
    const int X0 = sat_int_rint((m1 * (double)y + m2) * 1024.0) + 16;
    const int Y0 = sat_int_rint((m4 * (double)y + m5) * 1024.0) + 16;
    const int X = (X0 + adelta) >> 5, Y = (Y0 + bdelta) >> 5;
    WarpTaps t;
    t.sx = min(max(X >> 5, -32768), 32767);
    t.sy = min(max(Y >> 5, -32768), 32767);
    const int fx = X & 31, fy = Y & 31;
    t.w00 = (32 - fx) * (32 - fy) * 32;
    if (t.w00 > 32767) t.w00 = 32767;                     // saturate_cast<short>(1.0 * 32768)
    t.w01 = fx * (32 - fy) * 32;
    t.w10 = (32 - fx) * fy * 32;
    t.w11 = fx * fy * 32;
    t.x0 = t.sx >= 0 && t.sx < W;
    t.x1 = t.sx + 1 >= 0 && t.sx + 1 < W;
    t.y0 = t.sy >= 0 && t.sy < H;
    t.y1 = t.sy + 1 >= 0 && t.sy + 1 < H;
    return t;
}

// the interpolated byte of four taps (0 where a tap lies outside the image)
__device__ __forceinline__ int warp_blend(const WarpTaps& t, int p00, int p01, int p10, int p11) {
    const int v = (p00 * t.w00 + p01 * t.w01 + p10 * t.w10 + p11 * t.w11 + 16384) >> 15;
    return min(max(v, 0), 255);
}

}  // namespace lp
