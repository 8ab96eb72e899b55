// BatchNorm re-calibration of a supernet sub-network (lp_calib_*, engine.cpp): the training-mode forward of
// lib/models/pose_supermobilenet.py / layers/super_layers.py:19-28 as the reference's calibrate_test.py:44-122 runs it.
// Every BatchNorm normalises with the statistics of the batch and moves its running pair towards them.
//
// Per BatchNorm layer: the raw convolution (the library's unfused launches with an identity fold; the two raw forms below
// for the layers whose library kernel has its activation built in), then
//   bn_stats_kernel   one pass over the raw tensor: per-channel sum and sum of squares in fp64, one partial per workgroup
//   bn_apply_kernel   combines the partials of its channel in index order (every workgroup the same way, no atomics: two
//                     runs give the same bits), normalises in place, applies the activation and the residual add, and --
//                     the workgroup of slice 0 -- moves the channel's running pair
// Both stream the tensor with 16-byte accesses when the plane is a multiple of four floats (every plane above 1/16 of a
// 32-multiple input; the scalar form covers the rest).  The N planes of a channel are one unit range cut into S <= 64
// slices, so that a 16-channel layer still fills the chip and a 16x16 plane still fills a wave: grid = S x C workgroups.
#include "kernels.h"

namespace lp {

// slices of one channel: its N planes are ONE range of N * units units (float4s or floats; unit u = plane u / units,
// offset u % units), cut into S chunks of `chunk` units.  A 16x16 plane is 64 float4s: cutting planes instead would leave
// three lanes of four idle on the deep stages, where most of the BatchNorm layers are.
BnCut bn_cut(int N, int C, int HW) {
    BnCut k;
    k.vec = (HW & 3) == 0;
    const long total = (long)N * (k.vec ? HW >> 2 : HW);
    int want = (2048 + C - 1) / C;
    want = want < 1 ? 1 : (want > 64 ? 64 : want);
    long S = (total + 511) / 512;                       // at least two loads per lane and slice
    S = S < 1 ? 1 : (S > want ? want : S);
    k.chunk = (int)((total + S - 1) / S);
    k.S = (int)((total + k.chunk - 1) / k.chunk);
    return k;
}

// conv 3x3 stride 2 pad 1, 3 -> 32, raw (no bias, no activation): stem_kernel's loop without its epilogue
__global__ __launch_bounds__(256) void stem_raw_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                       float* __restrict__ out, int N, int H, int W) {
    const int OH = H >> 1, OW = W >> 1;
    const long total = (long)N * OH * OW;
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const int ox = (int)(g % OW);
    const int oy = (int)((g / OW) % OH);
    const int n = (int)(g / ((long)OW * OH));
    float v[27];
#pragma unroll
    for (int ci = 0; ci < 3; ++ci) {
        const float* plane = x + ((long)n * 3 + ci) * H * W;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = 2 * oy - 1 + ky;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = 2 * ox - 1 + kx;
                v[ci * 9 + ky * 3 + kx] = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? plane[(long)iy * W + ix] : 0.f;
            }
        }
    }
    float* o = out + (long)n * 32 * OH * OW + (long)oy * OW + ox;
#pragma unroll 4
    for (int co = 0; co < 32; ++co) {
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < 27; ++i) acc = fmaf(v[i], w[co * 27 + i], acc);
        o[(long)co * OH * OW] = acc;
    }
}

// ConvTranspose2d(k4, s2, p1) of the refined source + the same of the raw source (inB may be null: Cb = 0), raw sum.
// w [Ca+Cb][Cout][4][4].  One input cell per lane -> its 2x2 output cells, COT output channels per workgroup row.
constexpr int COT = 8;
__global__ __launch_bounds__(256) void deconv_raw_kernel(const float* __restrict__ inA, int Ca,
                                                         const float* __restrict__ inB, int Cb,
                                                         const float* __restrict__ w, float* __restrict__ out, int N,
                                                         int h, int w_, int Cout) {
    const long total = (long)N * h * w_;
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const int ix = (int)(g % w_);
    const int iy = (int)((g / w_) % h);
    const int n = (int)(g / ((long)w_ * h));
    const int co0 = blockIdx.y * COT;
    float acc[COT][4];
#pragma unroll
    for (int c = 0; c < COT; ++c) acc[c][0] = acc[c][1] = acc[c][2] = acc[c][3] = 0.f;
    for (int src = 0; src < 2; ++src) {
        const float* in = src == 0 ? inA : inB;
        const int Cs = src == 0 ? Ca : (inB ? Cb : 0);
        const int cbase = src == 0 ? 0 : Ca;
        for (int ci = 0; ci < Cs; ++ci) {
            const float* plane = in + ((long)n * Cs + ci) * h * w_;
            float v[3][3];
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    const int y = iy + dy, xx = ix + dx;
                    v[dy + 1][dx + 1] = (y >= 0 && y < h && xx >= 0 && xx < w_) ? plane[(long)y * w_ + xx] : 0.f;
                }
            const float* wc = w + ((long)(cbase + ci) * Cout + co0) * 16;
#pragma unroll
            for (int c = 0; c < COT; ++c) {
                if (co0 + c < Cout) {
                    const float* k = wc + c * 16;      // [ky][kx]
#pragma unroll
                    for (int a = 0; a < 2; ++a)
#pragma unroll
                        for (int bb = 0; bb < 2; ++bb) {
                            // output (2iy + a, 2ix + bb) = sum over the two rows / columns that reach it
                            const int dy0 = a == 0 ? 0 : 1, ky0 = a == 0 ? 1 : 0;
                            const int dy1 = a == 0 ? -1 : 0, ky1 = a == 0 ? 3 : 2;
                            const int dx0 = bb == 0 ? 0 : 1, kx0 = bb == 0 ? 1 : 0;
                            const int dx1 = bb == 0 ? -1 : 0, kx1 = bb == 0 ? 3 : 2;
                            float t = acc[c][a * 2 + bb];
                            t = fmaf(v[dy0 + 1][dx0 + 1], k[ky0 * 4 + kx0], t);
                            t = fmaf(v[dy0 + 1][dx1 + 1], k[ky0 * 4 + kx1], t);
                            t = fmaf(v[dy1 + 1][dx0 + 1], k[ky1 * 4 + kx0], t);
                            t = fmaf(v[dy1 + 1][dx1 + 1], k[ky1 * 4 + kx1], t);
                            acc[c][a * 2 + bb] = t;
                        }
                }
            }
        }
    }
    const int OW = 2 * w_, OH = 2 * h;
#pragma unroll
    for (int c = 0; c < COT; ++c) {
        const int co = co0 + c;
        if (co < Cout) {
            float* o = out + ((long)n * Cout + co) * OH * OW + (long)(2 * iy) * OW + 2 * ix;
            *reinterpret_cast<float2*>(o) = float2{acc[c][0], acc[c][1]};
            *reinterpret_cast<float2*>(o + OW) = float2{acc[c][2], acc[c][3]};
        }
    }
}

// per-channel partial (sum, sum of squares) in fp64.  grid (S, C): slice s reads units [s * chunk, (s + 1) * chunk) of
// the channel's N * units.  A lane steps 256 units at a time: (plane, offset) advance by (256 / units, 256 % units) with
// one carry, no division in the loop.  The workgroup's 256 values are added in a fixed tree.
template <bool VEC>
__global__ __launch_bounds__(256) void bn_stats_kernel(const float* __restrict__ x, double2* __restrict__ part, int N,
                                                       int C, int HW, int chunk) {
    const int s = blockIdx.x, c = blockIdx.y, S = gridDim.x;
    const int units = VEC ? HW >> 2 : HW;
    const long total = (long)N * units;
    const long u0 = (long)s * chunk, u1 = min(u0 + chunk, total);
    const int dn = 256 / units, di = 256 % units;
    const long plane = (long)C * HW;
    long u = u0 + threadIdx.x;
    int n = (int)(u / units), i = (int)(u - (long)n * units);
    const float* px = x + (long)c * HW;
    double sum = 0.0, sq = 0.0;
    for (; u < u1; u += 256) {
        if (VEC) {
            const float4 v = reinterpret_cast<const float4*>(px + n * plane)[i];
            const double a = v.x, b = v.y, d = v.z, e = v.w;
            sum += (a + b) + (d + e);
            sq += (a * a + b * b) + (d * d + e * e);
        } else {
            const double a = px[n * plane + i];
            sum += a;
            sq += a * a;
        }
        n += dn;
        i += di;
        if (i >= units) { i -= units; ++n; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_down(sum, o, 64);
        sq += __shfl_down(sq, o, 64);
    }
    __shared__ double2 wv[4];
    if ((threadIdx.x & 63) == 0) wv[threadIdx.x >> 6] = double2{sum, sq};
    __syncthreads();
    if (threadIdx.x == 0)
        part[(long)c * S + s] = double2{(wv[0].x + wv[1].x) + (wv[2].x + wv[3].x), (wv[0].y + wv[1].y) + (wv[2].y + wv[3].y)};
}

// x = act((x - mean) * rsqrt(var + eps) * gamma + beta) (+ res), in place, with the batch's biased variance; bn =
// [gamma | beta | running_mean | running_var] x C.  Slice 0 of a channel moves its running pair: (1 - m) * running + m *
// batch in fp64, rounded once, with the unbiased variance n / (n - 1) (torch.nn.functional.batch_norm, training = True).
template <bool VEC>
__global__ __launch_bounds__(256) void bn_apply_kernel(float* __restrict__ x, const float* __restrict__ res,
                                                       const double2* __restrict__ part, float* __restrict__ bn, int N,
                                                       int C, int HW, int chunk, int act, double momentum, double eps) {
    const int s = blockIdx.x, c = blockIdx.y, S = gridDim.x;
    double sum = 0.0, sq = 0.0;
    for (int i = 0; i < S; ++i) {
        const double2 d = part[(long)c * S + i];
        sum += d.x;
        sq += d.y;
    }
    const double cnt = (double)N * (double)HW;
    const double mean = sum / cnt;
    double var = sq / cnt - mean * mean;
    var = var < 0.0 ? 0.0 : var;                        // a NaN variance (a NaN or an Inf in the channel) stays NaN
    if (s == 0 && threadIdx.x == 0) {
        const double unb = cnt > 1.0 ? var * (cnt / (cnt - 1.0)) : var;
        bn[2 * C + c] = (float)((1.0 - momentum) * (double)bn[2 * C + c] + momentum * mean);
        bn[3 * C + c] = (float)((1.0 - momentum) * (double)bn[3 * C + c] + momentum * unb);
    }
    const float meanf = (float)mean, istd = (float)(1.0 / sqrt(var + eps));
    const float ga = bn[c], be = bn[C + c];
    const float lo = act == ACT_NONE ? -INFINITY : 0.f;
    const float hi = act == ACT_RELU6 ? 6.f : INFINITY;
    const int units = VEC ? HW >> 2 : HW;
    const long total = (long)N * units;
    const long u0 = (long)s * chunk, u1 = min(u0 + chunk, total);
    const int dn = 256 / units, di = 256 % units;
    const long plane = (long)C * HW;
    long u = u0 + threadIdx.x;
    int n = (int)(u / units), i = (int)(u - (long)n * units);
    auto f = [&](float v) {                             // a NaN stays a NaN, as in bn_fwd_kernel (layer_kernels.hip)
        const float z = ((v - meanf) * istd) * ga + be;
        return z != z ? z : fminf(fmaxf(z, lo), hi);
    };
    for (; u < u1; u += 256) {
        const long base = (long)c * HW + n * plane;
        if (VEC) {
            float4 v = reinterpret_cast<const float4*>(x + base)[i];
            v.x = f(v.x); v.y = f(v.y); v.z = f(v.z); v.w = f(v.w);
            if (res) {
                const float4 r = reinterpret_cast<const float4*>(res + base)[i];
                v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
            }
            reinterpret_cast<float4*>(x + base)[i] = v;
        } else {
            float v = f(x[base + i]);
            if (res) v += res[base + i];
            x[base + i] = v;
        }
        n += dn;
        i += di;
        if (i >= units) { i -= units; ++n; }
    }
}

void launch_stem_raw(const float* x, const float* w, float* out, int N, int H, int W, hipStream_t s) {
    const long total = (long)N * (H / 2) * (W / 2);
    LP_LAUNCH(stem_raw_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, w, out, N, H, W);
}

void launch_deconv_raw(const float* inA, int Ca, const float* inB, int Cb, const float* w, float* out, int N, int h,
                       int w_, int Cout, hipStream_t s) {
    const long total = (long)N * h * w_;
    dim3 grid((unsigned)((total + 255) / 256), (Cout + COT - 1) / COT), block(256);
    LP_LAUNCH(deconv_raw_kernel, grid, block, 0, s, inA, Ca, inB, Cb, w, out, N, h, w_, Cout);
}

size_t bn_partial_doubles(int N, int C, int HW) { return 2 * (size_t)C * bn_cut(N, C, HW).S; }

void launch_bn_stats(const float* x, double* part, int N, int C, int HW, hipStream_t s) {
    const BnCut k = bn_cut(N, C, HW);
    dim3 grid(k.S, C), block(256);
    if (k.vec)
        LP_LAUNCH(bn_stats_kernel<true>, grid, block, 0, s, x, (double2*)part, N, C, HW, k.chunk);
    else
        LP_LAUNCH(bn_stats_kernel<false>, grid, block, 0, s, x, (double2*)part, N, C, HW, k.chunk);
}

void launch_bn_apply(float* x, const float* res, const double* part, float* bn, int N, int C, int HW, int act,
                     double momentum, double eps, hipStream_t s) {
    const BnCut k = bn_cut(N, C, HW);
    dim3 grid(k.S, C), block(256);
    if (k.vec)
        LP_LAUNCH(bn_apply_kernel<true>, grid, block, 0, s, x, res, (const double2*)part, bn, N, C, HW, k.chunk, act,
                  momentum, eps);
    else
        LP_LAUNCH(bn_apply_kernel<false>, grid, block, 0, s, x, res, (const double2*)part, bn, N, C, HW, k.chunk, act,
                  momentum, eps);
}

}  // namespace lp
