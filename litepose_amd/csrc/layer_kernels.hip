// Training-mode layers (lp_bn_* / lp_pw_* / lp_dw_*, layer_api.cpp): the forwards that keep what a backward needs and the
// backwards of the three layer kinds every InvBottleneck, first.1 / first.2 and both SepConv2d heads are made of.
// fp32, planar NCHW.  No atomics anywhere: every sum has one order that depends on the shapes only, so two calls (and a
// graph replay) give the same bits.
//
//   BatchNorm (+ act, + residual)   bn_stats_kernel (calib_kernels.hip) -> bn_fwd_kernel, out of place: the raw input
//                                   survives, the channel's (mean, invstd) pair is kept in fp64 for the backward
//                                   bn_bwd_stats_kernel -> bn_bwd_apply_kernel: the twins of that pair
//   the same, synchronised over W ranks (lp_bn_sync_*): a collective of the caller's between the two halves of a pass --
//                                   bn_stats_kernel -> bn_row_kernel (this rank's partials -> one fp64 row) | all-gather |
//                                   bn_sync_fwd_kernel (the W rows added in rank order by every workgroup alike);
//                                   bn_bwd_stats_kernel -> bn_row_kernel | all-gather | bn_sync_bwd_kernel.  The plain and
//                                   the synchronised kernels share their bodies (bn_moments, bn_keep, bn_fwd_slice,
//                                   bn_bwd_slice): W = 1 gives the plain kernels' bits
//   1x1                             forward and data gradient are launch_pw on A fragments packed on the device
//                                   (pw_pack_kernel: W, or W^T for the data gradient); the weight gradient is
//                                   pw_wgrad_kernel, a GEMM over the N * HW pixels on v_mfma_f32_32x32x2_f32, cut into
//                                   slices of LP_PW_WGRAD_SLICE pixels -> fp32 partials -> slice_sum_kernel (fp64, in
//                                   index order, one rounding)
//   depthwise                       forward is launch_dw on taps duplicated on the device (dw_pack_kernel); the data
//                                   gradient dw_dgrad_kernel gathers, for both strides, the output taps that land on an
//                                   input cell (no scatter); the weight gradient dw_wgrad_kernel owns a (channel, slice
//                                   of LP_DW_WGRAD_SLICE 16x16 output tiles), stages the haloed input tile in LDS and
//                                   reduces its 256 lanes in a fixed tree -> fp32 partials -> slice_sum_kernel
#include "../../include/litepose_amd.h"
#include "kernels.h"

namespace lp {

typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));

// ====================================================================================== BatchNorm
// z = gamma * xhat + beta: THE expression of the forward, and what the backward recomputes to find the cells the
// activation passed.  Three fp32 roundings (subtract, multiply, fused multiply-add) on top of the two of (meanf, istd).
__device__ __forceinline__ float bn_z(float v, float meanf, float istd, float ga, float be) {
    return fmaf((v - meanf) * istd, ga, be);
}
// act'(z) as torch has it: strict inequalities (ReLU: z > 0; ReLU6: 0 < z < 6), written as torch's backward writes them,
// "closed where z <= 0 or z >= 6": a NaN z is on neither side of a kink and PASSES its gradient (threshold_backward,
// hardtanh_backward), so that dbeta of a channel that went NaN is the sum of dy, as torch's, and a NaN dy there shows.
__device__ __forceinline__ bool bn_pass(float z, int act) {
    return act == ACT_NONE || (!(z <= 0.f) && (act != ACT_RELU6 || !(z >= 6.f)));
}

// the slice walk of bn_stats_kernel: unit u of the channel's N * units -> element offset, 256 units per step
template <bool VEC, class F>
__device__ __forceinline__ void bn_walk(int N, int C, int HW, int chunk, int s, int c, F f) {
    const int units = VEC ? HW >> 2 : HW;
    const long total = (long)N * units;
    const long u0 = (long)s * chunk, u1 = min(u0 + chunk, total);
    const int dn = 256 / units, di = 256 % units;
    const long plane = (long)C * HW;
    long u = u0 + threadIdx.x;
    int n = (int)(u / units), i = (int)(u - (long)n * units);
    for (; u < u1; u += 256) {
        f((long)c * HW + n * plane + (VEC ? 4 * i : i));
        n += dn;
        i += di;
        if (i >= units) { i -= units; ++n; }
    }
}

// the workgroup's 256 pairs added in the fixed tree of bn_stats_kernel; the result is valid in thread 0
__device__ __forceinline__ double2 bn_block_sum(double a, double b) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_down(a, o, 64);
        b += __shfl_down(b, o, 64);
    }
    __shared__ double2 wv[4];
    if ((threadIdx.x & 63) == 0) wv[threadIdx.x >> 6] = double2{a, b};
    __syncthreads();
    return double2{(wv[0].x + wv[1].x) + (wv[2].x + wv[3].x), (wv[0].y + wv[1].y) + (wv[2].y + wv[3].y)};
}

// mean, the clamped biased variance and invstd of a channel from its (sum, sum of squares) over cnt cells: THE expression of
// bn_fwd_kernel and bn_sync_fwd_kernel
__device__ __forceinline__ void bn_moments(double sum, double sq, double cnt, double eps, double& mean, double& var,
                                           double& invstd) {
    mean = sum / cnt;
    var = sq / cnt - mean * mean;
    var = var < 0.0 ? 0.0 : var;                        // a NaN variance (a NaN or an Inf in the channel) stays NaN
    invstd = 1.0 / sqrt(var + eps);
}

// one thread per channel: the kept fp64 pair and the running pair moved by `momentum` with the unbiased variance over cnt
__device__ __forceinline__ void bn_keep(float* __restrict__ running, double* __restrict__ stat, int C, int c, double mean,
                                        double var, double invstd, double cnt, double momentum) {
    const double unb = cnt > 1.0 ? var * (cnt / (cnt - 1.0)) : var;
    running[c] = (float)((1.0 - momentum) * (double)running[c] + momentum * mean);
    running[C + c] = (float)((1.0 - momentum) * (double)running[C + c] + momentum * unb);
    stat[c] = mean;
    stat[C + c] = invstd;
}

// slice s of channel c: y = act(z(x)) (+ res) on the fp32 (meanf, istd).  Roundings of y: 3 (bn_z) + 1 with a residual
template <bool VEC>
__device__ __forceinline__ void bn_fwd_slice(const float* __restrict__ x, const float* __restrict__ res,
                                             const float* __restrict__ gamma, const float* __restrict__ beta,
                                             float* __restrict__ y, int N, int C, int HW, int chunk, int s, int c, int act,
                                             double mean, double invstd) {
    const float meanf = (float)mean, istd = (float)invstd;
    const float ga = gamma[c], be = beta[c];
    const float lo = act == ACT_NONE ? -INFINITY : 0.f;
    const float hi = act == ACT_RELU6 ? 6.f : INFINITY;
    // fmaxf / fminf return the operand that is not a NaN: the clamp alone would turn a NaN z into 0 (ReLU, ReLU6) or -inf
    // (none), where torch's relu, relu6 and batch_norm keep it.  Every other z takes the clamp it always took.
    auto f = [&](float v) {
        const float z = bn_z(v, meanf, istd, ga, be);
        return z != z ? z : fminf(fmaxf(z, lo), hi);
    };
    bn_walk<VEC>(N, C, HW, chunk, s, c, [&](long o) {
        if (VEC) {
            f32x4_t v = *reinterpret_cast<const f32x4_t*>(x + o);
            v[0] = f(v[0]); v[1] = f(v[1]); v[2] = f(v[2]); v[3] = f(v[3]);
            if (res) v += *reinterpret_cast<const f32x4_t*>(res + o);
            *reinterpret_cast<f32x4_t*>(y + o) = v;
        } else {
            float v = f(x[o]);
            if (res) v += res[o];
            y[o] = v;
        }
    });
}

// y = act(z(x)) (+ res).  TRAIN: the batch's statistics from the partials of bn_stats_kernel, combined in index order by
// every workgroup alike; slice 0 of a channel writes stat = [mean | invstd] x C (fp64) and moves the running pair
// (running = [mean | var] x C) as bn_apply_kernel does.  !TRAIN: the running pair is the statistics, nothing but y is written.
template <bool VEC, bool TRAIN>
__global__ __launch_bounds__(256) void bn_fwd_kernel(const float* __restrict__ x, const float* __restrict__ res,
                                                     const double2* __restrict__ part, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, float* __restrict__ running,
                                                     float* __restrict__ y, double* __restrict__ stat, int N, int C, int HW,
                                                     int chunk, int act, double momentum, double eps) {
    const int s = blockIdx.x, c = blockIdx.y, S = gridDim.x;
    double mean, invstd;
    if (TRAIN) {
        double sum = 0.0, sq = 0.0;
        for (int i = 0; i < S; ++i) {
            const double2 d = part[(long)c * S + i];
            sum += d.x;
            sq += d.y;
        }
        const double cnt = (double)N * (double)HW;
        double var;
        bn_moments(sum, sq, cnt, eps, mean, var, invstd);
        if (s == 0 && threadIdx.x == 0) bn_keep(running, stat, C, c, mean, var, invstd, cnt, momentum);
    } else {
        mean = (double)running[c];
        invstd = 1.0 / sqrt((double)running[C + c] + eps);
    }
    bn_fwd_slice<VEC>(x, res, gamma, beta, y, N, C, HW, chunk, s, c, act, mean, invstd);
}

// The synchronised forward: rows [W][2C + 2] = sum[C] | sumsq[C] | count | 0 of every rank, in rank order.  Every workgroup
// adds the W rows in rank order from 0.0 (W = 1: 0.0 + s == s, the plain kernel's bits), the cell count is the sum of the
// rows' counts; from there on bn_fwd_kernel<., true>'s own expressions.  Slice 0 of a channel keeps stat = mean[C] |
// invstd[C] | total count | 0 (channel 0 writes the tail) and moves the running pair.
template <bool VEC>
__global__ __launch_bounds__(256) void bn_sync_fwd_kernel(const float* __restrict__ x, const float* __restrict__ res,
                                                          const double* __restrict__ rows, int W,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          float* __restrict__ running, float* __restrict__ y,
                                                          double* __restrict__ stat, int N, int C, int HW, int chunk, int act,
                                                          double momentum, double eps) {
    const int s = blockIdx.x, c = blockIdx.y;
    const int RL = 2 * C + 2;
    double sum = 0.0, sq = 0.0, cnt = 0.0;
    for (int r = 0; r < W; ++r) {
        const double* row = rows + (long)r * RL;
        sum += row[c];
        sq += row[C + c];
        cnt += row[2 * C];
    }
    double mean, var, invstd;
    bn_moments(sum, sq, cnt, eps, mean, var, invstd);
    if (s == 0 && threadIdx.x == 0) {
        bn_keep(running, stat, C, c, mean, var, invstd, cnt, momentum);
        if (c == 0) {
            stat[2 * C] = cnt;
            stat[2 * C + 1] = 0.0;
        }
    }
    bn_fwd_slice<VEC>(x, res, gamma, beta, y, N, C, HW, chunk, s, c, act, mean, invstd);
}

// part [C][S] pairs -> one row: row[c] = the channel's S first members, row[C + c] its S second members, each added in
// index order from 0.0 (the order bn_fwd_kernel / bn_bwd_apply_kernel use); tail: row[2C] = cnt, row[2C + 1] = 0.
// One thread per channel: S <= 64 dependent adds
__global__ __launch_bounds__(256) void bn_row_kernel(const double2* __restrict__ part, int S, int C, double cnt, int tail,
                                                     double* __restrict__ row) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double a = 0.0, b = 0.0;
    for (int i = 0; i < S; ++i) {
        const double2 d = part[(long)c * S + i];
        a += d.x;
        b += d.y;
    }
    row[c] = a;
    row[C + c] = b;
    if (tail && c == 0) {
        row[2 * C] = cnt;
        row[2 * C + 1] = 0.0;
    }
}

// g = dy * act'(z), xhat = (x - mean) * invstd in fp64 from the kept pair: per-channel partial (sum g, sum g * xhat) in
// fp64, one per workgroup -- the twin of bn_stats_kernel
template <bool VEC>
__global__ __launch_bounds__(256) void bn_bwd_stats_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           const double* __restrict__ stat, double2* __restrict__ part,
                                                           int N, int C, int HW, int chunk, int act) {
    const int s = blockIdx.x, c = blockIdx.y, S = gridDim.x;
    const double mean = stat[c], invstd = stat[C + c];
    const float meanf = (float)mean, istd = (float)invstd;
    const float ga = gamma[c], be = beta[c];
    double sg = 0.0, sgx = 0.0;
    auto one = [&](float xv, float dv) {
        const double g = bn_pass(bn_z(xv, meanf, istd, ga, be), act) ? (double)dv : 0.0;
        sg += g;
        sgx += g * (((double)xv - mean) * invstd);
    };
    bn_walk<VEC>(N, C, HW, chunk, s, c, [&](long o) {
        if (VEC) {
            const f32x4_t xv = *reinterpret_cast<const f32x4_t*>(x + o);
            const f32x4_t dv = *reinterpret_cast<const f32x4_t*>(dy + o);
            one(xv[0], dv[0]); one(xv[1], dv[1]); one(xv[2], dv[2]); one(xv[3], dv[3]);
        } else {
            one(x[o], dy[o]);
        }
    });
    const double2 t = bn_block_sum(sg, sgx);
    if (threadIdx.x == 0) part[(long)c * S + s] = t;
}

// slice s of channel c: dx = gamma * invstd * (g - sum(g) / n - xhat * sum(g * xhat) / n), evaluated in fp64 on the fp32
// inputs and the kept fp64 pair and rounded ONCE; (sg, sgx) = (sum g, sum g * xhat) over the cnt cells of the channel
template <bool VEC>
__device__ __forceinline__ void bn_bwd_slice(const float* __restrict__ dy, const float* __restrict__ x,
                                             const float* __restrict__ gamma, const float* __restrict__ beta,
                                             const double* __restrict__ stat, float* __restrict__ dx, int N, int C, int HW,
                                             int chunk, int s, int c, int act, double sg, double sgx, double cnt) {
    const double mg = sg / cnt, mgx = sgx / cnt;
    const double mean = stat[c], invstd = stat[C + c];
    const float meanf = (float)mean, istd = (float)invstd;
    const float ga = gamma[c], be = beta[c];
    const double k = (double)ga * invstd;
    auto one = [&](float xv, float dv) {
        const double g = bn_pass(bn_z(xv, meanf, istd, ga, be), act) ? (double)dv : 0.0;
        const double xh = ((double)xv - mean) * invstd;
        return (float)(k * ((g - mg) - xh * mgx));
    };
    bn_walk<VEC>(N, C, HW, chunk, s, c, [&](long o) {
        if (VEC) {
            const f32x4_t xv = *reinterpret_cast<const f32x4_t*>(x + o);
            const f32x4_t dv = *reinterpret_cast<const f32x4_t*>(dy + o);
            *reinterpret_cast<f32x4_t*>(dx + o) = f32x4_t{one(xv[0], dv[0]), one(xv[1], dv[1]), one(xv[2], dv[2]),
                                                           one(xv[3], dv[3])};
        } else {
            dx[o] = one(x[o], dy[o]);
        }
    });
}

// dx by bn_bwd_slice; slice 0 of a channel writes dgamma = sum(g * xhat) and dbeta = sum(g), one rounding each.
// The partials are combined in index order by every workgroup alike -- the twin of bn_fwd_kernel.
template <bool VEC>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           const double* __restrict__ stat, const double2* __restrict__ part,
                                                           float* __restrict__ dx, float* __restrict__ dgamma,
                                                           float* __restrict__ dbeta, int N, int C, int HW, int chunk,
                                                           int act) {
    const int s = blockIdx.x, c = blockIdx.y, S = gridDim.x;
    double sg = 0.0, sgx = 0.0;
    for (int i = 0; i < S; ++i) {
        const double2 d = part[(long)c * S + i];
        sg += d.x;
        sgx += d.y;
    }
    if (s == 0 && threadIdx.x == 0) {
        dgamma[c] = (float)sgx;
        dbeta[c] = (float)sg;
    }
    const double cnt = (double)N * (double)HW;
    bn_bwd_slice<VEC>(dy, x, gamma, beta, stat, dx, N, C, HW, chunk, s, c, act, sg, sgx, cnt);
}

// The synchronised backward: rows [W][2C] = sum_g[C] | sum_gxhat[C] of every rank, added in rank order from 0.0 by every
// workgroup alike; n is the total count the forward kept in stat[2C].  dgamma / dbeta are THIS rank's row, rounded once
// (torch.nn.SyncBatchNorm's convention: averaging the parameter gradients over the ranks makes them global).
template <bool VEC>
__global__ __launch_bounds__(256) void bn_sync_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          const double* __restrict__ stat, const double* __restrict__ rows,
                                                          int W, int rank, float* __restrict__ dx, float* __restrict__ dgamma,
                                                          float* __restrict__ dbeta, int N, int C, int HW, int chunk,
                                                          int act) {
    const int s = blockIdx.x, c = blockIdx.y;
    double sg = 0.0, sgx = 0.0;
    for (int r = 0; r < W; ++r) {
        const double* row = rows + (long)r * 2 * C;
        sg += row[c];
        sgx += row[C + c];
    }
    if (s == 0 && threadIdx.x == 0) {
        const double* own = rows + (long)rank * 2 * C;
        dgamma[c] = (float)own[C + c];
        dbeta[c] = (float)own[c];
    }
    bn_bwd_slice<VEC>(dy, x, gamma, beta, stat, dx, N, C, HW, chunk, s, c, act, sg, sgx, stat[2 * C]);
}

void launch_bn_fwd(const float* x, const float* res, const double* part, const float* gamma, const float* beta,
                   float* running, float* y, double* stat, int N, int C, int HW, int act, bool training, double momentum,
                   double eps, hipStream_t s) {
    const BnCut k = bn_cut(N, C, HW);
    dim3 grid(k.S, C), block(256);
#define LP_GO(V, T)                                                                                                    \
    LP_LAUNCH((bn_fwd_kernel<V, T>), grid, block, 0, s, x, res, (const double2*)part, gamma, beta, running, y, stat, N, C, \
              HW, k.chunk, act, momentum, eps)
    if (k.vec) { if (training) LP_GO(true, true); else LP_GO(true, false); }
    else { if (training) LP_GO(false, true); else LP_GO(false, false); }
#undef LP_GO
}

void launch_bn_bwd(const float* dy, const float* x, const float* gamma, const float* beta, const double* stat, double* part,
                   float* dx, float* dgamma, float* dbeta, int N, int C, int HW, int act, hipStream_t s) {
    const BnCut k = bn_cut(N, C, HW);
    dim3 grid(k.S, C), block(256);
    if (k.vec) {
        LP_LAUNCH(bn_bwd_stats_kernel<true>, grid, block, 0, s, dy, x, gamma, beta, stat, (double2*)part, N, C, HW, k.chunk, act);
        LP_LAUNCH(bn_bwd_apply_kernel<true>, grid, block, 0, s, dy, x, gamma, beta, stat, (const double2*)part, dx, dgamma,
                  dbeta, N, C, HW, k.chunk, act);
    } else {
        LP_LAUNCH(bn_bwd_stats_kernel<false>, grid, block, 0, s, dy, x, gamma, beta, stat, (double2*)part, N, C, HW, k.chunk, act);
        LP_LAUNCH(bn_bwd_apply_kernel<false>, grid, block, 0, s, dy, x, gamma, beta, stat, (const double2*)part, dx, dgamma,
                  dbeta, N, C, HW, k.chunk, act);
    }
}

void launch_bn_row(const double* part, int S, int C, double cnt, bool tail, double* row, hipStream_t s) {
    LP_LAUNCH(bn_row_kernel, dim3((C + 255) / 256), dim3(256), 0, s, (const double2*)part, S, C, cnt, tail ? 1 : 0, row);
}

void launch_bn_sync_fwd(const float* x, const float* res, const double* rows, int W, const float* gamma, const float* beta,
                        float* running, float* y, double* stat, int N, int C, int HW, int act, double momentum, double eps,
                        hipStream_t s) {
    const BnCut k = bn_cut(N, C, HW);
    dim3 grid(k.S, C), block(256);
    if (k.vec)
        LP_LAUNCH(bn_sync_fwd_kernel<true>, grid, block, 0, s, x, res, rows, W, gamma, beta, running, y, stat, N, C, HW,
                  k.chunk, act, momentum, eps);
    else
        LP_LAUNCH(bn_sync_fwd_kernel<false>, grid, block, 0, s, x, res, rows, W, gamma, beta, running, y, stat, N, C, HW,
                  k.chunk, act, momentum, eps);
}

void launch_bn_sync_bwd_stats(const float* dy, const float* x, const float* gamma, const float* beta, const double* stat,
                              double* part, double* row, int N, int C, int HW, int act, hipStream_t s) {
    const BnCut k = bn_cut(N, C, HW);
    dim3 grid(k.S, C), block(256);
    if (k.vec)
        LP_LAUNCH(bn_bwd_stats_kernel<true>, grid, block, 0, s, dy, x, gamma, beta, stat, (double2*)part, N, C, HW, k.chunk, act);
    else
        LP_LAUNCH(bn_bwd_stats_kernel<false>, grid, block, 0, s, dy, x, gamma, beta, stat, (double2*)part, N, C, HW, k.chunk, act);
    launch_bn_row(part, k.S, C, 0.0, false, row, s);
}

void launch_bn_sync_bwd(const float* dy, const float* x, const float* gamma, const float* beta, const double* stat,
                        const double* rows, int W, int rank, float* dx, float* dgamma, float* dbeta, int N, int C, int HW,
                        int act, hipStream_t s) {
    const BnCut k = bn_cut(N, C, HW);
    dim3 grid(k.S, C), block(256);
    if (k.vec)
        LP_LAUNCH(bn_sync_bwd_kernel<true>, grid, block, 0, s, dy, x, gamma, beta, stat, rows, W, rank, dx, dgamma, dbeta, N,
                  C, HW, k.chunk, act);
    else
        LP_LAUNCH(bn_sync_bwd_kernel<false>, grid, block, 0, s, dy, x, gamma, beta, stat, rows, W, rank, dx, dgamma, dbeta, N,
                  C, HW, k.chunk, act);
}

// ====================================================================================== packing on the device
// w [Cout][Cin] -> the A fragments launch_pw reads, [ceil(M/32)][(K+1)/2][64]: lane l of k-pair kp holds A[32 blk + (l & 31)]
// [2 kp + (l >> 5)], zero beyond M or K (plan.cpp pack_pw).  transpose: A = W^T (M = Cin, K = Cout), the data gradient's
// weights.  zb: the zb_n zeros launch_pw takes as its bias (D-fragment order; all zeros in any order).
__global__ __launch_bounds__(256) void pw_pack_kernel(const float* __restrict__ w, int Cout, int Cin, int transpose,
                                                      float* __restrict__ wp, float* __restrict__ zb, int zb_n) {
    const int M = transpose ? Cin : Cout, K = transpose ? Cout : Cin;
    const int KP = (K + 1) >> 1;
    const long total = (long)((M + 31) >> 5) * KP * 64;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx < zb_n) zb[idx] = 0.f;
    if (idx >= total) return;
    const int l = (int)(idx & 63);
    const long q = idx >> 6;
    const int kp = (int)(q % KP), blk = (int)(q / KP);
    const int m = blk * 32 + (l & 31), k = 2 * kp + (l >> 5);
    float v = 0.f;
    if (m < M && k < K) v = transpose ? w[(long)k * Cin + m] : w[(long)m * Cin + k];
    wp[idx] = v;
}

// w [C][K*K] -> wdup [C][K*K][2] (every tap twice: plan.cpp pack_dw_dup) and the C zeros launch_dw takes as its bias
__global__ __launch_bounds__(256) void dw_pack_kernel(const float* __restrict__ w, int cnt, float* __restrict__ wdup,
                                                      float* __restrict__ zb, int C) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx < C) zb[idx] = 0.f;
    if (idx < cnt) {
        const float v = w[idx];
        wdup[2 * idx] = v;
        wdup[2 * idx + 1] = v;
    }
}

void launch_pw_pack(const float* w, int Cout, int Cin, bool transpose, float* wp, float* zb, hipStream_t s) {
    const int M = transpose ? Cin : Cout, K = transpose ? Cout : Cin;
    const int zb_n = ((M + 31) / 32) * 32;
    long total = (long)((M + 31) / 32) * ((K + 1) / 2) * 64;
    if (total < zb_n) total = zb_n;
    LP_LAUNCH(pw_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, w, Cout, Cin, transpose ? 1 : 0, wp, zb,
              zb_n);
}

void launch_dw_pack(const float* w, int C, int K, float* wdup, float* zb, hipStream_t s) {
    const int cnt = C * K * K;
    LP_LAUNCH(dw_pack_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, w, cnt, wdup, zb, C);
}

// out[i] = sum over the S slices of part[s * stride + i], i < count, in index order, in fp64, rounded once
__global__ __launch_bounds__(256) void slice_sum_kernel(const float* __restrict__ part, int S, int stride, int count,
                                                        float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    double a = 0.0;
    int s = 0;
    for (; s + 32 <= S; s += 32) {                      // 32 loads in flight, then their adds in index order
        float v[32];
#pragma unroll
        for (int j = 0; j < 32; ++j) v[j] = part[(long)(s + j) * stride + i];
#pragma unroll
        for (int j = 0; j < 32; ++j) a += (double)v[j];
    }
    for (; s < S; ++s) a += (double)part[(long)s * stride + i];
    out[i] = (float)a;
}

void launch_slice_sum(const float* part, int S, int stride, int count, float* out, hipStream_t s) {
    LP_LAUNCH(slice_sum_kernel, dim3((count + 255) / 256), dim3(256), 0, s, part, S, stride, count, out);
}

// ====================================================================================== 1x1: weight gradient
// dW[co][ci] = sum over the pixels g = n * HW + p of dY[n][co][p] * X[n][ci][p]: a GEMM whose reduction runs over the
// pixels.  One wave owns a 32 x 32 tile of dW for one slice of LP_PW_WGRAD_SLICE pixels (the four waves of a workgroup:
// the same 32 rows of dY, four neighbouring column blocks of X).  v_mfma_f32_32x32x2_f32 takes A[row = l & 31][k = l >> 5]
// and B[k = l >> 5][col = l & 31]; here k counts PIXELS: per step of 16 pixels lane l loads the 8 consecutive pixels
// g + 8 (l >> 5) .. + 7 of dY row co0 + (l & 31) and of X row ci0 + (l & 31) (two 16-byte loads each when the plane is a
// multiple of four floats) and feeds pixel e of both to MFMA e (the next step's loads fly under this step's MFMAs): which pixel pair an MFMA reduces is free as long as A
// and B agree.  Rows beyond Cout / Cin and pixels beyond the slice are zero operands read from a clamped address.
// part [slices][Cout][Cin] fp32.  NP = N * HW <= 2^31 - 256 (checked by the caller: the loop looks two steps ahead).
template <bool VEC>
__global__ __launch_bounds__(256) void pw_wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                       float* __restrict__ part, int HW, int Cout, int Cin, int NP) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int slice = blockIdx.x, cob = blockIdx.y, cib = blockIdx.z * 4 + wave;
    if (cib * 32 >= Cin) return;                                   // wave-uniform; no barrier below
    const int half = lane >> 5, r = lane & 31;
    const int co = cob * 32 + r, ci = cib * 32 + r;
    const bool co_ok = co < Cout, ci_ok = ci < Cin;
    const int coc = co_ok ? co : Cout - 1, cic = ci_ok ? ci : Cin - 1;
    const int g0 = slice * LP_PW_WGRAD_SLICE;
    const int g1 = min(g0 + LP_PW_WGRAD_SLICE, NP);
    f32x16_t acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    // operands of one step of 16 pixels from g; a step at or beyond the slice's end is all zeros read from a clamped address
    auto load = [&](int g, float (&a)[8], float (&b)[8]) {
        const int pg = g + 8 * half;
        if (VEC) {
            // HW, NP and the slice length are multiples of four: a quad lies inside one image and wholly inside or outside the slice
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int q = pg + 4 * h;
                const bool ok = q < g1;
                const int qc = ok ? q : g0;
                const int n = qc / HW, p = qc - n * HW;
                f32x4_t va = *reinterpret_cast<const f32x4_t*>(dy + ((long)n * Cout + coc) * HW + p);
                f32x4_t vb = *reinterpret_cast<const f32x4_t*>(x + ((long)n * Cin + cic) * HW + p);
                if (!(ok && co_ok)) va = f32x4_t{0.f, 0.f, 0.f, 0.f};
                if (!(ok && ci_ok)) vb = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int e = 0; e < 4; ++e) { a[4 * h + e] = va[e]; b[4 * h + e] = vb[e]; }
            }
        } else {
            const int qs = pg < g1 ? pg : g0;
            int n = qs / HW, p = qs - n * HW;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const bool ok = pg + e < g1;
                const float va = dy[((long)n * Cout + coc) * HW + p];
                const float vb = x[((long)n * Cin + cic) * HW + p];
                a[e] = ok && co_ok ? va : 0.f;
                b[e] = ok && ci_ok ? vb : 0.f;
                if (pg + e + 1 < g1) {                              // the next pixel exists: step to it (never past NP - 1)
                    if (++p == HW) { p = 0; ++n; }
                }
            }
        }
    };
    // two steps per turn, the operands of the next step loaded under the MFMAs of this one
    float a0[8], b0[8], a1[8], b1[8];
    load(g0, a0, b0);
    for (int g = g0; g < g1; g += 32) {
        load(g + 16, a1, b1);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[e], b0[e], acc, 0, 0, 0);
        load(g + 32, a0, b0);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[e], b1[e], acc, 0, 0, 0);
    }
    // D register i of lane l: row (i & 3) + 8 (i >> 2) + 4 (l >> 5), column l & 31
    float* pb = part + (long)slice * Cout * Cin;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int row = cob * 32 + (i & 3) + 8 * (i >> 2) + 4 * half;
        if (row < Cout && ci_ok) pb[(long)row * Cin + ci] = acc[i];
    }
}

int pw_wgrad_slices(long NP) { return (int)((NP + LP_PW_WGRAD_SLICE - 1) / LP_PW_WGRAD_SLICE); }

void launch_pw_wgrad(const float* dy, const float* x, float* part, float* dw, int N, int HW, int Cout, int Cin,
                     hipStream_t s) {
    const int NP = N * HW, S = pw_wgrad_slices(NP);
    const int cibs = (Cin + 31) / 32;
    dim3 grid(S, (Cout + 31) / 32, (cibs + 3) / 4), block(256);
    if ((HW & 3) == 0)
        LP_LAUNCH(pw_wgrad_kernel<true>, grid, block, 0, s, dy, x, part, HW, Cout, Cin, NP);
    else
        LP_LAUNCH(pw_wgrad_kernel<false>, grid, block, 0, s, dy, x, part, HW, Cout, Cin, NP);
    const int count = Cout * Cin;
    launch_slice_sum(part, S, count, count, dw, s);
}

// ====================================================================================== depthwise: data gradient
// dX[n][c][iy][ix] = sum over the taps (ky, kx) with iy + P - ky = S oy and ix + P - kx = S ox, (oy, ox) inside the
// output plane, of w[c][ky][kx] * dY[n][c][oy][ox]: a gather, one input cell per lane, taps in (ky, kx) order with one
// fused multiply-add each.  For S = 2 only the taps of the cell's own parity take part: ky = ((iy + P) & 1) + 2 j.
template <int K, int S>
__global__ __launch_bounds__(256) void dw_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                       float* __restrict__ dx, int C, int H, int W, int OH, int OW,
                                                       int tiles) {
    constexpr int P = K / 2, NT = (K + S - 1) / S;
    const int plane = blockIdx.x / tiles, t = blockIdx.x - plane * tiles;
    const int c = plane % C;
    const int idx = t * 256 + threadIdx.x;
    if (idx >= H * W) return;
    const int iy = idx / W, ix = idx - iy * W;
    const float* gp = dy + (long)plane * OH * OW;
    const float* wc = w + (long)c * K * K;
    const int ky0 = S == 1 ? 0 : ((iy + P) & 1), kx0 = S == 1 ? 0 : ((ix + P) & 1);
    float acc = 0.f;
#pragma unroll
    for (int jy = 0; jy < NT; ++jy) {
        const int ky = ky0 + S * jy;
        const int ty = iy + P - ky;
        const int oy = S == 1 ? ty : ty >> 1;
        const bool y_ok = ky < K && ty >= 0 && oy < OH;
#pragma unroll
        for (int jx = 0; jx < NT; ++jx) {
            const int kx = kx0 + S * jx;
            const int tx = ix + P - kx;
            const int ox = S == 1 ? tx : tx >> 1;
            const bool ok = y_ok && kx < K && tx >= 0 && ox < OW;
            const float g = gp[ok ? oy * OW + ox : 0];
            const float wv = wc[ok ? ky * K + kx : 0];
            acc = fmaf(ok ? wv : 0.f, ok ? g : 0.f, acc);
        }
    }
    dx[(long)plane * H * W + idx] = acc;
}

// ====================================================================================== depthwise: weight gradient
// dW[c][ky][kx] = sum over (n, oy, ox) of dY[n][c][oy][ox] * X[n][c][S oy - P + ky][S ox - P + kx].  A workgroup owns
// (channel, slice); a slice is LP_DW_WGRAD_SLICE units, a unit one 16x16 output tile of one image (unit = n * tiles +
// tile).  Per unit the haloed input tile (15 S + K)^2, zeros where the plane ends, is staged in LDS; lane (row, col) of
// the 256 holds its dY cell (zero outside the plane) and adds its K^2 products to K^2 fp32 accumulators, one fused
// multiply-add each, units in order.  Then the 256 lanes are reduced in a fixed tree (shuffles inside a wave, the four waves
// pairwise) -> part [slices][C][K*K] fp32.  A tap that only ever meets padding sums zeros: exactly zero.
template <int K, int S>
__global__ __launch_bounds__(256) void dw_wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                       float* __restrict__ part, int N, int C, int H, int W, int OH, int OW,
                                                       int tilesX, int tiles) {
    constexpr int P = K / 2, TI = 15 * S + K, RS = TI + 1, KK = K * K;
    __shared__ float tile[TI * RS];
    __shared__ float red[4][KK];
    const int slice = blockIdx.x, c = blockIdx.y;
    const int units = N * tiles;
    const int u0 = slice * LP_DW_WGRAD_SLICE, u1 = min(u0 + LP_DW_WGRAD_SLICE, units);
    const int row = threadIdx.x >> 4, col = threadIdx.x & 15;
    float acc[KK];
#pragma unroll
    for (int k = 0; k < KK; ++k) acc[k] = 0.f;
    for (int u = u0; u < u1; ++u) {
        const int n = u / tiles, t = u - n * tiles;
        const int ty = t / tilesX, tx = t - ty * tilesX;
        const float* xp = x + ((long)n * C + c) * H * W;
        const int iy0 = ty * 16 * S - P, ix0 = tx * 16 * S - P;
        for (int e = threadIdx.x; e < TI * TI; e += 256) {
            const int r = e / TI, q = e - r * TI;
            const int iy = iy0 + r, ix = ix0 + q;
            const bool ok = iy >= 0 && iy < H && ix >= 0 && ix < W;
            const float v = xp[ok ? iy * W + ix : 0];
            tile[r * RS + q] = ok ? v : 0.f;
        }
        const int oy = ty * 16 + row, ox = tx * 16 + col;
        const bool ok = oy < OH && ox < OW;
        const float gv = dy[((long)n * C + c) * OH * OW + (ok ? oy * OW + ox : 0)];
        const float g = ok ? gv : 0.f;
        __syncthreads();
        const float* tp = tile + (row * S) * RS + col * S;
#pragma unroll
        for (int ky = 0; ky < K; ++ky)
#pragma unroll
            for (int kx = 0; kx < K; ++kx) acc[ky * K + kx] = fmaf(g, tp[ky * RS + kx], acc[ky * K + kx]);
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < KK; ++k) {
        float v = acc[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < KK)
        part[((long)slice * C + c) * KK + threadIdx.x] =
            (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

int dw_wgrad_slices(int N, int OH, int OW) {
    const long units = (long)N * ((OH + 15) / 16) * ((OW + 15) / 16);
    return (int)((units + LP_DW_WGRAD_SLICE - 1) / LP_DW_WGRAD_SLICE);
}

template <int K, int S>
static void dw_backward_t(const float* dy, const float* x, const float* w, float* dx, float* part, float* dw, int N, int C,
                          int H, int W, hipStream_t s) {
    const int OH = (H - 1) / S + 1, OW = (W - 1) / S + 1;
    if (dx) {
        const int tiles = (H * W + 255) / 256;
        LP_LAUNCH((dw_dgrad_kernel<K, S>), dim3((unsigned)(N * C * tiles)), dim3(256), 0, s, dy, w, dx, C, H, W, OH, OW, tiles);
    }
    if (dw) {
        const int tilesX = (OW + 15) / 16, tiles = tilesX * ((OH + 15) / 16);
        const int SL = dw_wgrad_slices(N, OH, OW);
        LP_LAUNCH((dw_wgrad_kernel<K, S>), dim3(SL, C), dim3(256), 0, s, dy, x, part, N, C, H, W, OH, OW, tilesX, tiles);
        const int count = C * K * K;
        launch_slice_sum(part, SL, count, count, dw, s);
    }
}

void launch_dw_backward(const float* dy, const float* x, const float* w, float* dx, float* part, float* dw, int N, int C,
                        int H, int W, int K, int S, hipStream_t s) {
    if (K == 3 && S == 1) dw_backward_t<3, 1>(dy, x, w, dx, part, dw, N, C, H, W, s);
    else if (K == 3 && S == 2) dw_backward_t<3, 2>(dy, x, w, dx, part, dw, N, C, H, W, s);
    else if (K == 5 && S == 1) dw_backward_t<5, 1>(dy, x, w, dx, part, dw, N, C, H, W, s);
    else if (K == 5 && S == 2) dw_backward_t<5, 2>(dy, x, w, dx, part, dw, N, C, H, W, s);
    else if (K == 7 && S == 1) dw_backward_t<7, 1>(dy, x, w, dx, part, dw, N, C, H, W, s);
    else if (K == 7 && S == 2) dw_backward_t<7, 2>(dy, x, w, dx, part, dw, N, C, H, W, s);
}

}  // namespace lp
