// The LitePose training loss of one stage (lp_pose_loss; include/litepose_amd.h "training loss"):
//   lib/core/loss.py:30-39     HeatmapLoss.forward        (heat_partial_kernel + loss_finish_kernel)
//   lib/core/loss.py:95-149    AELoss.batchTagLoss        (loss_finish_kernel)
//   lib/core/loss.py:277-315   MultiLossFactory.forward   (the channel split and the factors)
// fp32 inputs widened to fp64, every sum in a fixed order (no atomics: two runs give the same bits), one rounding to fp32
// per result.  Compiled without FMA contraction, so that a product and the sum it goes into round separately, as in the
// plain fp64 restatement the tests hold this to.
//
//   heat_partial_kernel  the streaming read: a workgroup per strip of LOSS_STRIP floats of one (image, joint) plane of the
//                        prediction, the target and the image's mask -> one fp64 partial in the workspace.  16-byte loads
//                        when the plane is a multiple of four floats and the three bases are 16-byte aligned
//   loss_finish_kernel   a workgroup per image: adds the image's J * S partials in index order, and evaluates the pull and
//                        push terms of the image from its [M,J,2] joints (one person per lane of wave 0)
#include "kernels.h"

namespace lp {

namespace {

// fixed-order sum of one value per thread of a 256-thread workgroup; the result is valid in thread 0
__device__ __forceinline__ double block_sum256(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

__device__ __forceinline__ double sq_err(float p, float g, float m) {
    const double d = (double)p - (double)g;
    return (d * d) * (double)m;
}

}  // namespace

// blockIdx.x = (n * J + j) * S + s.  pred: d_out [N,C,R,R] (channel j < J), gt [N,J,R,R], mask [N,R,R].
template <bool VEC>
__global__ __launch_bounds__(256) void heat_partial_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                           const float* __restrict__ mask, int C, int J, int RR, int S,
                                                           double* __restrict__ partial) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const long b = blockIdx.x;
    const int s = (int)(b % S);
    const long nj = b / S;
    const int j = (int)(nj % J);
    const long n = nj / J;
    const int base = s * LOSS_STRIP;
    const int len = min(LOSS_STRIP, RR - base);
    const float* p = pred + (n * C + j) * RR + base;
    const float* g = gt + (n * J + j) * RR + base;
    const float* m = mask + n * RR + base;
    double acc = 0.0;
    if (VEC) {
        const float4* p4 = reinterpret_cast<const float4*>(p);
        const float4* g4 = reinterpret_cast<const float4*>(g);
        const float4* m4 = reinterpret_cast<const float4*>(m);
        const int units = len >> 2;
#pragma unroll 4
        for (int u = tid; u < units; u += 256) {
            const float4 a = p4[u], t = g4[u], k = m4[u];
            acc += sq_err(a.x, t.x, k.x);
            acc += sq_err(a.y, t.y, k.y);
            acc += sq_err(a.z, t.z, k.z);
            acc += sq_err(a.w, t.w, k.w);
        }
    } else {
        for (int u = tid; u < len; u += 256) acc += sq_err(p[u], g[u], m[u]);
    }
    const double tot = block_sum256(acc, red);
    if (tid == 0) partial[b] = tot;
}

// blockIdx.x = image n.  partial == nullptr: no heatmap term; tag_offset < 0: no tag terms.
__global__ __launch_bounds__(256) void loss_finish_kernel(const double* __restrict__ partial, int JS, double heat_count, double heat_factor,
                                                          const float* __restrict__ out, int C, int RR, int tag_offset,
                                                          const int* __restrict__ joints, int M, int J, int loss_type,
                                                          double push_factor, double pull_factor,
                                                          float* __restrict__ heat_loss, float* __restrict__ push_out,
                                                          float* __restrict__ pull_out) {
    __shared__ double red[256];
    __shared__ double s_mean[64], s_pull[64], s_row[64];
    __shared__ int s_has[64];
    const int tid = threadIdx.x;
    const int n = blockIdx.x;
    if (partial) {
        const double* q = partial + (long)n * JS;
        double acc = 0.0;
        for (int i = tid; i < JS; i += 256) acc += q[i];
        const double tot = block_sum256(acc, red);
        if (tid == 0) heat_loss[n] = (float)((tot / heat_count) * heat_factor);
    }
    if (tag_offset < 0) return;
    const float* tagmap = out + ((long)n * C + tag_offset) * RR;
    const long limit = (long)(C - tag_offset) * RR;
    if (tid < 64) {
        double mean = 0.0, pull = 0.0;
        int cnt = 0;
        if (tid < M) {
            const int* jp = joints + ((long)n * M + tid) * J * 2;
            double sum = 0.0;
            for (int k = 0; k < J; ++k) {
                const int idx = jp[2 * k];
                if (jp[2 * k + 1] > 0 && idx >= 0 && idx < limit) {
                    sum += (double)tagmap[idx];
                    ++cnt;
                }
            }
            if (cnt > 0) {
                mean = sum / (double)cnt;
                double sq = 0.0;
                for (int k = 0; k < J; ++k) {
                    const int idx = jp[2 * k];
                    if (jp[2 * k + 1] > 0 && idx >= 0 && idx < limit) {
                        const double d = (double)tagmap[idx] - mean;
                        sq += d * d;
                    }
                }
                pull = sq / (double)cnt;
            }
        }
        s_mean[tid] = mean;
        s_pull[tid] = pull;
        s_has[tid] = cnt > 0;
    }
    __syncthreads();
    if (tid < 64) {                                  // row p of the [M,M] push matrix, columns in order
        double row = 0.0;
        if (tid < M && s_has[tid]) {
            const double mp = s_mean[tid];
            for (int q = 0; q < M; ++q) {
                if (!s_has[q]) continue;
                const double d = mp - s_mean[q];
                if (loss_type == 0) {
                    row += exp(-(d * d));
                } else {
                    const double t = 1.0 - fabs(d);
                    row += t > 0.0 ? t : 0.0;
                }
            }
        }
        s_row[tid] = row;
    }
    __syncthreads();
    if (tid == 0) {
        int persons = 0;
        double pull = 0.0, push = 0.0;
        for (int p = 0; p < M; ++p) {
            persons += s_has[p];
            pull += s_pull[p];
            push += s_row[p];
        }
        const double pc = persons == 0 ? 1.0 : (double)persons;
        pull = pull / pc;
        if (persons < 2) {
            push = 0.0;
        } else {
            double den = (pc - 1.0) * pc;
            den = den < 1.0 ? 1.0 : den;
            push = 0.5 * (push - pc) / den;
        }
        push_out[n] = (float)(push * push_factor);
        pull_out[n] = (float)(pull * pull_factor);
    }
}

void launch_heat_partial(const float* pred, const float* gt, const float* mask, int N, int C, int J, int R, int S,
                         double* partial, hipStream_t s) {
    const int RR = R * R;
    const bool vec = (RR & 3) == 0 && ((((uintptr_t)pred) | ((uintptr_t)gt) | ((uintptr_t)mask)) & 15) == 0;
    const unsigned grid = (unsigned)((long)N * J * S);
    if (vec)
        hipLaunchKernelGGL(heat_partial_kernel<true>, dim3(grid), dim3(256), 0, s, pred, gt, mask, C, J, RR, S, partial);
    else
        hipLaunchKernelGGL(heat_partial_kernel<false>, dim3(grid), dim3(256), 0, s, pred, gt, mask, C, J, RR, S, partial);
}

void launch_loss_finish(const double* partial, int N, int JS, double heat_count, double heat_factor, const float* out, int C, int R,
                        int tag_offset, const int* joints, int M, int J, int loss_type, double push_factor,
                        double pull_factor, float* heat_loss, float* push_out, float* pull_out, hipStream_t s) {
    hipLaunchKernelGGL(loss_finish_kernel, dim3(N), dim3(256), 0, s, partial, JS, heat_count, heat_factor, out, C, R * R, tag_offset,
                       joints, M, J, loss_type, push_factor, pull_factor, heat_loss, push_out, pull_out);
}

}  // namespace lp
