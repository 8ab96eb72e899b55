// The optimizer updates (include/litepose_amd.h, "optimizers"): Adam and SGD over a list of tensors.  One launch per
// argument chunk (optim.h): the chunk travels BY VALUE in the launch's arguments -- pointers, lengths and the map from a
// workgroup to (tensor, block of LP_OPTIM_BLOCK_ELEMS elements) -- so nothing is copied to the device and a captured graph
// holds everything.  A workgroup owns its block alone: no LDS, no atomics, every element is read and written by one lane.
// Compiled with -ffp-contract=off: every product and sum below rounds on its own, as the header's formulas are written.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "optim.h"

namespace lp {

namespace {

// b^t for an integer t >= 1 by squaring, fp64: at most 2 * 31 products, the same on every lane
__device__ inline double powi(double b, unsigned t) {
    double r = 1.0;
    while (t) {
        if (t & 1u) r *= b;
        b *= b;
        t >>= 1;
    }
    return r;
}

struct AdamCoef {
    float b1, omb1, b2, omb2, eps, wd, step_size, rsq2;     // step_size = lr / (1 - b1^t), rsq2 = sqrt(1 - b2^t)
    bool decay;
};

__device__ inline void adam_one(float& p, float g, float& m, float& v, const AdamCoef& c) {
    if (c.decay) g = g + c.wd * p;
    m = c.b1 * m + c.omb1 * g;
    v = c.b2 * v + (c.omb2 * g) * g;
    const float denom = sqrtf(v) / c.rsq2 + c.eps;
    p = p - c.step_size * (m / denom);
}

struct SgdCoef {
    float lr, mu, wd;
    bool decay, nesterov;
};

template <bool MOM>
__device__ inline void sgd_one(float& p, float g, float& buf, const SgdCoef& c) {
    if (c.decay) g = g + c.wd * p;
    float d = g;
    if (MOM) {
        buf = c.mu * buf + g;
        d = c.nesterov ? g + c.mu * buf : buf;
    }
    p = p - c.lr * d;
}

__device__ inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

// grid = chunk.blocks workgroups of OPTIM_THREADS lanes; workgroup b updates block (map & 0xffffff) of tensor (map >> 24)
__global__ __launch_bounds__(OPTIM_THREADS) void adam_kernel(const OptimChunk ck, const float* __restrict__ step,
                                                             const double* __restrict__ lr, double beta1, double beta2,
                                                             double eps, double weight_decay) {
    const uint32_t e = ck.map[blockIdx.x];
    const int t = (int)(e >> 24);
    const int64_t n = ck.numel[t];
    const int64_t e0 = (int64_t)(e & 0xffffffu) * LP_OPTIM_BLOCK_ELEMS;
    float* __restrict__ p = ck.ptr[0][t];
    const float* __restrict__ g = ck.ptr[1][t];
    float* __restrict__ m = ck.ptr[2][t];
    float* __restrict__ v = ck.ptr[3][t];

    const unsigned tt = (unsigned)step[ck.first + t] + 1u;                    // the step value from before the call
    AdamCoef c;
    c.b1 = (float)beta1, c.omb1 = (float)(1.0 - beta1), c.b2 = (float)beta2, c.omb2 = (float)(1.0 - beta2);
    c.eps = (float)eps, c.wd = (float)weight_decay, c.decay = weight_decay != 0.0;
    c.step_size = (float)(*lr / (1.0 - powi(beta1, tt)));
    c.rsq2 = (float)sqrt(1.0 - powi(beta2, tt));

    if (al16(p) && al16(g) && al16(m) && al16(v)) {
#pragma unroll
        for (int it = 0; it < LP_OPTIM_BLOCK_ELEMS / (4 * OPTIM_THREADS); ++it) {
            const int64_t i = e0 + (int64_t)(it * OPTIM_THREADS + (int)threadIdx.x) * 4;
            if (i + 4 <= n) {
                float4 P = *reinterpret_cast<const float4*>(p + i), G = *reinterpret_cast<const float4*>(g + i);
                float4 M = *reinterpret_cast<const float4*>(m + i), V = *reinterpret_cast<const float4*>(v + i);
                adam_one(P.x, G.x, M.x, V.x, c);
                adam_one(P.y, G.y, M.y, V.y, c);
                adam_one(P.z, G.z, M.z, V.z, c);
                adam_one(P.w, G.w, M.w, V.w, c);
                *reinterpret_cast<float4*>(p + i) = P;
                *reinterpret_cast<float4*>(m + i) = M;
                *reinterpret_cast<float4*>(v + i) = V;
            } else {
                for (int64_t j = i; j < n; ++j) {                              // the ragged tail: at most 3 elements
                    float P = p[j], M = m[j], V = v[j];
                    adam_one(P, g[j], M, V, c);
                    p[j] = P, m[j] = M, v[j] = V;
                }
            }
        }
    } else {
#pragma unroll 4
        for (int it = 0; it < LP_OPTIM_BLOCK_ELEMS / OPTIM_THREADS; ++it) {
            const int64_t j = e0 + it * OPTIM_THREADS + (int)threadIdx.x;
            if (j < n) {
                float P = p[j], M = m[j], V = v[j];
                adam_one(P, g[j], M, V, c);
                p[j] = P, m[j] = M, v[j] = V;
            }
        }
    }
}

// after every adam_kernel of the call (stream order): the counters move once, whatever the number of chunks a tensor spans
__global__ __launch_bounds__(OPTIM_THREADS) void step_advance_kernel(float* __restrict__ step, int count) {
    const int i = (int)(blockIdx.x * OPTIM_THREADS + threadIdx.x);
    if (i < count) step[i] = step[i] + 1.0f;
}

template <bool MOM>
__global__ __launch_bounds__(OPTIM_THREADS) void sgd_kernel(const OptimChunk ck, const double* __restrict__ lr, double momentum,
                                                            double weight_decay, int nesterov) {
    const uint32_t e = ck.map[blockIdx.x];
    const int t = (int)(e >> 24);
    const int64_t n = ck.numel[t];
    const int64_t e0 = (int64_t)(e & 0xffffffu) * LP_OPTIM_BLOCK_ELEMS;
    float* __restrict__ p = ck.ptr[0][t];
    const float* __restrict__ g = ck.ptr[1][t];
    float* __restrict__ b = MOM ? ck.ptr[2][t] : nullptr;

    SgdCoef c;
    c.lr = (float)*lr, c.mu = (float)momentum, c.wd = (float)weight_decay;
    c.decay = weight_decay != 0.0, c.nesterov = nesterov != 0;

    if (al16(p) && al16(g) && al16(b)) {
#pragma unroll
        for (int it = 0; it < LP_OPTIM_BLOCK_ELEMS / (4 * OPTIM_THREADS); ++it) {
            const int64_t i = e0 + (int64_t)(it * OPTIM_THREADS + (int)threadIdx.x) * 4;
            if (i + 4 <= n) {
                float4 P = *reinterpret_cast<const float4*>(p + i), G = *reinterpret_cast<const float4*>(g + i);
                float4 B = make_float4(0.f, 0.f, 0.f, 0.f);
                if (MOM) B = *reinterpret_cast<const float4*>(b + i);
                sgd_one<MOM>(P.x, G.x, B.x, c);
                sgd_one<MOM>(P.y, G.y, B.y, c);
                sgd_one<MOM>(P.z, G.z, B.z, c);
                sgd_one<MOM>(P.w, G.w, B.w, c);
                *reinterpret_cast<float4*>(p + i) = P;
                if (MOM) *reinterpret_cast<float4*>(b + i) = B;
            } else {
                for (int64_t j = i; j < n; ++j) {
                    float P = p[j], B = MOM ? b[j] : 0.f;
                    sgd_one<MOM>(P, g[j], B, c);
                    p[j] = P;
                    if (MOM) b[j] = B;
                }
            }
        }
    } else {
#pragma unroll 4
        for (int it = 0; it < LP_OPTIM_BLOCK_ELEMS / OPTIM_THREADS; ++it) {
            const int64_t j = e0 + it * OPTIM_THREADS + (int)threadIdx.x;
            if (j < n) {
                float P = p[j], B = MOM ? b[j] : 0.f;
                sgd_one<MOM>(P, g[j], B, c);
                p[j] = P;
                if (MOM) b[j] = B;
            }
        }
    }
}

void launch_adam_chunk(const OptimChunk& ck, const float* step, const double* lr, double beta1, double beta2, double eps,
                       double weight_decay, hipStream_t s) {
    hipLaunchKernelGGL(adam_kernel, dim3(ck.blocks), dim3(OPTIM_THREADS), 0, s, ck, step, lr, beta1, beta2, eps, weight_decay);
}

void launch_step_advance(float* step, int count, hipStream_t s) {
    hipLaunchKernelGGL(step_advance_kernel, dim3((count + OPTIM_THREADS - 1) / OPTIM_THREADS), dim3(OPTIM_THREADS), 0, s, step,
                       count);
}

void launch_sgd_chunk(const OptimChunk& ck, bool with_momentum, const double* lr, double momentum, double weight_decay,
                      int nesterov, hipStream_t s) {
    if (with_momentum)
        hipLaunchKernelGGL(sgd_kernel<true>, dim3(ck.blocks), dim3(OPTIM_THREADS), 0, s, ck, lr, momentum, weight_decay, nesterov);
    else
        hipLaunchKernelGGL(sgd_kernel<false>, dim3(ck.blocks), dim3(OPTIM_THREADS), 0, s, ck, lr, momentum, weight_decay, nesterov);
}

}  // namespace lp
