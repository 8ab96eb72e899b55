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
//
// and its gradient with respect to the stage output (lp_pose_loss_grad), in the same arithmetic:
//   heat_grad_kernel     the streaming write: a workgroup per strip of every (image, channel) plane of grad_out.  A heatmap
//                        plane reads the prediction, the target and the mask and writes k_n * ((p - g) * m); every other
//                        plane is written with zeros.  16-byte loads and stores under the rule above, grad_out included
//   tag_grad_kernel      a workgroup per image, after the streaming kernel on the same stream: every slot's (index, tag) into
//                        LDS, one slot per thread; means and counts added as loss_finish_kernel adds them; one push
//                        derivative per person (one person per lane, columns in order); every slot's fp64 contribution in
//                        LDS; and one store per cell by the first slot that names it, which adds the later slots of that
//                        cell in slot order (no atomics)
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
                    row += t < 0.0 ? 0.0 : t;                // a NaN gap stays in the sum, as torch.clamp(min=0) keeps it
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

// blockIdx.x = (n * C + c) * S + s.  Planes c < JH are heatmap planes (JH = 0: none); g_heat [N], the upstream gradient.
template <bool VEC>
__global__ __launch_bounds__(256) void heat_grad_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                        const float* __restrict__ mask, const float* __restrict__ g_heat,
                                                        int C, int JH, int J, int RR, int S, double heat_factor,
                                                        double heat_count, float* __restrict__ grad) {
    const int tid = threadIdx.x;
    const long b = blockIdx.x;
    const int s = (int)(b % S);
    const long nc = b / S;
    const int c = (int)(nc % C);
    const long n = nc / C;
    const int base = s * LOSS_STRIP;
    const int len = min(LOSS_STRIP, RR - base);
    float* o = grad + nc * RR + base;
    if (c >= JH) {                                   // outside the heatmap term: zeros (tag_grad_kernel fills its cells later)
        if (VEC) {
            float4* o4 = reinterpret_cast<float4*>(o);
            const int units = len >> 2;
#pragma unroll 4
            for (int u = tid; u < units; u += 256) o4[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            for (int u = tid; u < len; u += 256) o[u] = 0.f;
        }
        return;
    }
    const double k = (((double)g_heat[n] * heat_factor) * 2.0) / heat_count;
    const float* p = pred + nc * RR + base;
    const float* g = gt + (n * J + c) * RR + base;
    const float* m = mask + n * RR + base;
    if (VEC) {
        const float4* p4 = reinterpret_cast<const float4*>(p);
        const float4* g4 = reinterpret_cast<const float4*>(g);
        const float4* m4 = reinterpret_cast<const float4*>(m);
        float4* o4 = reinterpret_cast<float4*>(o);
        const int units = len >> 2;
#pragma unroll 4
        for (int u = tid; u < units; u += 256) {
            const float4 a = p4[u], t = g4[u], w = m4[u];
            float4 r;
            r.x = (float)(k * (((double)a.x - (double)t.x) * (double)w.x));
            r.y = (float)(k * (((double)a.y - (double)t.y) * (double)w.y));
            r.z = (float)(k * (((double)a.z - (double)t.z) * (double)w.z));
            r.w = (float)(k * (((double)a.w - (double)t.w) * (double)w.w));
            o4[u] = r;
        }
    } else {
        for (int u = tid; u < len; u += 256) o[u] = (float)(k * (((double)p[u] - (double)g[u]) * (double)m[u]));
    }
}

constexpr int TAG_SLOTS = 64 * 32;                   // M * J at most

// one table entry `key` at slot j against the scanning slot i of the same cell: an earlier one takes the cell away, a later
// one is added to its sum
__device__ __forceinline__ void tag_cell_hit(int key, int k, int j, int i, const double* val, bool& owner, double& sum) {
    if (k != key) return;
    if (j < i) owner = false;
    else if (j > i) sum += val[j];
}

// blockIdx.x = image n.  g_push / g_pull [N] or nullptr (a term without an upstream gradient adds nothing); at least one
// is given.  Writes only the cells of grad that a counting slot names; heat_grad_kernel has zeroed the rest.
__global__ __launch_bounds__(256) void tag_grad_kernel(const float* __restrict__ out, int C, int RR, int tag_offset,
                                                       const int* __restrict__ joints, int M, int J, int loss_type,
                                                       double push_factor, double pull_factor,
                                                       const float* __restrict__ g_push, const float* __restrict__ g_pull,
                                                       float* __restrict__ grad) {
    __shared__ double s_val[TAG_SLOTS];              // the slot's tag, then its contribution to its cell
    __shared__ __attribute__((aligned(16))) int s_idx[TAG_SLOTS];    // the slot's cell, -1 for a slot that does not count
    __shared__ double s_mean[64], s_dsum[64];
    __shared__ int s_cnt[64];
    const int tid = threadIdx.x;
    const int n = blockIdx.x;
    const float* tagmap = out + ((long)n * C + tag_offset) * RR;
    float* gmap = grad + ((long)n * C + tag_offset) * RR;
    const long limit = (long)(C - tag_offset) * RR;
    const int* jn = joints + (long)n * M * J * 2;
    const int slots = M * J;
    const int padded = (slots + 15) & ~15;           // the scan below reads 16 entries at a time; TAG_SLOTS is a multiple
    const float up_push = g_push ? g_push[n] : 0.f;  // loaded here, used after the means: off the critical path
    const float up_pull = g_pull ? g_pull[n] : 0.f;
    for (int i = tid; i < padded; i += 256) {        // every slot's cell and tag, one slot per thread
        int key = -1;
        double t = 0.0;
        if (i < slots) {
            const int idx = jn[2 * i];
            if (jn[2 * i + 1] > 0 && idx >= 0 && idx < limit) {
                key = idx;
                t = (double)tagmap[idx];
            }
        }
        s_idx[i] = key;
        s_val[i] = t;
    }
    __syncthreads();
    if (tid < 64) {                                  // the person's count and mean, added as loss_finish_kernel adds them
        double mean = 0.0;
        int cnt = 0;
        if (tid < M) {
            double sum = 0.0;
            for (int k = 0; k < J; ++k) {
                if (s_idx[tid * J + k] >= 0) {
                    sum += s_val[tid * J + k];
                    ++cnt;
                }
            }
            if (cnt > 0) mean = sum / (double)cnt;
        }
        s_mean[tid] = mean;
        s_cnt[tid] = cnt;
    }
    __syncthreads();
    int persons = 0;
    for (int p = 0; p < M; ++p) persons += s_cnt[p] > 0;
    const double pc = persons == 0 ? 1.0 : (double)persons;
    double den = (pc - 1.0) * pc;
    den = den < 1.0 ? 1.0 : den;
    const bool push_on = g_push != nullptr && persons >= 2;
    if (tid < 64) {                                  // D_p: the derivative of row p and column p of the push matrix
        double dsum = 0.0;
        if (push_on && tid < M && s_cnt[tid] > 0) {
            const double mp = s_mean[tid];
            for (int q = 0; q < M; ++q) {
                if (s_cnt[q] <= 0) continue;
                const double d = mp - s_mean[q];
                if (loss_type == 0) {
                    dsum += (-2.0 * d) * exp(-(d * d));
                } else if (fabs(d) < 1.0) {
                    dsum += d > 0.0 ? -1.0 : (d < 0.0 ? 1.0 : 0.0);
                }
            }
        }
        s_dsum[tid] = dsum;
    }
    __syncthreads();
    const double wpull = g_pull ? ((double)up_pull * pull_factor) * 2.0 : 0.0;
    const double wpush = push_on ? (double)up_push * push_factor : 0.0;
    for (int i = tid; i < slots; i += 256) {         // the slot's tag becomes its contribution (its own entry only)
        if (s_idx[i] < 0) continue;
        const int p = i / J;
        const double cnt = (double)s_cnt[p];
        double v = 0.0;
        if (g_pull) v = (wpull * (s_val[i] - s_mean[p])) / (cnt * pc);
        if (push_on) v += (wpush * s_dsum[p]) / (den * cnt);
        s_val[i] = v;
    }
    __syncthreads();
    const int4* idx4 = reinterpret_cast<const int4*>(s_idx);
    for (int i = tid; i < slots; i += 256) {         // every lane of a wave reads the same entries: broadcast reads
        const int key = s_idx[i];
        if (key < 0) continue;
        bool owner = true;
        double sum = s_val[i];
        for (int j = 0; j < padded; j += 16) {
            const int4 a = idx4[j >> 2], b = idx4[(j >> 2) + 1], c = idx4[(j >> 2) + 2], d = idx4[(j >> 2) + 3];
            const bool hit = a.x == key || a.y == key || a.z == key || a.w == key || b.x == key || b.y == key ||
                             b.z == key || b.w == key || c.x == key || c.y == key || c.z == key || c.w == key ||
                             d.x == key || d.y == key || d.z == key || d.w == key;
            if (!hit) continue;
            tag_cell_hit(key, a.x, j, i, s_val, owner, sum);
            tag_cell_hit(key, a.y, j + 1, i, s_val, owner, sum);
            tag_cell_hit(key, a.z, j + 2, i, s_val, owner, sum);
            tag_cell_hit(key, a.w, j + 3, i, s_val, owner, sum);
            tag_cell_hit(key, b.x, j + 4, i, s_val, owner, sum);
            tag_cell_hit(key, b.y, j + 5, i, s_val, owner, sum);
            tag_cell_hit(key, b.z, j + 6, i, s_val, owner, sum);
            tag_cell_hit(key, b.w, j + 7, i, s_val, owner, sum);
            tag_cell_hit(key, c.x, j + 8, i, s_val, owner, sum);
            tag_cell_hit(key, c.y, j + 9, i, s_val, owner, sum);
            tag_cell_hit(key, c.z, j + 10, i, s_val, owner, sum);
            tag_cell_hit(key, c.w, j + 11, i, s_val, owner, sum);
            tag_cell_hit(key, d.x, j + 12, i, s_val, owner, sum);
            tag_cell_hit(key, d.y, j + 13, i, s_val, owner, sum);
            tag_cell_hit(key, d.z, j + 14, i, s_val, owner, sum);
            tag_cell_hit(key, d.w, j + 15, i, s_val, owner, sum);
        }
        if (owner) gmap[key] = (float)sum;
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

void launch_heat_grad(const float* pred, const float* gt, const float* mask, const float* g_heat, int N, int C, int JH, int J,
                      int R, int S, double heat_factor, float* grad, hipStream_t s) {
    const int RR = R * R;
    const bool vec = (RR & 3) == 0 &&
                     ((((uintptr_t)pred) | ((uintptr_t)gt) | ((uintptr_t)mask) | ((uintptr_t)grad)) & 15) == 0;
    const unsigned grid = (unsigned)((long)N * C * S);
    const double count = (double)J * R * R;
    if (vec)
        hipLaunchKernelGGL(heat_grad_kernel<true>, dim3(grid), dim3(256), 0, s, pred, gt, mask, g_heat, C, JH, J, RR, S,
                           heat_factor, count, grad);
    else
        hipLaunchKernelGGL(heat_grad_kernel<false>, dim3(grid), dim3(256), 0, s, pred, gt, mask, g_heat, C, JH, J, RR, S,
                           heat_factor, count, grad);
}

void launch_tag_grad(const float* out, int N, int C, int R, int tag_offset, const int* joints, int M, int J, int loss_type,
                     double push_factor, double pull_factor, const float* g_push, const float* g_pull, float* grad,
                     hipStream_t s) {
    hipLaunchKernelGGL(tag_grad_kernel, dim3(N), dim3(256), 0, s, out, C, R * R, tag_offset, joints, M, J, loss_type,
                       push_factor, pull_factor, g_push, g_pull, grad);
}

}  // namespace lp
