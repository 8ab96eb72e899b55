// Supernet training (include/litepose_amd.h, "supernet training"): the sampled sub-network's parameters gathered from
// the supernet's tensors into one packed buffer, their gradients scattered back into full-size tensors, and the
// random-resolution resize of a batch.  Compiled without FMA contraction: the window transform and its gradients round
// every product and every sum on their own, in the order the header states.
//
// Gather and scatter run one thread per group of four consecutive elements of the buffer they WRITE (the packed
// sub-network buffer, the packed full-gradient buffer); the thread finds the descriptor that owns its group by a binary
// search over the table's offsets, staged in LDS.  Offsets are multiples of 64 elements, so a group never straddles two
// descriptors.  Every store index is below the element count passed by value, whatever the table says.
#include "supertrain.h"

namespace lp {

constexpr int TPB = 256;

__device__ __forceinline__ int64_t a64(int64_t n) { return (n + 63) & ~(int64_t)63; }

__device__ __forceinline__ bool desc_ok(const lp_subnet_desc& d) {
    if (!d.src || d.rows < 1 || d.R < 1 || d.rows > d.R) return false;
    if (d.kind == 0) return d.cols >= 1 && d.C >= 1 && d.cols <= d.C && d.t >= 1 && d.t <= 65536;
    if (d.kind == 1) return true;
    if (d.kind == 2) return d.cols == 7 || ((d.cols == 5 || d.cols == 3) && d.lin_w && d.lin_b);
    return false;
}

// elements of the sliced tensor in the packed sub-network buffer
__device__ __forceinline__ int64_t sub_numel(const lp_subnet_desc& d) {
    if (d.kind == 0) return (int64_t)d.rows * d.cols * d.t;
    if (d.kind == 1) return d.rows;
    return (int64_t)d.rows * d.cols * d.cols;
}

// the last index whose offset is <= e, or -1
__device__ __forceinline__ int find_owner(const int64_t* offs, int count, int64_t e) {
    if (offs[0] > e) return -1;
    int lo = 0, hi = count;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offs[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// crop index i of a k x k window -> index in the 7 x 7 filter
__device__ __forceinline__ int win_index(int i, int k) {
    const int l = 3 - k / 2;
    return (l + i / k) * 7 + l + i % k;
}

// packed element j (< sub_numel) of descriptor d
__device__ float gather_elem(const lp_subnet_desc& d, int64_t j) {
    if (d.kind == 0) {
        const int64_t W = (int64_t)d.cols * d.t, r = j / W, c = j - r * W;
        return d.src[r * ((int64_t)d.C * d.t) + c];
    }
    if (d.kind == 1 || d.cols == 7) return d.src[j];
    const int k = d.cols, kk = k * k;
    const int64_t c = j / kk;
    const int o = (int)(j - c * kk);
    const float* w = d.src + c * 49;
    const float* L = d.lin_w + o * kk;
    float acc = d.lin_b[o];
    for (int i = 0; i < kk; ++i) acc = acc + w[win_index(i, k)] * L[i];
    return acc;
}

__global__ __launch_bounds__(TPB) void subnet_gather_kernel(const lp_subnet_desc* __restrict__ desc, int count,
                                                            float* __restrict__ sub, int64_t sub_elems) {
    __shared__ int64_t offs[LP_SUBNET_MAX_DESC];
    for (int i = threadIdx.x; i < count; i += TPB) offs[i] = desc[i].sub_offset;
    __syncthreads();
    const int64_t e0 = ((int64_t)blockIdx.x * TPB + threadIdx.x) * 4;
    if (e0 >= sub_elems) return;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const int owner = find_owner(offs, count, e0);
    if (owner >= 0) {
        const lp_subnet_desc d = desc[owner];
        const int64_t j = e0 - d.sub_offset, n = desc_ok(d) ? sub_numel(d) : 0;
        if (j + 3 < n) {
            bool vec = (d.kind == 1 || (d.kind == 2 && d.cols == 7)) && al16(d.src) && (j & 3) == 0;
            int64_t si = j;
            if (d.kind == 0) {
                const int64_t W = (int64_t)d.cols * d.t, CT = (int64_t)d.C * d.t, r = j / W, c = j - r * W;
                vec = (W & 3) == 0 && (CT & 3) == 0 && (c & 3) == 0 && al16(d.src);
                si = r * CT + c;
            }
            if (vec) {
                const float4 q = *reinterpret_cast<const float4*>(d.src + si);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            } else {
                for (int q = 0; q < 4; ++q) v[q] = gather_elem(d, j + q);
            }
        } else {
            for (int q = 0; q < 4; ++q)
                if (j + q < n) v[q] = gather_elem(d, j + q);
        }
    }
    if (e0 + 3 < sub_elems) {
        *reinterpret_cast<float4*>(sub + e0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int q = 0; q < 4; ++q)
            if (e0 + q < sub_elems) sub[e0 + q] = v[q];
    }
}

__device__ __forceinline__ float gsub_at(const float* g, int64_t i, int64_t sub_elems) {
    return i >= 0 && i < sub_elems ? g[i] : 0.0f;
}

// Element jf of what descriptor d owns in the full-gradient buffer.  *skip: the element belongs to gL / gb, which
// subnet_window_wgrad_kernel writes.
__device__ float scatter_elem(const lp_subnet_desc& d, int64_t jf, const float* g, int64_t sub_elems, bool* skip) {
    *skip = false;
    if (d.kind == 0) {
        const int64_t CT = (int64_t)d.C * d.t, W = (int64_t)d.cols * d.t;
        if (jf >= (int64_t)d.R * CT) return 0.0f;
        const int64_t r = jf / CT, c = jf - r * CT;
        return r < d.rows && c < W ? gsub_at(g, d.sub_offset + r * W + c, sub_elems) : 0.0f;
    }
    if (d.kind == 1) return jf < d.rows ? gsub_at(g, d.sub_offset + jf, sub_elems) : 0.0f;
    const int k = d.cols, kk = k * k;
    if (k == 7) return jf < (int64_t)d.rows * 49 ? gsub_at(g, d.sub_offset + jf, sub_elems) : 0.0f;
    const int64_t n7 = (int64_t)d.R * 49;
    if (jf >= n7) {
        const int64_t offL = a64(n7), offB = offL + a64((int64_t)kk * kk);
        *skip = (jf >= offL && jf < offL + (int64_t)kk * kk) || (jf >= offB && jf < offB + kk);
        return 0.0f;
    }
    const int64_t c = jf / 49;
    const int p = (int)(jf - c * 49), l = 3 - k / 2, y = p / 7 - l, x = p % 7 - l;
    if (c >= d.rows || y < 0 || y >= k || x < 0 || x >= k) return 0.0f;
    const int i = y * k + x;
    const int64_t gi = d.sub_offset + c * kk;
    float acc = gsub_at(g, gi, sub_elems) * d.lin_w[i];
    for (int o = 1; o < kk; ++o) acc = acc + gsub_at(g, gi + o, sub_elems) * d.lin_w[o * kk + i];
    return acc;
}

__global__ __launch_bounds__(TPB) void subnet_scatter_kernel(const lp_subnet_desc* __restrict__ desc, int count,
                                                             const float* __restrict__ g, int64_t sub_elems,
                                                             float* __restrict__ full, int64_t full_elems) {
    __shared__ int64_t offs[LP_SUBNET_MAX_DESC];
    for (int i = threadIdx.x; i < count; i += TPB) offs[i] = desc[i].full_offset;
    __syncthreads();
    const int64_t e0 = ((int64_t)blockIdx.x * TPB + threadIdx.x) * 4;
    if (e0 >= full_elems) return;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    bool skip[4] = {false, false, false, false};
    const int owner = find_owner(offs, count, e0);
    if (owner >= 0) {
        const lp_subnet_desc d = desc[owner];
        if (desc_ok(d)) {
            const int64_t jf = e0 - d.full_offset;
            // four cells of one row, all inside or all outside the slice: one 16-byte load of the packed gradient
            bool vec = false;
            int64_t gi = 0;
            if (d.kind == 0) {
                const int64_t CT = (int64_t)d.C * d.t, W = (int64_t)d.cols * d.t, r = jf / CT, c = jf - r * CT;
                vec = (W & 3) == 0 && (CT & 3) == 0 && (jf & 3) == 0 && r < d.rows && c < W;
                gi = d.sub_offset + r * W + c;
            } else if (d.kind == 1 || d.cols == 7) {
                const int64_t n = d.kind == 1 ? d.rows : (int64_t)d.rows * 49;
                vec = (jf & 3) == 0 && jf + 3 < n;
                gi = d.sub_offset + jf;
            }
            if (vec && (gi & 3) == 0 && gi >= 0 && gi + 3 < sub_elems) {
                const float4 q = *reinterpret_cast<const float4*>(g + gi);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            } else {
                for (int q = 0; q < 4; ++q) v[q] = scatter_elem(d, jf + q, g, sub_elems, &skip[q]);
            }
        }
    }
    if (e0 + 3 < full_elems && !(skip[0] || skip[1] || skip[2] || skip[3])) {
        *reinterpret_cast<float4*>(full + e0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int q = 0; q < 4; ++q)
            if (e0 + q < full_elems && !skip[q]) full[e0 + q] = v[q];
    }
}

// gL[o][i] and gb[o] of one window descriptor (blockIdx.y) and one output o (blockIdx.x): thread (seg, lane) sums
// segment seg of the channels for column i = lane (lane 31: gb); the 8 partials meet in LDS and are added in order.
__global__ __launch_bounds__(TPB) void subnet_window_wgrad_kernel(const lp_subnet_desc* __restrict__ desc,
                                                                  const float* __restrict__ g, int64_t sub_elems,
                                                                  float* __restrict__ full, int64_t full_elems) {
    __shared__ float part[LP_SUBNET_SEGS][32];
    const lp_subnet_desc d = desc[blockIdx.y];
    if (d.kind != 2 || d.cols == 7 || !desc_ok(d)) return;
    const int k = d.cols, kk = k * k, o = blockIdx.x;
    if (o >= kk) return;
    const int lane = threadIdx.x & 31, seg = threadIdx.x >> 5;
    const int sl = (d.rows + LP_SUBNET_SEGS - 1) / LP_SUBNET_SEGS;
    const int c0 = seg * sl, c1 = min(d.rows, c0 + sl);
    float acc = 0.0f;
    if (lane < kk) {
        const int wi = win_index(lane, k);
        for (int c = c0; c < c1; ++c)
            acc = acc + gsub_at(g, d.sub_offset + (int64_t)c * kk + o, sub_elems) * d.src[(int64_t)c * 49 + wi];
    } else if (lane == 31) {
        for (int c = c0; c < c1; ++c) acc = acc + gsub_at(g, d.sub_offset + (int64_t)c * kk + o, sub_elems);
    }
    part[seg][lane] = acc;
    __syncthreads();
    if (seg != 0 || !(lane < kk || lane == 31)) return;
    float tot = part[0][lane];
    for (int s = 1; s < LP_SUBNET_SEGS; ++s) tot = tot + part[s][lane];
    const int64_t offL = d.full_offset + a64((int64_t)d.R * 49), offB = offL + a64((int64_t)kk * kk);
    const int64_t at = lane < kk ? offL + (int64_t)o * kk + lane : offB + o;
    if (at >= 0 && at < full_elems) full[at] = tot;
}

// ---------------------------------------------------------------------------------- random-resolution resize
__global__ __launch_bounds__(TPB) void train_resize_kernel(ResizeJobs jobs) {
    const ResizeJob jb = jobs.job[blockIdx.y];
    const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (jb.kind == 1) {
        if (t >= jb.planes) return;
        const int32_t* src = static_cast<const int32_t*>(jb.src);
        int32_t* dst = static_cast<int32_t*>(jb.dst);
        const int32_t j = src[2 * t], B = jobs.B, S = jobs.S;
        int32_t q = j / B, m = j - q * B;              // floor division and its non-negative remainder
        if (m < 0) { m += B; q -= 1; }
        const int32_t x = (int32_t)((int64_t)m * S / B), y = (int32_t)((int64_t)q * S / B);
        dst[2 * t] = y * S + x;
        dst[2 * t + 1] = src[2 * t + 1];
        return;
    }
    // four consecutive cells of the output tensor (out is even, so a plane is a whole number of groups; a group may
    // run over the end of a row)
    const int64_t groups = (int64_t)jb.planes * jb.out * jb.out / 4;
    if (t >= groups) return;
    const float* src = static_cast<const float*>(jb.src);
    float v[4];
    for (int q = 0; q < 4; ++q) {
        const int64_t e = t * 4 + q, row = e / jb.out, plane = row / jb.out;
        const int dx = (int)(e - row * jb.out), dy = (int)(row - plane * jb.out);
        const int sy = min((int)((int64_t)dy * jb.in / jb.out), jb.in - 1);
        const int sx = min((int)((int64_t)dx * jb.in / jb.out), jb.in - 1);
        v[q] = src[(plane * jb.in + sy) * jb.in + sx];
    }
    *reinterpret_cast<float4*>(static_cast<float*>(jb.dst) + t * 4) = make_float4(v[0], v[1], v[2], v[3]);
}

int64_t resize_job_threads(const ResizeJob& j) {
    return j.kind == 1 ? (int64_t)j.planes : (int64_t)j.planes * j.out * j.out / 4;
}

void launch_subnet_gather(const lp_subnet_desc* desc, int count, float* sub, int64_t sub_elems, hipStream_t s) {
    const int64_t groups = (sub_elems + 3) / 4;
    subnet_gather_kernel<<<dim3((unsigned)((groups + TPB - 1) / TPB)), TPB, 0, s>>>(desc, count, sub, sub_elems);
}

void launch_subnet_scatter(const lp_subnet_desc* desc, int count, const float* gsub, int64_t sub_elems, float* full,
                           int64_t full_elems, hipStream_t s) {
    const int64_t groups = (full_elems + 3) / 4;
    subnet_scatter_kernel<<<dim3((unsigned)((groups + TPB - 1) / TPB)), TPB, 0, s>>>(desc, count, gsub, sub_elems, full,
                                                                                      full_elems);
    subnet_window_wgrad_kernel<<<dim3(25, (unsigned)count), TPB, 0, s>>>(desc, gsub, sub_elems, full, full_elems);
}

void launch_train_resize(const ResizeJobs& jobs, hipStream_t s) {
    int64_t most = 1;
    for (int i = 0; i < jobs.njobs; ++i) most = max(most, resize_job_threads(jobs.job[i]));
    train_resize_kernel<<<dim3((unsigned)((most + TPB - 1) / TPB), (unsigned)jobs.njobs), TPB, 0, s>>>(jobs);
}

}  // namespace lp
