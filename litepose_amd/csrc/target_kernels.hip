// The label side of the train loader (lp_target_maps, lp_target_masks; include/litepose_amd.h "training targets"):
//   lib/dataset/transforms/transforms.py:124-129,169-171   RandomAffineTransform._affine_joints   (joint_cell)
//   lib/dataset/transforms/transforms.py:67-72              RandomHorizontalFlip on joints / masks (joint_cell, mask kernel)
//   lib/dataset/target_generators/target_generators.py:28-50    HeatmapGenerator.__call__          (target_maps_kernel)
//   lib/dataset/target_generators/target_generators.py:99-115   JointsGenerator.__call__           (target_maps_kernel)
//   lib/dataset/transforms/transforms.py:163-167            cv2.warpAffine of the uint8 mask, / 255 > 0.5 (target_masks_kernel)
// Compiled without FMA contraction: the fp64 joint transform rounds operation by operation, and the mask warp shares the
// fixed-point arithmetic of the image warp (warp_fixed.h).
#include "kernels.h"
#include "warp_fixed.h"

namespace lp {

namespace {

constexpr int TM_ROWS = 32;         // rows of a plane per workgroup of target_maps_kernel

// The cell of output joint j of person `prs` (a row of joints [P_tot,J,3]) under one descriptor: the source joint is
// flip_index[j] when the row is mirrored, the coordinates go through the forward matrix as (m0*x + m1*y) + m2, the mirror
// is x = R - x - 1, and the cell is the coordinate truncated toward zero.  Returns false for v <= 0 or a cell outside the
// plane.  trunc(c) in [0, R) <=> -1 < c < R, tested in fp64 (a NaN fails), so the conversion never overflows.
__device__ __forceinline__ bool joint_cell(const double* __restrict__ joints, long prs, int J, int j,
                                           const TargetDesc& d, const TargetFlip& fi, int R, int& cx, int& cy) {
    const int js = d.flip ? fi.idx[j] : j;
    const double* p = joints + (prs * J + js) * 3;
    const double x = p[0], y = p[1], v = p[2];
    double tx = (d.mat[0] * x + d.mat[1] * y) + d.mat[2];
    const double ty = (d.mat[3] * x + d.mat[4] * y) + d.mat[5];
    if (d.flip) tx = ((double)R - tx) - 1.0;
    if (!(v > 0.0) || !(tx > -1.0 && tx < (double)R) || !(ty > -1.0 && ty < (double)R)) return false;
    cx = (int)tx;
    cy = (int)ty;
    return true;
}

}  // namespace

// blockIdx.x = n * JB + jb (JB = J with heat, 1 without), blockIdx.y = strip of TM_ROWS rows.
// Heat: wave 0 computes the cell of joint j of the row's first M persons and packs the valid ones into LDS; then every
// pixel of the strip takes the maximum of the table entries of the persons whose window [c - s3 - 1, c + s3 + 2) covers it
// (a gather: no atomics, one store per pixel).  Joints: the workgroup (jb 0, strip 0) of an image walks each person's
// joints in order, one person per lane, and writes the whole [M,J,2] block of the image.
__global__ __launch_bounds__(256) void target_maps_kernel(
    const double* __restrict__ joints, long P_tot, const int* __restrict__ first, const TargetDesc* __restrict__ desc,
    TargetFlip fi, int J, int JB, int R, const float* __restrict__ gauss, int side, int s3, int M, int tag_per_joint,
    float* __restrict__ heat, int* __restrict__ jout) {
    __shared__ int s_cx[64], s_cy[64];
    __shared__ int s_n;
    const int n = blockIdx.x / JB, j = blockIdx.x - n * JB;
    const int tid = threadIdx.x;
    const TargetDesc& d = desc[n];
    const long lo = first[n], hi = first[n + 1];
    const bool ok = d.reserved == 0 && lo >= 0 && hi >= lo && hi <= P_tot;
    const int cnt = ok ? (int)min(hi - lo, (long)M) : 0;

    if (jout && j == 0 && blockIdx.y == 0 && tid < M) {
        int* o = jout + ((long)n * M + tid) * J * 2;
        int tot = 0;
        if (tid < cnt) {
            for (int k = 0; k < J; ++k) {
                int cx, cy;
                if (joint_cell(joints, lo + tid, J, k, d, fi, R, cx, cy)) {
                    o[2 * tot] = (tag_per_joint ? k * R * R : 0) + cy * R + cx;
                    o[2 * tot + 1] = 1;
                    ++tot;
                }
            }
        }
        for (int k = tot; k < J; ++k) { o[2 * k] = 0; o[2 * k + 1] = 0; }
    }
    if (!heat) return;

    if (tid < 64) {                                           // wave 0: M <= 64 persons, one per lane
        int cx = 0, cy = 0;
        const bool v = tid < cnt && joint_cell(joints, lo + tid, J, j, d, fi, R, cx, cy);
        const unsigned long long m = __ballot(v);
        if (v) {
            const int slot = __popcll(m & ((1ull << tid) - 1ull));
            s_cx[slot] = cx;
            s_cy[slot] = cy;
        }
        if (tid == 0) s_n = __popcll(m);
    }
    __syncthreads();
    const int nv = s_n;
    const int y0 = blockIdx.y * TM_ROWS;
    const int rows = min(TM_ROWS, R - y0);
    float* plane = heat + ((long)n * J + j) * R * R;
    for (int e = tid; e < rows * R; e += 256) {
        const int py = y0 + e / R, px = e % R;
        float best = 0.f;
        for (int k = 0; k < nv; ++k) {
            const int gx = px - (s_cx[k] - s3 - 1), gy = py - (s_cy[k] - s3 - 1);
            if (gx >= 0 && gx < side && gy >= 0 && gy < side) best = fmaxf(best, gauss[gy * side + gx]);
        }
        plane[(long)py * R + px] = best;
    }
}

// One thread per output pixel: blockIdx.z = row n of the table, blockIdx.y = y.  The one-channel form of
// warp_affine_flip_norm_v_kernel: the same taps and weights (warp_fixed.h) on a byte that is 255 where the source mask is
// set -- or everywhere inside the H x W source when src_offset is -1 -- and 0 outside; 1 iff the interpolated byte is >= 128
// (v / 255 > 0.5).  The mirror is by index.  A bad descriptor writes zeros and reads nothing.
__global__ __launch_bounds__(256) void target_masks_kernel(const unsigned char* __restrict__ src, long long src_bytes,
                                                           const AugDesc* __restrict__ desc, int R,
                                                           float* __restrict__ out) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= R) return;
    const AugDesc& d = desc[blockIdx.z];
    const long long off = d.src_offset;
    const int H = d.H, W = d.W;
    float* o = out + ((long)blockIdx.z * R + y) * R + x;
    const bool ones = off == -1;
    const bool ok = H >= 1 && W >= 1 && H <= 32767 && W <= 32767 && d.reserved == 0 &&
                    (ones || (src != nullptr && off >= 0 && off <= src_bytes && (long long)H * W <= src_bytes - off));
    if (!ok) {
        *o = 0.f;
        return;
    }
    const int xs = d.flip ? R - 1 - x : x;           // the warped column this output column takes
    const WarpTaps t = warp_taps(H, W, xs, y, d.minv[0], d.minv[1], d.minv[2], d.minv[3], d.minv[4], d.minv[5]);
    const unsigned char* m = ones ? nullptr : src + off;
    auto tap = [&](bool in, int yy, int xx) -> int {
        if (!in) return 0;
        return (ones || m[(long)yy * W + xx] != 0) ? 255 : 0;
    };
    const int v = warp_blend(t, tap(t.y0 && t.x0, t.sy, t.sx), tap(t.y0 && t.x1, t.sy, t.sx + 1),
                             tap(t.y1 && t.x0, t.sy + 1, t.sx), tap(t.y1 && t.x1, t.sy + 1, t.sx + 1));
    *o = v >= 128 ? 1.f : 0.f;
}

void launch_target_maps(const double* joints, long P_tot, const int* first, const TargetDesc* desc, int N, int J, int R,
                        const TargetFlip& fi, const float* gauss, int side, int s3, int M, int tag_per_joint, float* heat,
                        int* jout, hipStream_t s) {
    const int JB = heat ? J : 1;
    const int strips = heat ? (R + TM_ROWS - 1) / TM_ROWS : 1;
    hipLaunchKernelGGL(target_maps_kernel, dim3((unsigned)N * JB, strips), dim3(256), 0, s, joints, P_tot, first, desc, fi,
                       J, JB, R, gauss, side, s3, M, tag_per_joint, heat, jout);
}

void launch_target_masks(const unsigned char* src, long long src_bytes, const AugDesc* desc, int N, int R, float* out,
                         hipStream_t s) {
    hipLaunchKernelGGL(target_masks_kernel, dim3((R + 255) / 256, R, N), dim3(256), 0, s, src, src_bytes, desc, R, out);
}

}  // namespace lp
