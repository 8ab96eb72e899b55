// gfx950 kernel of utils.vis (reference lib/utils/vis.py:68-118, add_joints / get_annotated_image): skeletons drawn into
// uint8 HWC images on the device.  The raster rule is this library's own: a joint mark is the integer disc
// |P - C|^2 <= Rj^2, a link the integer capsule dist(P, AB)^2 <= Rl^2, both evaluated exactly in 64-bit integers.  It is
// NOT pinned against cv2.circle / cv2.line (cv2 was not available to pin it).
#include "kernels.h"

namespace lp {

namespace {
constexpr int VIS_THREADS = 256;
constexpr int VIS_TW = 16;                 // tile: 16 columns x 64 rows (standing limbs are taller than wide); a thread
constexpr int VIS_TH = 64;                 // owns column tid % 16 of rows tid / 16 + 16 k, k < 4
constexpr int VIS_PX = VIS_TW * VIS_TH / VIS_THREADS;

struct Prim {                              // a capsule A-B of radius r (a joint mark: A == B), 16 bytes
    short ax, ay, bx, by;
    int person;
    int r;
};

// visible: val > 0, x and y finite, trunc(x) and trunc(y) inside [-16384, 16383] (a NaN fails every comparison)
__device__ inline bool joint_at(const float* __restrict__ k, int& x, int& y) {
    const float fx = k[0], fy = k[1], v = k[2];
    const bool ok = v > 0.f && fx > -16385.f && fx < 16384.f && fy > -16385.f && fy < 16384.f;
    x = ok ? (int)fx : 0;                  // float -> int truncates toward zero, like Python's int()
    y = ok ? (int)fy : 0;
    return ok;
}

__device__ inline bool covers(const Prim& q, int px, int py) {
    const long long apx = px - q.ax, apy = py - q.ay, abx = q.bx - q.ax, aby = q.by - q.ay;
    const long long d = apx * abx + apy * aby, L = abx * abx + aby * aby;
    const long long r2 = q.r * q.r;
    if (d <= 0) return apx * apx + apy * apy <= r2;
    if (d >= L) {
        const long long bpx = px - q.bx, bpy = py - q.by;
        return bpx * bpx + bpy * bpy <= r2;
    }
    const long long c = apx * aby - apy * abx;             // |c| < 2^31: c * c stays inside int64
    return c * c <= r2 * L;
}
}  // namespace

// One workgroup walks tiles t = blockIdx.y, blockIdx.y + gridDim.y, ... of image blockIdx.x.  The image's primitives --
// person p < P = min(max(count, 0), pcap), then joint j < J or link l < n_links -- are taken in passes of VIS_PASS_PRIMS:
// every thread resolves some of them once (visibility, truncation) into the LDS table `all`; then, per tile, the entries
// whose bounding box, widened by the radius, meets the tile are listed, and every pixel of the tile tests the list and
// keeps the highest person index that covers it (the painter's order of the reference's loop; the order of the table and
// of the list does not matter, so the LDS counters do not make the result depend on scheduling).  A later pass holds
// persons of the same or a higher index and is painted over the earlier ones by the same thread.  A tile whose list is
// empty touches no pixel.
// desc == nullptr: equal-sized images [N,H,W,3]; otherwise image n lies at desc[n].offset of the `bytes`-long buffer with
// its own size, and a descriptor that does not fit is skipped before anything is read or written.
__global__ __launch_bounds__(VIS_THREADS) void draw_poses_kernel(
    unsigned char* __restrict__ images, long long bytes, const ImageDesc* __restrict__ desc, int H, int W,
    const float* __restrict__ kpts, const int* __restrict__ count, int pcap, int J, int D, VisTables tb, int n_links,
    int n_colors, int Rj, int Rl) {
    __shared__ Prim all[VIS_PASS_PRIMS];
    __shared__ unsigned short list[VIS_PASS_PRIMS];
    __shared__ int s_all, s_n;
    __shared__ unsigned char s_la[64], s_lb[64], s_pal[96];
    const int tid = threadIdx.x;
    const size_t n = blockIdx.x;
    unsigned char* img;
    if (desc) {
        const long long off = desc[n].offset;
        H = desc[n].H;
        W = desc[n].W;
        if (H < 1 || W < 1 || H > 16384 || W > 16384 || off < 0 || off > bytes || (long long)H * W * 3 > bytes - off)
            return;
        img = images + off;
    } else {
        img = images + n * H * W * 3;
    }
    const int ntx = (W + VIS_TW - 1) / VIS_TW, nty = (H + VIS_TH - 1) / VIS_TH;
    if ((int)blockIdx.y >= ntx * nty) return;              // a worker without a tile
    const int c = count[n];
    const int P = c < 0 ? 0 : (c < pcap ? c : pcap);
    if (P == 0) return;
    if (tid < 64) {
        s_la[tid] = tb.la[tid];
        s_lb[tid] = tb.lb[tid];
    }
    if (tid < 96) s_pal[tid] = tb.pal[tid];
    const int K = J + n_links;
    const long long total = (long long)P * K;
    const float* kp = kpts + n * pcap * J * D;
    const int lx = tid % VIS_TW, ly = tid / VIS_TW;
    for (long long q0 = 0; q0 < total; q0 += VIS_PASS_PRIMS) {
        __syncthreads();                                   // the table of the previous pass is no longer read
        if (tid == 0) s_all = 0;
        __syncthreads();
        const long long q1 = min(q0 + VIS_PASS_PRIMS, total);
        for (long long q = q0 + tid; q < q1; q += VIS_THREADS) {
            const int p = (int)(q / K), k = (int)(q % K);
            const float* pk = kp + (size_t)p * J * D;
            int ax, ay, bx, by, r;
            bool ok;
            if (k < J) {
                ok = joint_at(pk + (size_t)k * D, ax, ay);
                bx = ax, by = ay, r = Rj;
            } else {
                const int a = s_la[k - J], b = s_lb[k - J];
                ok = a < J && b < J;
                if (ok) {
                    const bool va = joint_at(pk + (size_t)a * D, ax, ay);
                    const bool vb = joint_at(pk + (size_t)b * D, bx, by);
                    ok = va && vb;
                }
                r = Rl;
            }
            if (ok) {
                const int slot = atomicAdd(&s_all, 1);     // LDS counter, at most VIS_PASS_PRIMS appends per pass
                all[slot] = Prim{(short)ax, (short)ay, (short)bx, (short)by, p, r};
            }
        }
        __syncthreads();
        const int na = s_all;
        if (na == 0) continue;
        for (int t = blockIdx.y; t < ntx * nty; t += gridDim.y) {
            const int x0 = (t % ntx) * VIS_TW, y0 = (t / ntx) * VIS_TH;
            const int x1 = min(x0 + VIS_TW, W), y1 = min(y0 + VIS_TH, H);
            __syncthreads();                               // the list of the previous tile is no longer read
            if (tid == 0) s_n = 0;
            __syncthreads();
            for (int i = tid; i < na; i += VIS_THREADS) {
                const Prim q = all[i];
                if (min(q.ax, q.bx) - q.r < x1 && max(q.ax, q.bx) + q.r >= x0 && min(q.ay, q.by) - q.r < y1 &&
                    max(q.ay, q.by) + q.r >= y0)
                    list[atomicAdd(&s_n, 1)] = (unsigned short)i;
            }
            __syncthreads();
            const int cnt = s_n;
            if (cnt == 0) continue;
            int best[VIS_PX];
#pragma unroll
            for (int j = 0; j < VIS_PX; ++j) best[j] = -1;
            for (int i = 0; i < cnt; ++i) {
                const Prim q = all[list[i]];
#pragma unroll
                for (int j = 0; j < VIS_PX; ++j) {
                    const int py = y0 + ly + j * (VIS_THREADS / VIS_TW);
                    if (q.person > best[j] && covers(q, x0 + lx, py)) best[j] = q.person;
                }
            }
#pragma unroll
            for (int j = 0; j < VIS_PX; ++j) {
                const int px = x0 + lx, py = y0 + ly + j * (VIS_THREADS / VIS_TW);
                if (best[j] >= 0 && px < x1 && py < y1) {
                    const int col = (best[j] % n_colors) * 3;
                    unsigned char* o = img + ((size_t)py * W + px) * 3;
                    o[0] = s_pal[col];
                    o[1] = s_pal[col + 1];
                    o[2] = s_pal[col + 2];
                }
            }
        }
    }
}

void launch_draw_poses(unsigned char* images, long long bytes, const ImageDesc* desc, int N, int H, int W,
                       const float* kpts, const int* count, int pcap, int J, int D, const int* links, int n_links,
                       const unsigned char* palette, int n_colors, int Rj, int Rl, hipStream_t s) {
    VisTables tb;
    for (int i = 0; i < 64; ++i) {                         // an index >= J is skipped by the kernel: 255 stands for all
        tb.la[i] = i < n_links ? (unsigned char)(links[2 * i] < 255 ? links[2 * i] : 255) : 255;
        tb.lb[i] = i < n_links ? (unsigned char)(links[2 * i + 1] < 255 ? links[2 * i + 1] : 255) : 255;
    }
    for (int i = 0; i < 96; ++i) tb.pal[i] = i < n_colors * 3 ? palette[i] : 0;
    // workgroups per image: every tile of equal-sized images up to a cap that keeps the grid near 4096 workgroups; the
    // per-image form does not know its sizes on the host and takes the cap (a workgroup without a tile returns at once)
    int gx = 4096 / N;
    gx = gx < 8 ? 8 : (gx > 512 ? 512 : gx);
    if (!desc) {
        const long long tiles = (long long)((W + VIS_TW - 1) / VIS_TW) * ((H + VIS_TH - 1) / VIS_TH);
        if (tiles < gx) gx = (int)tiles;
    }
    draw_poses_kernel<<<dim3((unsigned)N, (unsigned)gx), dim3(VIS_THREADS), 0, s>>>(
        images, bytes, desc, H, W, kpts, count, pcap, J, D, tb, n_links, n_colors, Rj, Rl);
}

}  // namespace lp
