// gfx950 kernels for the LitePose network (planar NCHW fp32).
//
// Layout choice: planar NCHW, pixels innermost.  For fp32 the matrix cores take ONE
// f32 per lane per operand (v_mfma_f32_32x32x2_f32: B[k = lane>>5][j = lane&31]), so
// a B fragment is "32 consecutive pixels of channel k | 32 consecutive pixels of
// channel k+1": with pixels innermost both halves are single 128-byte coalesced
// global loads and the 1x1 convs need no LDS transpose at all.  The depthwise convs
// get their 49 per-channel weights as wave-uniform SGPR operands (v_fma v, s, v, v)
// because a wave works on one channel plane, and stage a halo tile per WAVEFRONT in
// LDS.  (NHWC would put per-lane weight vectors in VGPRs and strided B fragments.)
//
// Reference semantics: lib/models/layers/layers.py:18-24 (convbnrelu), :90-118
// (InvBottleneck), :120-133 (SepConv2d); lib/models/pose_mobilenet.py:113-131,143-156
// (Fusion Deconv Head).  BN is folded on the host (engine.cpp).
#include "kernels.h"
#include "fused_common.h"
#include "split3.h"

#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <utility>

namespace lp {

thread_local const char* last_kernel_tag = "";
thread_local LaunchNote last_launch;
thread_local bool launch_notes = false;

void note_launch(const void* fn, dim3 grid, dim3 block, size_t lds) {
    int per_cu = 0;
    const int threads = (int)(block.x * block.y * block.z);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, threads, lds) != hipSuccess) per_cu = 0;
    last_launch.grid = (int)((long)grid.x * grid.y * grid.z);
    last_launch.block = threads;
    last_launch.lds = (int)lds;
    last_launch.wgs_per_cu = per_cu;
}

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// tiles are dealt to workgroups XCD-contiguously (xcd_contiguous_id, fused_common.h); measured on every tiled kernel in rounds
// 1-3, the hardware order never won
static constexpr int xcd_remap_mode() { return 1; }

// The bounds of ACT_NONE in the branch-free clamp fminf(fmaxf(v, lo), hi) of the planar 1x1 and depthwise launchers the
// training layers call.  fmaxf / fminf are IEEE maxNum / minNum: they return the operand that is not a NaN, and a NaN only
// when both are.  Against a NaN bound every v comes back as itself, a NaN v included; against -inf / +inf a NaN sum would
// leave the layer as -inf, and a diverged training run would look finite.  The same instructions, another constant.
#define ACT_NONE_BOUND __builtin_nanf("")

__device__ __forceinline__ float apply_act(float v, int act) {
    if (act == ACT_RELU) return fmaxf(v, 0.f);
    if (act == ACT_RELU6) return fminf(fmaxf(v, 0.f), 6.f);
    return v;
}


// -------------------------------------------------------------------------------------
// Packed-fp32 depthwise row (stride 1).  A wave64 VALU instruction costs ~4 cycles on this
// chip whether it carries one FMA or two, so the 7x7 inner loop is issued as v_pk_fma_f32.
// A lane owns outputs o0..o3 of a row and holds the input row as six ALIGNED register pairs
// P[m] = (v[2m], v[2m+1]).  Tap kx of output o_i reads v[off + i], off = 4 - HALO + kx:
//   off even: (o0,o1) += w*P[off/2], (o2,o3) += w*P[off/2+1]                    2 pk_fma
//   off odd : the pairs (o0,o1) would straddle two register pairs, so the tap is applied to
//             the shifted pairing (o-1,o0),(o1,o2),(o3,o4) instead, which IS aligned; 3 pk_fma
// The o-1 / o4 halves are wasted work (the neighbour lanes compute those outputs themselves).
// 7 taps: 18 pk_fma instead of 28 v_fma.
// -------------------------------------------------------------------------------------
typedef float f32x2 __attribute__((ext_vector_type(2)));

template <int K>
__device__ __forceinline__ void dw_row_pk(const f32x4 (&q)[3], const f32x2* __restrict__ wrow,   // taps as (w, w) pairs
                                          f32x2 (&A)[2], f32x2 (&B)[3]) {
    const f32x2 P[6] = {{q[0][0], q[0][1]}, {q[0][2], q[0][3]}, {q[1][0], q[1][1]},
                        {q[1][2], q[1][3]}, {q[2][0], q[2][1]}, {q[2][2], q[2][3]}};
#pragma unroll
    for (int kx = 0; kx < K; ++kx) {
        // an aligned (w, w) pair from the duplicated weight array: a 64-bit scalar operand that needs no op_sel
        // (broadcasting the tap of an odd SGPR takes op_sel:[0,1,0], the packed form DESIGN 5b forbids)
        const f32x2 w2 = wrow[kx];
        constexpr int BASE = 4 - K / 2;
        const int off = BASE + kx;
        if ((off & 1) == 0) {
            const int m = off >> 1;
            A[0] = __builtin_elementwise_fma(P[m], w2, A[0]);
            A[1] = __builtin_elementwise_fma(P[m + 1], w2, A[1]);
        } else {
            const int m = (off - 1) >> 1;
            B[0] = __builtin_elementwise_fma(P[m], w2, B[0]);
            B[1] = __builtin_elementwise_fma(P[m + 1], w2, B[1]);
            B[2] = __builtin_elementwise_fma(P[m + 2], w2, B[2]);
        }
    }
}

// o[0..3] of this lane from the two pairings (the o-1 / o4 halves of B are simply unused: they
// duplicate what the neighbour lanes compute for themselves)
__device__ __forceinline__ void dw_pk_combine(const f32x2 (&A)[2], const f32x2 (&B)[3], float (&o)[4]) {
    o[0] = A[0][0] + B[0][1];
    o[1] = A[0][1] + B[1][0];
    o[2] = A[1][0] + B[1][1];
    o[3] = A[1][1] + B[2][0];
}

// =====================================================================================
// stem: conv 3x3 stride 2 pad 1, 3 -> 32, + bias + ReLU6.  One output pixel per lane,
// all 32 output channels per lane; the 864 weights are wave-uniform (scalar loads).
// =====================================================================================
__global__ __launch_bounds__(256) void stem_kernel(const float* __restrict__ x,
                                                   const float* __restrict__ w,
                                                   const float* __restrict__ b,
                                                   float* __restrict__ out, int N, int H, int W,
                                                   int flip_from, int x_batch) {
    const int OH = H >> 1, OW = W >> 1;
    const long total = (long)N * OH * OW;
    long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const int ox = (int)(g % OW);
    const int oy = (int)((g / OW) % OH);
    const int n = (int)(g / ((long)OW * OH));
    const bool flip = n >= flip_from;
    const int nsrc = n % x_batch;
    float v[27];
#pragma unroll
    for (int ci = 0; ci < 3; ++ci) {
        const float* plane = x + ((long)nsrc * 3 + ci) * H * W;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = 2 * oy - 1 + ky;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = 2 * ox - 1 + kx;
                float t = 0.f;
                if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
                    const int sx = flip ? (W - 1 - ix) : ix;
                    t = plane[(long)iy * W + sx];
                }
                v[ci * 9 + ky * 3 + kx] = t;
            }
        }
    }
    float* o = out + (long)n * 32 * OH * OW + (long)oy * OW + ox;
#pragma unroll 4
    for (int co = 0; co < 32; ++co) {
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < 27; ++i) acc = fmaf(v[i], w[co * 27 + i], acc);
        acc += b[co];
        o[(long)co * OH * OW] = fminf(fmaxf(acc, 0.f), 6.f);
    }
}

void launch_stem(const float* x, const float* w, const float* b, float* out, int N, int H, int W,
                 int flip_from, int x_batch, hipStream_t s) {
    const long total = (long)N * (H / 2) * (W / 2);
    const int grid = (int)((total + 255) / 256);
    LP_LAUNCH(stem_kernel, dim3(grid), dim3(256), 0, s, x, w, b, out, N, H, W, flip_from,
                       x_batch);
    last_kernel_tag = "stem_kernel";
}

// =====================================================================================
// depthwise KxK (K in 3,5,7), stride S in 1,2, + bias + act.
// One WAVEFRONT per 16x16 output tile of one (image, channel) plane:
//   * the haloed input tile is staged in a wave-private LDS region with 16-byte global
//     loads; the tile starts 4 columns left of the first needed pixel so every row is
//     float4-aligned both in HBM and in LDS
//   * lane = (row = lane>>2, strip = lane&3) computes 4 horizontally adjacent outputs
//     from ds_read_b128 row segments; the K*K weights + bias are SGPRs
// =====================================================================================
template <int K, int S>
struct DwGeom {
    static constexpr int HALO = K / 2;
    static constexpr int IH = 15 * S + K;                   // input rows per tile
    static constexpr int NV = (S == 1) ? 3 : 4;              // float4 per lane per row
    // LDS row stride (floats).  S=1 needs 23 columns; 48 (not 24) makes the four rows of each
    // ds_read_b128 lane group start 16 banks apart -> conflict-free (24 was 2-way: 44 % of
    // the LDS cycles were SQ_LDS_BANK_CONFLICT, profiles/r01_pmc_dw.txt)
    static constexpr int RS = (S == 1) ? 48 : 40;
    static constexpr int QPR = (S == 1) ? 6 : 10;            // float4 actually staged per row
    static constexpr int LDS_FLOATS = IH * RS;
};

template <int K, int S, bool VEC>
__global__ __launch_bounds__(256) void dw_kernel(const float* __restrict__ in,
                                                 const float* __restrict__ w,       // [C][K*K]       (stride 2: scalar FMAs)
                                                 const float* __restrict__ wdup,    // [C][K*K][2]    (stride 1: packed FMAs)
                                                 const float* __restrict__ b,
                                                 float* __restrict__ out, int N, int C, int H, int W,
                                                 int OH, int OW, int tilesX, int tilesY, int act,
                                                 int units, int tpw) {
    using G = DwGeom<K, S>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // 32-bit unit arithmetic (64-bit division is a software loop on the GPU)
    const int u0 = (blockIdx.x * 4 + wave) * tpw;
    if (u0 >= units) return;                          // wave-uniform
    const int u1 = min(units, u0 + tpw);
    float* tile = smem + wave * G::LDS_FLOATS;
    constexpr int QPR = G::QPR;                       // float4 staged per row
    constexpr int NQ = G::IH * QPR;                   // float4 per tile
    constexpr int NLD = (NQ + 63) / 64;               // float4 per lane
    const float lo = act == ACT_NONE ? ACT_NONE_BOUND : 0.f;
    const float hi = act == ACT_RELU6 ? 6.f : (act == ACT_NONE ? ACT_NONE_BOUND : INFINITY);
    const int row = lane >> 2, strip = lane & 3;

    f32x4 pre[NLD];
    // global -> registers for one tile (software prefetch: issued one tile ahead)
    auto issue = [&](int unit) {
        const int tq = unit / tilesX;
        const int tx = unit - tq * tilesX;
        const int nc = tq / tilesY;
        const int ty = tq - nc * tilesY;
        const float* plane = in + (long)nc * H * W;
        const int ix0 = tx * 16 * S - 4, iy0 = ty * 16 * S - G::HALO;
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int e = lane + 64 * i;
            const int r = e / QPR, q = e - r * QPR;
            const int iy = iy0 + r, ix = ix0 + 4 * q;
            // branch-free: always load from a clamped address, then zero what is padding
            const bool row_ok = e < NQ && iy >= 0 && iy < H;
            const int iyc = min(max(iy, 0), H - 1);
            const float* rowp = plane + (long)iyc * W;
            f32x4 v;
            if (VEC) {
                const bool ok = row_ok && ix >= 0 && ix < W;
                const int ixc = min(max(ix, 0), W - 4);
                v = *reinterpret_cast<const f32x4*>(rowp + ixc);
                if (!ok) v = f32x4{0.f, 0.f, 0.f, 0.f};
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int xx = ix + t;
                    const float tv = rowp[min(max(xx, 0), W - 1)];
                    v[t] = (row_ok && xx >= 0 && xx < W) ? tv : 0.f;
                }
            }
            pre[i] = v;
        }
    };
    issue(u0);
    for (int unit = u0; unit < u1; ++unit) {
        // registers -> wave-private LDS tile (LDS ops of one wave execute in order)
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int e = lane + 64 * i;
            if (e < NQ) {
                const int r = e / QPR, q = e - r * QPR;
                *reinterpret_cast<f32x4*>(tile + r * G::RS + 4 * q) = pre[i];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (unit + 1 < u1) issue(unit + 1);           // next tile's HBM loads fly under the FMAs

        const int tq = unit / tilesX;
        const int tx = unit - tq * tilesX;
        const int nc = tq / tilesY;
        const int ty = tq - nc * tilesY;
        const int c = __builtin_amdgcn_readfirstlane(nc % C);
        const float* wc = w + (long)c * K * K;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        if (S == 1) {
            f32x2 A[2] = {{0.f, 0.f}, {0.f, 0.f}}, B[3] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
            for (int ky = 0; ky < K; ++ky) {
                const float* lr = tile + (row + ky) * G::RS + strip * 4;
                f32x4 q[3];
#pragma unroll
                for (int t = 0; t < 3; ++t) { q[t] = *reinterpret_cast<const f32x4*>(lr + 4 * t); keep_b128(q[t]); }
                dw_row_pk<K>(q, reinterpret_cast<const f32x2*>(wdup) + (long)c * K * K + ky * K, A, B);
            }
            dw_pk_combine(A, B, acc);
        } else {
#pragma unroll
            for (int ky = 0; ky < K; ++ky) {
                const float* lr = tile + (row * S + ky) * G::RS + strip * 4 * S;
                float v[4 * G::NV];
#pragma unroll
                for (int q = 0; q < G::NV; ++q) {
                    f32x4 t = *reinterpret_cast<const f32x4*>(lr + 4 * q);
                    keep_b128(t);
                    v[4 * q + 0] = t[0]; v[4 * q + 1] = t[1]; v[4 * q + 2] = t[2]; v[4 * q + 3] = t[3];
                }
#pragma unroll
                for (int kx = 0; kx < K; ++kx) {
                    const float wk = wc[ky * K + kx];
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        acc[i] = fmaf(v[(4 - G::HALO) + kx + i * S], wk, acc[i]);
                }
            }
        }
        const float bias = b[c];
        const int oy = ty * 16 + row, ox = tx * 16 + strip * 4;
        if (oy < OH) {
            float* o = out + (long)nc * OH * OW + (long)oy * OW + ox;
            const float r0 = fminf(fmaxf(acc[0] + bias, lo), hi), r1 = fminf(fmaxf(acc[1] + bias, lo), hi);
            const float r2 = fminf(fmaxf(acc[2] + bias, lo), hi), r3 = fminf(fmaxf(acc[3] + bias, lo), hi);
            if (ox + 3 < OW && (OW & 3) == 0) {
                f32x4 t = {r0, r1, r2, r3};
                *reinterpret_cast<f32x4*>(o) = t;
            } else {
                if (ox + 0 < OW) o[0] = r0;
                if (ox + 1 < OW) o[1] = r1;
                if (ox + 2 < OW) o[2] = r2;
                if (ox + 3 < OW) o[3] = r3;
            }
        }
        // the LDS reads above complete (in order) before the next iteration's writes
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

template <int K, int S>
static void launch_dw_t(const float* in, const float* w, const float* wdup, const float* b, float* out, int N, int C,
                        int H, int W, int act, hipStream_t s) {
    const int OH = (H + 2 * (K / 2) - K) / S + 1, OW = (W + 2 * (K / 2) - K) / S + 1;
    const int tilesX = (OW + 15) / 16, tilesY = (OH + 15) / 16;
    const int units = N * C * tilesX * tilesY;
    // tiles per wave: 2 when the grid is large (amortises the prologue; measured best of
    // 1/2/4/8/16 on MI355X: more tiles per wave only lose thread-level latency hiding)
    const int tpw = units >= 65536 ? 2 : 1;
    const int nwaves = (units + tpw - 1) / tpw;
    const int grid = (int)((nwaves + 3) / 4);
    const size_t lds = 4 * DwGeom<K, S>::LDS_FLOATS * sizeof(float);
    last_kernel_tag = K == 7 ? (S == 1 ? "dw_kernel<7,1>" : "dw_kernel<7,2>") : (K == 5 ? (S == 1 ? "dw_kernel<5,1>" : "dw_kernel<5,2>") : (S == 1 ? "dw_kernel<3,1>" : "dw_kernel<3,2>"));
    if ((W & 3) == 0)
        LP_LAUNCH((dw_kernel<K, S, true>), dim3(grid), dim3(256), lds, s, in, w, wdup, b, out, N, C, H,
                           W, OH, OW, tilesX, tilesY, act, units, tpw);
    else
        LP_LAUNCH((dw_kernel<K, S, false>), dim3(grid), dim3(256), lds, s, in, w, wdup, b, out, N, C, H,
                           W, OH, OW, tilesX, tilesY, act, units, tpw);
}

// =====================================================================================
// depthwise KxK stride 1, IMAGE-PAIRED: one wavefront per 16x16 output tile of the same
// channel of TWO images.  The two haloed input tiles are staged interleaved in LDS -- a 16-byte
// slot holds (img0,img1) of two adjacent pixels -- so every register pair read back is
// (in_n[y][x], in_n+1[y][x]) and every tap of every output is ONE aligned v_pk_fma_f32 against a
// broadcast SGPR weight: K*K*4 packed FMAs per two tiles, none wasted (the single-image kernel
// above spends 18 per 7-tap row instead of 14 because odd tap offsets straddle register pairs).
//   * row stride 17 slots and the quad->row table below make every ds_read_b128 lane group
//     {q0,q3,q5,q6},{q1,q2,q4,q7},.. (MI355X_MICROARCH.md, LDS) hit 16 distinct 16-byte slots
//   * the two halves of a packed FMA never mix, so image n's result does not depend on which
//     image it is paired with (an odd last image is paired with itself and stored once)
// =====================================================================================
template <int K>
struct DwPairGeom {
    static constexpr int HALO = K / 2;
    static constexpr int IH = 15 + K;                        // input rows per tile
    static constexpr int QPR = 6;                            // float4 staged per row per image (x0-4 .. x0+19)
    static constexpr int RSLOT = 17;                         // row stride in 16-byte slots (12 used)
    static constexpr int LDS_FLOATS = IH * RSLOT * 4;
    static constexpr int T0 = (4 - HALO) / 2;                // first / last slot a lane reads per row
    static constexpr int T1 = (4 - HALO + 3 + K - 1) / 2;
};

template <int K, bool VEC>
__global__ __launch_bounds__(256) void dw_pair_kernel(const float* __restrict__ in,
                                                      const float* __restrict__ wdup,    // [C][K*K][2]: every tap twice
                                                      const float* __restrict__ b,
                                                      float* __restrict__ out, int N, int C, int H, int W,
                                                      int tilesX, int tiles, int act, int xcd_remap) {
    using G = DwPairGeom<K>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // grid = ((channel, tile) units / 4, image pair); neighbouring tiles of a plane share halo lines, so
    // consecutive unit quads stay on one XCD (see xcd_contiguous_id)
    const int unit = (xcd_remap ? xcd_contiguous_id(blockIdx.x, gridDim.x) : blockIdx.x) * 4 + wave;
    if (unit >= C * tiles) return;                    // wave-uniform
    const int np = blockIdx.y;
    const int c = unit / tiles, t = unit - c * tiles;
    const int ty = t / tilesX, tx = t - ty * tilesX;
    float* tile = smem + wave * G::LDS_FLOATS;
    constexpr int QPR = G::QPR;
    constexpr int NQ = G::IH * QPR;                   // float4 per tile per image
    constexpr int NLD = (NQ + 63) / 64;
    const long plane_sz = (long)H * W;
    const int n0 = 2 * np, n1 = min(2 * np + 1, N - 1);
    const float* plane0 = in + ((long)n0 * C + c) * plane_sz;
    const float* plane1 = in + ((long)n1 * C + c) * plane_sz;
    const int ix0 = tx * 16 - 4, iy0 = ty * 16 - G::HALO;
    // global -> registers -> wave-private LDS tile, the two images interleaved per pixel
    f32x4 pre0[NLD], pre1[NLD];
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
        const int e = lane + 64 * i;
        const int r = e / QPR, q = e - r * QPR;
        const int iy = iy0 + r, ix = ix0 + 4 * q;
        // branch-free: always load from a clamped address, then zero what is padding
        const bool row_ok = e < NQ && iy >= 0 && iy < H;
        const int iyc = min(max(iy, 0), H - 1);
        f32x4 v0, v1;
        if (VEC) {
            const bool ok = row_ok && ix >= 0 && ix < W;
            const int ixc = min(max(ix, 0), W - 4);
            const int o = iyc * W + ixc;
            v0 = *reinterpret_cast<const f32x4*>(plane0 + o);
            v1 = *reinterpret_cast<const f32x4*>(plane1 + o);
            if (!ok) { v0 = f32x4{0.f, 0.f, 0.f, 0.f}; v1 = v0; }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int xx = ix + k;
                const int o = iyc * W + min(max(xx, 0), W - 1);
                const bool ok = row_ok && xx >= 0 && xx < W;
                const float a0 = plane0[o], a1 = plane1[o];
                v0[k] = ok ? a0 : 0.f;
                v1[k] = ok ? a1 : 0.f;
            }
        }
        pre0[i] = v0;
        pre1[i] = v1;
    }
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
        const int e = lane + 64 * i;
        if (e < NQ) {
            const int r = e / QPR, q = e - r * QPR;
            float* dst = tile + (r * G::RSLOT + 2 * q) * 4;
            *reinterpret_cast<f32x4*>(dst) = f32x4{pre0[i][0], pre1[i][0], pre0[i][1], pre1[i][1]};
            *reinterpret_cast<f32x4*>(dst + 4) = f32x4{pre0[i][2], pre1[i][2], pre0[i][3], pre1[i][3]};
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    const float lo = act == ACT_NONE ? ACT_NONE_BOUND : 0.f;
    const float hi = act == ACT_RELU6 ? 6.f : (act == ACT_NONE ? ACT_NONE_BOUND : INFINITY);
    // quad -> tile row: lane groups of ds_read_b128 then cover rows {0,1,8,9},{2,3,10,11},...
    const int row = (int)((0xFDCE5764B98A1320ull >> (4 * (lane >> 2))) & 15);
    const int strip = lane & 3;
    const f32x2* wc2 = reinterpret_cast<const f32x2*>(wdup) + (long)c * K * K;
    f32x2 acc[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
    for (int ky = 0; ky < K; ++ky) {
        const float* lr = tile + ((row + ky) * G::RSLOT + strip * 2) * 4;
        f32x2 P[12];
#pragma unroll
        for (int k = G::T0; k <= G::T1; ++k) {
            f32x4 q4 = *reinterpret_cast<const f32x4*>(lr + 4 * k);
            keep_b128(q4);                                          // a half-used slot stays ds_read_b128 (split3.h)
            P[2 * k] = f32x2{q4[0], q4[1]};
            P[2 * k + 1] = f32x2{q4[2], q4[3]};
        }
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
            const f32x2 w2 = wc2[ky * K + kx];                     // aligned (w, w): no op_sel on the packed FMA
#pragma unroll
            for (int i = 0; i < 4; ++i)
                acc[i] = __builtin_elementwise_fma(P[4 - G::HALO + kx + i], w2, acc[i]);
        }
    }
    const float bias = b[c];
    const int oy = ty * 16 + row, ox = tx * 16 + strip * 4;
    if (oy < H) {
        float* o0 = out + ((long)n0 * C + c) * plane_sz + oy * W + ox;
        float r0[4], r1[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            r0[i] = fminf(fmaxf(acc[i][0] + bias, lo), hi);
            r1[i] = fminf(fmaxf(acc[i][1] + bias, lo), hi);
        }
        const bool second = n0 + 1 < N;
        float* o1 = o0 + (long)C * plane_sz;
        if (ox + 3 < W && (W & 3) == 0) {
            *reinterpret_cast<f32x4*>(o0) = f32x4{r0[0], r0[1], r0[2], r0[3]};
            if (second) *reinterpret_cast<f32x4*>(o1) = f32x4{r1[0], r1[1], r1[2], r1[3]};
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (ox + i < W) {
                    o0[i] = r0[i];
                    if (second) o1[i] = r1[i];
                }
        }
    }
}

// Whole-plane variant for 16x16 planes (stages 3-4 of XS@256): the tile IS the plane, so staging is one
// 16-byte load per lane per image with no clamping or masking, and the zero halo is written straight to
// LDS.  Same lane mapping and FMA order as dw_pair_kernel (bit-identical results).
template <int K>
__global__ __launch_bounds__(256) void dw_pair16_kernel(const float* __restrict__ in,
                                                        const float* __restrict__ wdup,  // [C][K*K][2]: every tap twice
                                                        const float* __restrict__ b,
                                                        float* __restrict__ out, int N, int C, int act) {
    using G = DwPairGeom<K>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = blockIdx.x * 4 + wave;              // grid = (channel quads, image pairs)
    if (c >= C) return;                               // wave-uniform
    float* tile = smem + wave * G::LDS_FLOATS;
    const int np = blockIdx.y;
    const int n0 = 2 * np, n1 = min(2 * np + 1, N - 1);
    const f32x4 v0 = *reinterpret_cast<const f32x4*>(in + ((long)n0 * C + c) * 256 + lane * 4);
    const f32x4 v1 = *reinterpret_cast<const f32x4*>(in + ((long)n1 * C + c) * 256 + lane * 4);
    // zero halo: HALO rows above and below (slots 0..11), and slots 0,1,10,11 of the 16 data rows
    constexpr int ZROWS = 2 * G::HALO * 12;
    constexpr int Z = ZROWS + 16 * 4;
#pragma unroll
    for (int i = 0; i < (Z + 63) / 64; ++i) {
        const int idx = lane + 64 * i;
        if (idx < Z) {
            int zr, zs;
            if (idx < ZROWS) {
                const int rr = idx / 12;
                zs = idx - rr * 12;
                zr = rr < G::HALO ? rr : rr + 16;
            } else {
                const int j = idx - ZROWS;
                zr = G::HALO + (j >> 2);
                zs = (j & 3) < 2 ? (j & 3) : (j & 3) + 8;
            }
            *reinterpret_cast<f32x4*>(tile + (zr * G::RSLOT + zs) * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    {
        float* dst = tile + ((G::HALO + (lane >> 2)) * G::RSLOT + 2 * ((lane & 3) + 1)) * 4;
        *reinterpret_cast<f32x4*>(dst) = f32x4{v0[0], v1[0], v0[1], v1[1]};
        *reinterpret_cast<f32x4*>(dst + 4) = f32x4{v0[2], v1[2], v0[3], v1[3]};
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    const float lo = act == ACT_NONE ? ACT_NONE_BOUND : 0.f;
    const float hi = act == ACT_RELU6 ? 6.f : (act == ACT_NONE ? ACT_NONE_BOUND : INFINITY);
    const int row = (int)((0xFDCE5764B98A1320ull >> (4 * (lane >> 2))) & 15);
    const int strip = lane & 3;
    const f32x2* wc2 = reinterpret_cast<const f32x2*>(wdup) + (long)c * K * K;
    f32x2 acc[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
    for (int ky = 0; ky < K; ++ky) {
        const float* lr = tile + ((row + ky) * G::RSLOT + strip * 2) * 4;
        f32x2 P[12];
#pragma unroll
        for (int t = G::T0; t <= G::T1; ++t) {
            f32x4 q4 = *reinterpret_cast<const f32x4*>(lr + 4 * t);
            keep_b128(q4);                                          // a half-used slot stays ds_read_b128 (split3.h)
            P[2 * t] = f32x2{q4[0], q4[1]};
            P[2 * t + 1] = f32x2{q4[2], q4[3]};
        }
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
            const f32x2 w2 = wc2[ky * K + kx];                     // aligned (w, w): no op_sel on the packed FMA
#pragma unroll
            for (int i = 0; i < 4; ++i)
                acc[i] = __builtin_elementwise_fma(P[4 - G::HALO + kx + i], w2, acc[i]);
        }
    }
    const float bias = b[c];
    float r0[4], r1[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        r0[i] = fminf(fmaxf(acc[i][0] + bias, lo), hi);
        r1[i] = fminf(fmaxf(acc[i][1] + bias, lo), hi);
    }
    float* o0 = out + ((long)n0 * C + c) * 256 + row * 16 + strip * 4;
    *reinterpret_cast<f32x4*>(o0) = f32x4{r0[0], r0[1], r0[2], r0[3]};
    if (n0 + 1 < N) *reinterpret_cast<f32x4*>(o0 + (long)C * 256) = f32x4{r1[0], r1[1], r1[2], r1[3]};
}

template <int K>
static void launch_dw_pair_t(const float* in, const float* w, const float* b, float* out, int N, int C,
                             int H, int W, int act, hipStream_t s) {
    const int tilesX = (W + 15) / 16, tilesY = (H + 15) / 16;
    const int pairs = (N + 1) / 2;
    const size_t lds = 4 * DwPairGeom<K>::LDS_FLOATS * sizeof(float);
    last_kernel_tag = K == 7 ? "dw_pair_kernel<7>" : (K == 5 ? "dw_pair_kernel<5>" : "dw_pair_kernel<3>");
    // one unit (tile pair) per wave: two per wave measured 3-17 % slower on every layer (profiles/README.md)
    if (H == 16 && W == 16) {
        last_kernel_tag = K == 7 ? "dw_pair16_kernel<7>" : (K == 5 ? "dw_pair16_kernel<5>" : "dw_pair16_kernel<3>");
        LP_LAUNCH((dw_pair16_kernel<K>), dim3((C + 3) / 4, pairs), dim3(256), lds, s, in, w, b, out, N, C,
                           act);
        return;
    }
    const int tiles = tilesX * tilesY;
    const dim3 grid((C * tiles + 3) / 4, pairs);
    if ((W & 3) == 0)
        LP_LAUNCH((dw_pair_kernel<K, true>), grid, dim3(256), lds, s, in, w, b, out, N, C, H, W, tilesX,
                           tiles, act, tiles > 4 ? xcd_remap_mode() : 0);
    else
        LP_LAUNCH((dw_pair_kernel<K, false>), grid, dim3(256), lds, s, in, w, b, out, N, C, H, W, tilesX,
                           tiles, act, tiles > 4 ? xcd_remap_mode() : 0);
}

void launch_dw(const float* in, const float* w, const float* wdup, const float* b, float* out, int N, int C, int H,
               int W, int K, int S, int act, hipStream_t s) {
    // stride 1: the image-paired kernel for every batch size (numerics must not depend on N); the pair
    // index is a grid y dimension (<= 65535 pairs)
    if (S == 1 && (K == 7 || K == 5 || K == 3) && (N + 1) / 2 <= 65535) {
        if (K == 7) launch_dw_pair_t<7>(in, wdup, b, out, N, C, H, W, act, s);
        else if (K == 5) launch_dw_pair_t<5>(in, wdup, b, out, N, C, H, W, act, s);
        else launch_dw_pair_t<3>(in, wdup, b, out, N, C, H, W, act, s);
        return;
    }
    if (K == 7 && S == 1) launch_dw_t<7, 1>(in, w, wdup, b, out, N, C, H, W, act, s);
    else if (K == 7 && S == 2) launch_dw_t<7, 2>(in, w, wdup, b, out, N, C, H, W, act, s);
    else if (K == 5 && S == 1) launch_dw_t<5, 1>(in, w, wdup, b, out, N, C, H, W, act, s);
    else if (K == 5 && S == 2) launch_dw_t<5, 2>(in, w, wdup, b, out, N, C, H, W, act, s);
    else if (K == 3 && S == 1) launch_dw_t<3, 1>(in, w, wdup, b, out, N, C, H, W, act, s);
    else if (K == 3 && S == 2) launch_dw_t<3, 2>(in, w, wdup, b, out, N, C, H, W, act, s);
}

// =====================================================================================
// pointwise 1x1 as an exact-fp32 MFMA GEMM:  D[co][px] = sum_k W[co][k] * X[k][px]
//   v_mfma_f32_32x32x2_f32:  A lane l = W[co0 + (l&31)][k0 + (l>>5)]   (packed on host,
//                            one contiguous 256-byte load per fragment, L1/L2 resident)
//                            B lane l = X[k0 + (l>>5)][column (l&31)]  (coalesced rows
//                            straight from HBM, no LDS)
//   D reg r of lane l     -> co = co0 + (r&3) + 8*(r>>2) + 4*(l>>5),  column l&31
// Fused epilogue: + bias, act, + residual.
// =====================================================================================
// -------------------------------------------------------------------------------------
// One wave = PXV*32 pixels x NB*32 output channels.
// Each lane loads PXV CONSECUTIVE pixels of channel (2kp + lane>>5) with one 16-byte
// (PXV=4) load -- 512 contiguous bytes per half-wave -- and feeds component v to MFMA
// "column set" v (the MFMA column index j = lane&31 may be any pixel permutation as long
// as the epilogue uses the same one: set v, column j  <->  pixel 4j + v).  The epilogue
// then owns 4 consecutive pixels per lane and stores/loads (residual) 16 bytes per lane.
// A fragments (packed weights) and B vectors are double-buffered in registers CH k-pairs
// ahead so that >= 4 KB of HBM loads per wave are in flight behind the MFMA stream.
// -------------------------------------------------------------------------------------
template <int PXV> struct PxVec;
template <> struct PxVec<4> { typedef f32x4 type; };
template <> struct PxVec<2> { typedef float type __attribute__((ext_vector_type(2))); };
template <> struct PxVec<1> { typedef float type __attribute__((ext_vector_type(1))); };

template <int NB, int PXV, bool RES>
__global__ __launch_bounds__(256) void pw2_kernel(const float* __restrict__ inA, int Ca,
                                                  const float* __restrict__ inB, int Cb,
                                                  const float* __restrict__ wp,
                                                  const float* __restrict__ bias,
                                                  const float* __restrict__ res,
                                                  float* __restrict__ out, long NG, int HWV, int HW,
                                                  int Cout, int act) {
    typedef typename PxVec<PXV>::type vec_t;
    constexpr int CH = 4;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const long g0 = ((long)blockIdx.x * 4 + wave) * 32;
    if (g0 >= NG) return;
    const int half = lane >> 5, pl = lane & 31;
    const long g = g0 + pl;
    const bool valid = g < NG;
    const long gc = valid ? g : NG - 1;
    const int n = (int)(gc / HWV);
    const int p = (int)(gc - (long)n * HWV) * PXV;
    const int KP = ((Ca + 1) >> 1) + ((Cb + 1) >> 1);        // pack_pw: the k-pairs of each source, an odd one padded
    const int cb0 = blockIdx.y * NB;
    const int cblocks = (Cout + 31) >> 5;

    f32x16 acc[NB][PXV];
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int v = 0; v < PXV; ++v)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][v][r] = 0.f;

    const float* wl[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) wl[i] = wp + (long)min(cb0 + i, cblocks - 1) * KP * 64 + lane;
    // bias in D-fragment order (packed on host: [cblock][half][16]), fetched up front
    f32x4 bfr[NB][4];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const f32x4* bp = reinterpret_cast<const f32x4*>(bias + ((long)min(cb0 + i, cblocks - 1) * 2 + half) * 16);
#pragma unroll
        for (int q = 0; q < 4; ++q) bfr[i][q] = bp[q];
    }

#pragma unroll 1
    for (int srcsel = 0; srcsel < 2; ++srcsel) {
        const int C = srcsel == 0 ? Ca : Cb;
        if (C == 0) continue;
        const float* sp = (srcsel == 0 ? inA : inB) + ((long)n * C + half) * HW + p;
        const int kofs = srcsel == 0 ? 0 : ((Ca + 1) >> 1);
        const int nkp = C >> 1;
        const int nch = nkp / CH;
        vec_t bc[CH], bn[CH];
        float ac[CH][NB], an[CH][NB];
        if (nch > 0) {
#pragma unroll
            for (int j = 0; j < CH; ++j) {
                bc[j] = *reinterpret_cast<const vec_t*>(sp + (long)(2 * j) * HW);
#pragma unroll
                for (int i = 0; i < NB; ++i) ac[j][i] = wl[i][(long)(kofs + j) * 64];
            }
        }
#pragma unroll 1
        for (int c = 0; c < nch; ++c) {
            const bool more = c + 1 < nch;
            if (more) {
                const int k0 = (c + 1) * CH;
#pragma unroll
                for (int j = 0; j < CH; ++j) {
                    bn[j] = *reinterpret_cast<const vec_t*>(sp + (long)(2 * (k0 + j)) * HW);
#pragma unroll
                    for (int i = 0; i < NB; ++i) an[j][i] = wl[i][(long)(kofs + k0 + j) * 64];
                }
            }
#pragma unroll
            for (int j = 0; j < CH; ++j)
#pragma unroll
                for (int i = 0; i < NB; ++i)
#pragma unroll
                    for (int v = 0; v < PXV; ++v)
                        acc[i][v] = __builtin_amdgcn_mfma_f32_32x32x2f32(ac[j][i], bc[j][v], acc[i][v], 0, 0, 0);
            if (more) {
#pragma unroll
                for (int j = 0; j < CH; ++j) {
                    bc[j] = bn[j];
#pragma unroll
                    for (int i = 0; i < NB; ++i) ac[j][i] = an[j][i];
                }
            }
        }
        for (int kp = nch * CH; kp < nkp; ++kp) {          // K/2 not a multiple of CH
            const vec_t bv = *reinterpret_cast<const vec_t*>(sp + (long)(2 * kp) * HW);
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const float av = wl[i][(long)(kofs + kp) * 64];
#pragma unroll
                for (int v = 0; v < PXV; ++v)
                    acc[i][v] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[v], acc[i][v], 0, 0, 0);
            }
        }
        if (C & 1) {                                        // the last channel alone: its absent partner is a zero
            vec_t bv;                                       // operand (its weight is zero too) and is never loaded
#pragma unroll
            for (int v = 0; v < PXV; ++v) bv[v] = 0.f;
            if (half == 0) bv = *reinterpret_cast<const vec_t*>(sp + (long)(2 * nkp) * HW);
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const float av = wl[i][(long)(kofs + nkp) * 64];
#pragma unroll
                for (int v = 0; v < PXV; ++v)
                    acc[i][v] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[v], acc[i][v], 0, 0, 0);
            }
        }
    }
    if (!valid) return;
    // branch-free activation: clamp to [lo, hi]
    const float lo = act == ACT_NONE ? ACT_NONE_BOUND : 0.f;
    const float hi = act == ACT_RELU6 ? 6.f : (act == ACT_NONE ? ACT_NONE_BOUND : INFINITY);
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int cob = (cb0 + i) * 32 + 4 * half;
        if (cb0 + i >= cblocks) break;
        float* ob = out + ((long)n * Cout + cob) * HW + p;
        const float* rb = RES ? res + ((long)n * Cout + cob) * HW + p : nullptr;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int dco = (r & 3) + 8 * (r >> 2);
            if (cob + dco < Cout) {
                const float bb = bfr[i][r >> 2][r & 3];
                vec_t v;
#pragma unroll
                for (int e = 0; e < PXV; ++e) v[e] = fminf(fmaxf(acc[i][e][r] + bb, lo), hi);
                if (RES) {
                    const vec_t rr = *reinterpret_cast<const vec_t*>(rb + (long)dco * HW);
#pragma unroll
                    for (int e = 0; e < PXV; ++e) v[e] += rr[e];
                }
                *reinterpret_cast<vec_t*>(ob + (long)dco * HW) = v;
            }
        }
    }
}

// -------------------------------------------------------------------------------------
// pw3: the same 1x1 GEMM for COMPUTE-bound layers (16x16 / 32x32 planes, K or Cout >= 192),
// where the fp32 matrix-core rate (157 TF, 1/16 of bf16) is the limit.  Every fp32 value is
// split EXACTLY into three bf16 pieces (8+8+8 mantissa bits by truncation:
//   hi = x & 0xffff0000, mid = (x-hi) & 0xffff0000, lo = x-hi-mid, all subtractions exact),
// weights on the host, activations in registers, and the product is evaluated as the six
// bf16 MFMAs whose weight is >= 2^-16:  hh + hm + mh + hl + lh + mm  (dropped: ml+lm+ll
// <= 3*2^-24 relative, the size of one fp32 rounding).  v_mfma_f32_32x32x16_bf16 does 16 k
// in 32 cycles against 2 k in 64 cycles for the fp32 form: 6 passes -> 2.67x the fp32-MFMA
// rate at fp32 accuracy (products of bf16 pairs are exact in fp32, accumulation is fp32).
// Fragment = 8 consecutive k per lane: channels k0 + 8*(lane>>5) + 0..7 of pixel column
// lane&31, so the planar layout still loads 16-byte coalesced rows (one per channel).
// -------------------------------------------------------------------------------------
typedef short bf16x8_t __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

template <int PXV, bool RES>
__global__ __launch_bounds__(256) void pw3_kernel(const float* __restrict__ inA, int C,
                                                  const u32x4* __restrict__ wsp,   // [cb][ks][3][64] x4 dw
                                                  const float* __restrict__ bias,
                                                  const float* __restrict__ res,
                                                  float* __restrict__ out, long NG, int HWV, int HW,
                                                  int Cout, int act) {
    constexpr int NB = 1;                                  // channel blocks of 32 per wave: most waves, shortest chains
    typedef typename PxVec<PXV>::type vec_t;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const long g0 = ((long)blockIdx.x * 4 + wave) * 32;
    if (g0 >= NG) return;
    const int half = lane >> 5, pl = lane & 31;
    const long g = g0 + pl;
    const bool valid = g < NG;
    const long gc = valid ? g : NG - 1;
    const int n = (int)(gc / HWV);
    const int p = (int)(gc - (long)n * HWV) * PXV;
    const int KS = C >> 4;
    const int cb0 = blockIdx.y * NB;
    const int cblocks = (Cout + 31) >> 5;

    f32x16 acc[NB][PXV];
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int v = 0; v < PXV; ++v)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][v][r] = 0.f;
    f32x4 bfr[NB][4];
    const u32x4* wl[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int cb = min(cb0 + i, cblocks - 1);
        const f32x4* bp = reinterpret_cast<const f32x4*>(bias + ((long)cb * 2 + half) * 16);
#pragma unroll
        for (int q = 0; q < 4; ++q) bfr[i][q] = bp[q];
        wl[i] = wsp + (long)cb * KS * 3 * 64 + lane;
    }
    const float* sp = inA + ((long)n * C + 8 * half) * HW + p;
    vec_t bq[8], bn[8];
    u32x4 aq[NB][3], an[NB][3];
#pragma unroll
    for (int c = 0; c < 8; ++c) bq[c] = *reinterpret_cast<const vec_t*>(sp + (long)c * HW);
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int t = 0; t < 3; ++t) aq[i][t] = wl[i][t * 64];
#pragma unroll 1
    for (int ks = 0; ks < KS; ++ks) {
        const bool more = ks + 1 < KS;
        if (more) {
#pragma unroll
            for (int c = 0; c < 8; ++c)
                bn[c] = *reinterpret_cast<const vec_t*>(sp + (long)((ks + 1) * 16 + c) * HW);
#pragma unroll
            for (int i = 0; i < NB; ++i)
#pragma unroll
                for (int t = 0; t < 3; ++t) an[i][t] = wl[i][((long)(ks + 1) * 3 + t) * 64];
        }
        // exact 3-way bf16 split of the 8 channels x 4 pixels held by this lane
        u32x4 fh[PXV], fm[PXV], fl[PXV];
#pragma unroll
        for (int v = 0; v < PXV; ++v)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float x0 = bq[2 * j][v], x1 = bq[2 * j + 1][v];
                const unsigned u0 = __float_as_uint(x0), u1 = __float_as_uint(x1);
                const float r0 = x0 - __uint_as_float(u0 & 0xffff0000u);
                const float r1 = x1 - __uint_as_float(u1 & 0xffff0000u);
                const unsigned m0 = __float_as_uint(r0), m1 = __float_as_uint(r1);
                const float s0 = r0 - __uint_as_float(m0 & 0xffff0000u);
                const float s1 = r1 - __uint_as_float(m1 & 0xffff0000u);
                fh[v][j] = __builtin_amdgcn_perm(u1, u0, 0x07060302u);
                fm[v][j] = __builtin_amdgcn_perm(m1, m0, 0x07060302u);
                fl[v][j] = __builtin_amdgcn_perm(__float_as_uint(s1), __float_as_uint(s0), 0x07060302u);
            }
#define LP_MM(AT, BT)                                                                               \
    _Pragma("unroll") for (int i = 0; i < NB; ++i) _Pragma("unroll") for (int v = 0; v < PXV; ++v)  \
        acc[i][v] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, aq[i][AT]), \
                                                            __builtin_bit_cast(bf16x8_t, BT[v]), acc[i][v], 0, 0, 0)
        LP_MM(2, fh);      // lo*hi   (smallest terms first)
        LP_MM(0, fl);      // hi*lo
        LP_MM(1, fm);      // mid*mid
        LP_MM(1, fh);      // mid*hi
        LP_MM(0, fm);      // hi*mid
        LP_MM(0, fh);      // hi*hi
#undef LP_MM
        if (more) {
#pragma unroll
            for (int c = 0; c < 8; ++c) bq[c] = bn[c];
#pragma unroll
            for (int i = 0; i < NB; ++i)
#pragma unroll
                for (int t = 0; t < 3; ++t) aq[i][t] = an[i][t];
        }
    }
    if (!valid) return;
    const float lo = act == ACT_NONE ? -INFINITY : 0.f;
    const float hi = act == ACT_RELU6 ? 6.f : INFINITY;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int cob = (cb0 + i) * 32 + 4 * half;
        if (cb0 + i >= cblocks) break;
        float* ob = out + ((long)n * Cout + cob) * HW + p;
        const float* rb = RES ? res + ((long)n * Cout + cob) * HW + p : nullptr;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int dco = (r & 3) + 8 * (r >> 2);
            if (cob + dco < Cout) {
                const float bb = bfr[i][r >> 2][r & 3];
                vec_t v;
#pragma unroll
                for (int e = 0; e < PXV; ++e) v[e] = fminf(fmaxf(acc[i][e][r] + bb, lo), hi);
                if (RES) {
                    const vec_t rr = *reinterpret_cast<const vec_t*>(rb + (long)dco * HW);
#pragma unroll
                    for (int e = 0; e < PXV; ++e) v[e] += rr[e];
                }
                *reinterpret_cast<vec_t*>(ob + (long)dco * HW) = v;
            }
        }
    }
}

// pw3d (round 6): pw3_kernel for SMALL launches (a few images: the reference's own operating point is batch 1).  There a
// layer is a handful of workgroups -- nothing hides a load behind another wave -- and pw3_kernel's one-step-ahead prefetch
// leaves every k-step waiting on an L2 round trip: 16 us for the K = 480 project of two images, ~1100 cycles per k-step for
// 12 MFMAs.  Here the loads run D k-steps ahead through a ring of register stages and a wave owns 32 pixels (PXV = 1: most
// waves, shortest chain).  Same fragments, same six products per k-step in the same order, k-steps in the same order:
// bit-identical to pw3_kernel (and so to mb16_kernel), which a GPU test asserts -- the parity protocol's P4 (a batched run
// equals the per-image runs bit for bit) does not depend on which of the two a launch takes.
template <bool RES>
__global__ __launch_bounds__(256) void pw3d_kernel(const float* __restrict__ inA, int C, const u32x4* __restrict__ wsp,
                                                   const float* __restrict__ bias, const float* __restrict__ res,
                                                   float* __restrict__ out, long NG, int HWV, int HW, int Cout, int act) {
    constexpr int NB = 1, PXV = 1, D = 4;                  // one channel block, 32 pixels per wave, loads 4 k-steps ahead
    typedef typename PxVec<PXV>::type vec_t;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const long g0 = ((long)blockIdx.x * 4 + wave) * 32;
    if (g0 >= NG) return;
    const int half = lane >> 5, pl = lane & 31;
    const long g = g0 + pl;
    const bool valid = g < NG;
    const long gc = valid ? g : NG - 1;
    const int n = (int)(gc / HWV);
    const int p = (int)(gc - (long)n * HWV) * PXV;
    const int KS = C >> 4;
    const int cb0 = blockIdx.y * NB;
    const int cblocks = (Cout + 31) >> 5;

    f32x16 acc[NB][PXV];
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int v = 0; v < PXV; ++v)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][v][r] = 0.f;
    const u32x4* wl[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) wl[i] = wsp + (long)min(cb0 + i, cblocks - 1) * KS * 3 * 64 + lane;
    const float* sp = inA + ((long)n * C + 8 * half) * HW + p;
    vec_t bq[D][8];
    u32x4 aq[D][NB][3];
    auto load_b = [&](vec_t (&dst)[8], int ks) {
        const int kc = min(ks, KS - 1);                               // the tail re-requests the last step: harmless
#pragma unroll
        for (int c = 0; c < 8; ++c) dst[c] = *reinterpret_cast<const vec_t*>(sp + (long)(kc * 16 + c) * HW);
    };
    auto load_a = [&](u32x4 (&dst)[NB][3], int ks) {
        const int kc = min(ks, KS - 1);
#pragma unroll
        for (int i = 0; i < NB; ++i)
#pragma unroll
            for (int t = 0; t < 3; ++t) dst[i][t] = wl[i][((long)kc * 3 + t) * 64];
    };
#pragma unroll
    for (int d = 0; d < D; ++d) {
        load_b(bq[d], d);
        load_a(aq[d], d);
    }
#pragma unroll 1
    for (int ks0 = 0; ks0 < KS; ks0 += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int ks = ks0 + d;
            if (ks < KS) {                                            // wave-uniform
                u32x4 fh[PXV], fm[PXV], fl[PXV];
#pragma unroll
                for (int v = 0; v < PXV; ++v)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float x0 = bq[d][2 * j][v], x1 = bq[d][2 * j + 1][v];
                        const unsigned u0 = __float_as_uint(x0), u1 = __float_as_uint(x1);
                        const float r0 = x0 - __uint_as_float(u0 & 0xffff0000u);
                        const float r1 = x1 - __uint_as_float(u1 & 0xffff0000u);
                        const unsigned m0 = __float_as_uint(r0), m1 = __float_as_uint(r1);
                        const float s0 = r0 - __uint_as_float(m0 & 0xffff0000u);
                        const float s1 = r1 - __uint_as_float(m1 & 0xffff0000u);
                        fh[v][j] = __builtin_amdgcn_perm(u1, u0, 0x07060302u);
                        fm[v][j] = __builtin_amdgcn_perm(m1, m0, 0x07060302u);
                        fl[v][j] = __builtin_amdgcn_perm(__float_as_uint(s1), __float_as_uint(s0), 0x07060302u);
                    }
                load_b(bq[d], ks + D);                                // this stage's pixels are split: refill it
#define LP_MMD(AT, BT)                                                                                  \
    _Pragma("unroll") for (int i = 0; i < NB; ++i) _Pragma("unroll") for (int v = 0; v < PXV; ++v)      \
        acc[i][v] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, aq[d][i][AT]), \
                                                            __builtin_bit_cast(bf16x8_t, BT[v]), acc[i][v], 0, 0, 0)
                LP_MMD(2, fh);     // pw3_kernel's order: lo*hi, hi*lo, mid*mid, mid*hi, hi*mid, hi*hi
                LP_MMD(0, fl);
                LP_MMD(1, fm);
                LP_MMD(1, fh);
                LP_MMD(0, fm);
                LP_MMD(0, fh);
#undef LP_MMD
                load_a(aq[d], ks + D);
            }
        }
    }
    if (!valid) return;
    const float lo = act == ACT_NONE ? -INFINITY : 0.f;
    const float hi = act == ACT_RELU6 ? 6.f : INFINITY;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int cob = (cb0 + i) * 32 + 4 * half;
        if (cb0 + i >= cblocks) break;
        float* ob = out + ((long)n * Cout + cob) * HW + p;
        const float* rb = RES ? res + ((long)n * Cout + cob) * HW + p : nullptr;
        const f32x4* bp = reinterpret_cast<const f32x4*>(bias + ((long)(cb0 + i) * 2 + half) * 16);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int dco = (r & 3) + 8 * (r >> 2);
            if (cob + dco < Cout) {
                const float bb = bp[r >> 2][r & 3];
                vec_t v;
#pragma unroll
                for (int e = 0; e < PXV; ++e) v[e] = fminf(fmaxf(acc[i][e][r] + bb, lo), hi);
                if (RES) {
                    const vec_t rr = *reinterpret_cast<const vec_t*>(rb + (long)dco * HW);
#pragma unroll
                    for (int e = 0; e < PXV; ++e) v[e] += rr[e];
                }
                *reinterpret_cast<vec_t*>(ob + (long)dco * HW) = v;
            }
        }
    }
}

// both bf16x3 forms: one workgroup = 4 waves x 32 pixel groups, one 32-channel block per wave (grid.y = the blocks)
static void launch_pw3d(const float* inA, int C, const void* wsp, const float* b, const float* res,
                        float* out, long NP, int HW, int Cout, int act, hipStream_t s) {
    dim3 grid((unsigned)((NP + 127) / 128), (Cout + 31) / 32), block(256);
    last_kernel_tag = "pw3d_kernel";
    if (res)
        LP_LAUNCH(pw3d_kernel<true>, grid, block, 0, s, inA, C, (const u32x4*)wsp, b, res, out, NP, HW, HW, Cout, act);
    else
        LP_LAUNCH(pw3d_kernel<false>, grid, block, 0, s, inA, C, (const u32x4*)wsp, b, res, out, NP, HW, HW, Cout, act);
}

template <int PXV>
static void launch_pw3_t(const float* inA, int C, const void* wsp, const float* b, const float* res,
                         float* out, long NP, int HW, int Cout, int act, hipStream_t s) {
    const long NG = NP / PXV;
    dim3 grid((unsigned)((NG + 127) / 128), (Cout + 31) / 32), block(256);
    last_kernel_tag = "pw3_kernel";
    if (res)
        LP_LAUNCH((pw3_kernel<PXV, true>), grid, block, 0, s, inA, C, (const u32x4*)wsp, b, res,
                           out, NG, HW / PXV, HW, Cout, act);
    else
        LP_LAUNCH((pw3_kernel<PXV, false>), grid, block, 0, s, inA, C, (const u32x4*)wsp, b, res,
                           out, NG, HW / PXV, HW, Cout, act);
}

template <int NB, int PXV>
static void launch_pw2_t(const float* inA, int Ca, const float* inB, int Cb, const float* wp,
                         const float* b, const float* res, float* out, long NP, int HW, int Cout,
                         int act, hipStream_t s) {
    const long NG = NP / PXV;
    const int cblocks = (Cout + 31) / 32;
    dim3 grid((unsigned)((NG + 127) / 128), (cblocks + NB - 1) / NB), block(256);
    last_kernel_tag = "pw2_kernel";
    if (res)
        LP_LAUNCH((pw2_kernel<NB, PXV, true>), grid, block, 0, s, inA, Ca, inB, Cb, wp, b, res, out,
                           NG, HW / PXV, HW, Cout, act);
    else
        LP_LAUNCH((pw2_kernel<NB, PXV, false>), grid, block, 0, s, inA, Ca, inB, Cb, wp, b, res, out,
                           NG, HW / PXV, HW, Cout, act);
}

// Tile choice of the fp32 MFMA 1x1 (pw2_kernel<NB, PXV>): a wave owns PXV*32 pixels x NB*32 channels.  PXV is as wide as
// the plane size allows (16-byte loads/stores); NB in {1,2,3} minimises a small cost model fitted to a sweep on MI355X
// (profiles/r01_pw_tile_sweep.txt):
//   time ~ rounds(waves / (1024 SIMDs * occupancy)) * (occupancy_used * mfma_cycles + overhead)
// Host arithmetic only: launch_pw's one source of the choice, and what lp_pw_tile_choice reports.
PwTile pw_tile_choice(int N, int Ca, int Cb, int Cout, int HW, bool has_res) {
    const long NP = (long)N * HW;
    const int cblocks = (Cout + 31) / 32;
    PwTile t{1, (HW % 4 == 0) ? 4 : (HW % 2 == 0 ? 2 : 1)};
    const int PXV = t.PXV;
    const long ptiles = (NP / PXV + 31) / 32;
    const int KP = (Ca + Cb) / 2;
    double best = 1e300;
    for (int nb = 1; nb <= 3 && nb <= cblocks; ++nb) {
        const long waves = ptiles * ((cblocks + nb - 1) / nb);
        const int regs = nb * PXV * 16 * 2 + 32;                       // VGPR+AGPR estimate
        const int occ = regs <= 128 ? 4 : (regs <= 168 ? 3 : (regs <= 256 ? 2 : 1));
        const long slots = 1024L * occ;
        const long rounds = (waves + slots - 1) / slots;
        const double per_simd = (double)waves / 1024.0 / rounds;       // waves sharing a SIMD
        const double used = per_simd < 1.0 ? 1.0 : (per_simd > occ ? occ : per_simd);
        const double t_mfma = rounds * (used * (double)KP * nb * PXV * 64.0 + 8000.0);
        // HBM term: the input is re-read once per channel group; ~2.3 B/cycle/SIMD at 5 TB/s
        const double bytes = (double)NP * 4.0 * ((double)(Ca + Cb) * ((cblocks + nb - 1) / nb) +
                                                 (double)Cout * (has_res ? 2 : 1));
        const double t_mem = bytes / (1024.0 * 2.3);
        const double tt = t_mfma > t_mem ? t_mfma : t_mem;
        if (tt < best * 0.999) { best = tt; t.NB = nb; }
    }
    return t;
}

void launch_pw(const float* inA, int Ca, const float* inB, int Cb, const float* wp, const float* b,
               const float* res, float* out, int N, int HW, int Cout, int act, hipStream_t s,
               const void* wsplit, int pw3d_mode) {
    const long NP = (long)N * HW;
    const int cblocks = (Cout + 31) / 32;
    const PwTile tile = pw_tile_choice(N, Ca, Cb, Cout, HW, res != nullptr);
    const int PXV = tile.PXV, NB = tile.NB;
    bool bound_mfma = false;
    // compute-bound under fp32 MFMA -> exact bf16x3 split kernel (2.67x the matrix-core rate).
    // The choice depends on the LAYER SHAPE only (arithmetic intensity K*Cout/(K+Cout) in MAC per
    // element moved; fp32-MFMA balance ~ 31 FLOP/B), never on the batch size, so that a batched run
    // is bit-identical to the per-image run (parity protocol P4).
    bound_mfma = (double)Ca * Cout / (double)(Ca + Cout) >= 36.0;
    if (bound_mfma && wsplit && Cb == 0 && (Ca & 15) == 0 && PXV == 4) {
        {
            // tile choice from the sweep in profiles/r01_pw3_tile_sweep.txt: one channel block per
            // wave (most waves, shortest chains); 64-pixel tiles for the project layers and the
            // narrow expands, 128-pixel tiles for the wide-K expands
            // option "pw3d": small launches (<= 8192 pixels: 16 images of a 16x16 plane) take the deep-prefetch form, which is
            // bit-identical (1 = by that rule, 2 = always, 0 = never)
            if (pw3d_mode == 2 || (pw3d_mode == 1 && NP <= 8192)) {
                launch_pw3d(inA, Ca, wsplit, b, res, out, NP, HW, Cout, act, s);
                return;
            }
            const int pxv3 = (cblocks <= 3 || Ca < 64) ? 2 : 4;
            if (pxv3 == 2) launch_pw3_t<2>(inA, Ca, wsplit, b, res, out, NP, HW, Cout, act, s);
            else launch_pw3_t<4>(inA, Ca, wsplit, b, res, out, NP, HW, Cout, act, s);
            return;
        }
    }
#define LP_GO(NBV, PV) launch_pw2_t<NBV, PV>(inA, Ca, inB, Cb, wp, b, res, out, NP, HW, Cout, act, s)
    if (PXV == 4) { if (NB == 3) LP_GO(3, 4); else if (NB == 2) LP_GO(2, 4); else LP_GO(1, 4); }
    else if (PXV == 2) { if (NB == 3) LP_GO(3, 2); else if (NB == 2) LP_GO(2, 2); else LP_GO(1, 2); }
    else { if (NB == 3) LP_GO(3, 1); else if (NB == 2) LP_GO(2, 1); else LP_GO(1, 1); }
#undef LP_GO
}

// =====================================================================================
// Fused depthwise + project (the second half of an InvBottleneck, layers.py:100-117):
//   out = W2 . relu6(dw_KxK(E) + b_dw) + b2 (+ x)
// The depthwise result never goes to HBM: one workgroup owns a 16x16 output tile of one
// image and walks the expanded channels in chunks of 32:
//   phase 1  each wave runs the LDS-tiled depthwise (same inner loop as dw_kernel) for
//            8 of the 32 channels and parks the 256 activated outputs of each channel in a
//            32 KB LDS chunk buffer  DW[32 ch][256 px]
//   phase 2  the chunk is the K-slice of the 1x1: wave w owns tile pixels [64w, 64w+64)
//            (32 lanes x 2 px, ds_read_b64 straight into MFMA B operands) and accumulates
//            D[NB*32 co][64 px] += W2[:, chunk] . DW  on the fp32 matrix cores
// epilogue: + bias (+ residual), 8-byte stores.  HBM traffic per block drops from
// E-read + DW-write + DW-read + out-write to E-read + out-write.
// =====================================================================================
// Diagnostic record of dwpw_kernel<..., DIAG = true> (lp_net_set_option "diag_dwpw", tools/flake_hunt.py --diag): the
// kernel fetches its project bias BOTH ways -- as the half-broadcast 16-byte vector loads of round 3's builds and
// through the scalar cache -- compares them lane by lane and logs every disagreement.  Word 0 = number of events;
// 16 words per event (see the kernel).
// Round 5: the variant, its log and the host read exist only in the DIAGNOSTICS FLAVOUR of the library
// (python -m litepose_amd.build --flavour diag -> lib/liblitepose_amd_diag.so, -DLP_DIAG_BUILD): it is the one kernel that
// keeps the erratum-prone v_pk_add_f32 op_sel:[0,1] on purpose, and the product library must not link it.
#ifdef LP_DIAG_BUILD
__device__ unsigned lp_dwpw_diag_log[1 + 16 * 256];
#endif

template <int K, int S, int NB, bool RES, bool DIAG = false>
__global__ __launch_bounds__(256) void dwpw_kernel(const float* __restrict__ in,     // E [N,C,H,W]
                                                   const float* __restrict__ wdw,    // [C][K*K]
                                                   const float* __restrict__ bdw,    // [C]
                                                   const float* __restrict__ wp,     // A frags
                                                   const float* __restrict__ bias,   // D-frag order
                                                   const float* __restrict__ res,    // [N,Cout,OH,OW]
                                                   float* __restrict__ out, int C, int H, int W,
                                                   int OH, int OW, int tilesX, int tilesY, int Cout,
                                                   int xcd_remap) {
    using G = DwGeom<K, S>;
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int CK = 32;
    float* dwb = smem;                                    // [CK][256]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* tile = smem + CK * 256 + wave * G::LDS_FLOATS;
    const int unit = (xcd_remap & 255) ? xcd_contiguous_id(blockIdx.x, gridDim.x) : blockIdx.x;
    const int tq = unit / tilesX;
    const int tx = unit - tq * tilesX;
    const int n = tq / tilesY;
    const int ty = tq - n * tilesY;
    const int ix0 = tx * 16 * S - 4, iy0 = ty * 16 * S - G::HALO;
    constexpr int QPR = G::QPR, NQ = G::IH * QPR, NLD = (NQ + 63) / 64;
    const int row = lane >> 2, strip = lane & 3;
    const int half = lane >> 5, pl = lane & 31;
    const int KP = C >> 1;
    const int cblocks = (Cout + 31) >> 5;

    f32x16 acc[NB][2];
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int v = 0; v < 2; ++v)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][v][r] = 0.f;
    // The bias reaches the lanes through the SCALAR cache (both halves' 16 values per filter block as wave-uniform s_load,
    // the lane's half picked with v_cndmask).  History: round 3 saw this kernel's output off by exactly one
    // folded bias in 16 pixels, one batch in 2000 - 12 000, and blamed the bias fetch -- then a 16-byte vector load whose
    // 32 lanes of a wave half ask for one address.  Round 4's self-checking variant (DIAG, option "diag_dwpw") showed
    // the fetched registers are right after the load AND right before their use while the output is still wrong: the add
    // itself lost its operand -- hipcc had built it as v_pk_add_f32 op_sel:[0,1], the gfx950 packed-fp32 form that returns
    // src0 + 0 in lanes 48-63 next to a bf16-MFMA wave on the same SIMD (tools/ubench/pk_vs_mfma.hip).  LDS-DMA, the first
    // suspect, was a bystander and stays the default weight staging of the fused blocks (fused_common.h: stage_issue).  The
    // scalar form stays: it is no slower, keeps 16 registers free, and makes hipcc emit a plain v_pk_add_f32.
    f32x4 bfr[NB][4];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const float* bl = bias + (long)min(i, cblocks - 1) * 32;              // wave-uniform address
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float lo = bl[4 * q + e], hi = bl[16 + 4 * q + e];
                bfr[i][q][e] = half ? hi : lo;
            }
    }
    f32x4 bsc[NB][4];                                      // DIAG: the scalar-cache copy, kept for the second check
    // DIAG: compare the vector-loaded bias registers with the scalar-cache copy, log every disagreement (where = 0 after
    // the load, 1 before the use in the epilogue) together with what an immediate re-fetch returns
    auto diag_check = [&](int where) {
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const f32x4* bp = reinterpret_cast<const f32x4*>(bias + (long)min(i, cblocks - 1) * 32 + 16 * half);
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const bool badl = __float_as_uint(bfr[i][q][e]) != __float_as_uint(bsc[i][q][e]);
                    const unsigned long long bm = __ballot(badl);
                    if (bm) {
                        f32x4 again;
                        asm volatile("global_load_dwordx4 %0, %1, off\n\ts_waitcnt vmcnt(0)" : "=v"(again) : "v"(bp + q));
                        const unsigned long long bm2 = __ballot(__float_as_uint(again[e]) != __float_as_uint(bsc[i][q][e]));
                        const int fl = __ffsll((long long)bm) - 1;
                        const unsigned got = __builtin_amdgcn_readlane(__float_as_uint(bfr[i][q][e]), fl);
                        const unsigned want = __builtin_amdgcn_readlane(__float_as_uint(bsc[i][q][e]), fl);
#ifdef LP_DIAG_BUILD
                        if (lane == 0) {
                            const unsigned k = atomicAdd(&lp_dwpw_diag_log[0], 1u);
                            if (k < 256) {
                                unsigned hw, xcc;
                                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
                                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
                                const unsigned long long t = __builtin_readcyclecounter();
                                unsigned* r = lp_dwpw_diag_log + 1 + 16 * k;
                                r[0] = blockIdx.x; r[1] = (unsigned)wave; r[2] = (16u * i + 4u * q + e) | ((unsigned)where << 8);
                                r[3] = (unsigned)bm; r[4] = (unsigned)(bm >> 32);
                                r[5] = (unsigned)bm2; r[6] = (unsigned)(bm2 >> 32);
                                r[7] = got; r[8] = want; r[9] = hw; r[10] = xcc;
                                r[11] = (unsigned)t; r[12] = (unsigned)(t >> 32); r[13] = (unsigned)K; r[14] = gridDim.x;
                                r[15] = (unsigned)Cout;
                            }
                        }
#else
                        (void)bm2; (void)got; (void)want;
#endif
                    }
                }
        }
    };
    if constexpr (DIAG) {
        // round 3's form of the same fetch (no register footprint, 96 registers): four 16-byte vector loads whose 32 lanes
        // of a wave half ask for ONE address, into the registers the epilogue adds; the kernel goes on with them, so a bad
        // dword also shows in the block's output.  diag >> 1: positive control of the log (one lane, one bit, after check 0)
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const f32x4* bp = reinterpret_cast<const f32x4*>(bias + (long)min(i, cblocks - 1) * 32 + 16 * half);
            f32x4 bv[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(bv[q]) : "v"(bp + q));
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(bv[0]), "+v"(bv[1]), "+v"(bv[2]), "+v"(bv[3]));
#pragma unroll
            for (int q = 0; q < 4; ++q) { bsc[i][q] = bfr[i][q]; bfr[i][q] = bv[q]; }
        }
        diag_check(0);
        if ((xcd_remap >> 8) == 2 && blockIdx.x == 5 && wave == 1 && lane == 37)
            bfr[0][2][3] = __uint_as_float(__float_as_uint(bfr[0][2][3]) ^ 0x00010000u);
    }

    // per-lane staging coordinates are the same for every channel
    int st_off[NLD];       // offset inside the plane (clamped), -1 = zero fill
    int st_lds[NLD];
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
        const int e = lane + 64 * i;
        const int r = e / QPR, q = e - r * QPR;
        const int iy = iy0 + r, ix = ix0 + 4 * q;
        const bool ok = e < NQ && iy >= 0 && iy < H && ix >= 0 && ix < W;
        st_off[i] = ok ? iy * W + ix : -1;
        st_lds[i] = e < NQ ? r * G::RS + 4 * q : -1;
    }
    const float* img = in + (long)n * C * H * W;
    f32x4 pre[NLD];
    auto issue = [&](int c) {
        const float* plane = img + (long)c * H * W;
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            f32x4 v = *reinterpret_cast<const f32x4*>(plane + max(st_off[i], 0));
            if (st_off[i] < 0) v = f32x4{0.f, 0.f, 0.f, 0.f};
            pre[i] = v;
        }
    };

    const int nchunks = C / CK;                            // C is a multiple of 32 here
    issue(wave);
    for (int ch = 0; ch < nchunks; ++ch) {
        // ---------------- phase 1: depthwise for channels ch*32 + wave + 4*t ----------
#pragma unroll 1
        for (int t = 0; t < CK / 4; ++t) {
            const int cc = wave + 4 * t;                   // channel inside the chunk
            const int c = ch * CK + cc;
#pragma unroll
            for (int i = 0; i < NLD; ++i)
                if (st_lds[i] >= 0) *reinterpret_cast<f32x4*>(tile + st_lds[i]) = pre[i];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            {   // prefetch the next channel this wave will process
                int nc = c + 4;
                if (t == CK / 4 - 1) nc = (ch + 1) * CK + wave;
                if (nc < C) issue(nc);
            }
            const float* wc = wdw + (long)c * K * K;
            float a4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ky = 0; ky < K; ++ky) {
                const float* lr = tile + (row * S + ky) * G::RS + strip * 4 * S;
                float v[4 * G::NV];
#pragma unroll
                for (int q = 0; q < G::NV; ++q) {
                    f32x4 tt = *reinterpret_cast<const f32x4*>(lr + 4 * q);
                    keep_b128(tt);
                    v[4 * q + 0] = tt[0]; v[4 * q + 1] = tt[1]; v[4 * q + 2] = tt[2]; v[4 * q + 3] = tt[3];
                }
#pragma unroll
                for (int kx = 0; kx < K; ++kx) {
                    const float wk = wc[ky * K + kx];
#pragma unroll
                    for (int i = 0; i < 4; ++i) a4[i] = fmaf(v[(4 - G::HALO) + kx + i * S], wk, a4[i]);
                }
            }
            const float bb = bdw[c];
            f32x4 o4;
#pragma unroll
            for (int i = 0; i < 4; ++i) o4[i] = fminf(fmaxf(a4[i] + bb, 0.f), 6.f);
            *reinterpret_cast<f32x4*>(dwb + cc * 256 + lane * 4) = o4;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        __syncthreads();
        // ---------------- phase 2: D += W2[:, chunk] . DW  (K-slice of 16 k-pairs) -----
        {
            const float* bsrc = dwb + half * 256 + wave * 64 + 2 * pl;
            const float* asrc = wp + (long)(ch * (CK / 2)) * 64 + lane;
#pragma unroll 4
            for (int kp = 0; kp < CK / 2; ++kp) {
                const f32x2 bv = *reinterpret_cast<const f32x2*>(bsrc + kp * 512);
#pragma unroll
                for (int i = 0; i < NB; ++i) {
                    const float av = asrc[((long)min(i, cblocks - 1) * KP + kp) * 64];
                    acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[0], acc[i][0], 0, 0, 0);
                    acc[i][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[1], acc[i][1], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }
    // ---------------- epilogue ---------------------------------------------------------
    if constexpr (DIAG) diag_check(1);                     // are the bias registers still what was loaded?
    const int p0 = wave * 64 + 2 * pl;                     // first of this lane's 2 tile pixels
    const int oy = ty * 16 + (p0 >> 4), ox = tx * 16 + (p0 & 15);
    if (oy >= OH || ox >= OW) return;
    const bool two = ox + 1 < OW;
    const long HWo = (long)OH * OW;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        if (i >= cblocks) break;
        const int cob = i * 32 + 4 * half;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = cob + (r & 3) + 8 * (r >> 2);
            if (co < Cout) {
                const float bb = bfr[i][r >> 2][r & 3];
                const long o = ((long)n * Cout + co) * HWo + (long)oy * OW + ox;
                float v0 = acc[i][0][r] + bb, v1 = acc[i][1][r] + bb;
                if (two && (OW & 1) == 0) {
                    if (RES) {
                        const f32x2 rr = *reinterpret_cast<const f32x2*>(res + o);
                        v0 += rr[0];
                        v1 += rr[1];
                    }
                    *reinterpret_cast<f32x2*>(out + o) = f32x2{v0, v1};
                } else {
                    if (RES) v0 += res[o];
                    out[o] = v0;
                    if (two) {
                        if (RES) v1 += res[o + 1];
                        out[o + 1] = v1;
                    }
                }
            }
        }
    }
}

template <int K, int S, int NB>
static void launch_dwpw_t(const float* in, const float* wdw, const float* bdw, const float* wp,
                          const float* bias, const float* res, float* out, int N, int C, int H, int W,
                          int Cout, hipStream_t s, int diag = 0) {
    const int OH = (H + 2 * (K / 2) - K) / S + 1, OW = (W + 2 * (K / 2) - K) / S + 1;
    const int tilesX = (OW + 15) / 16, tilesY = (OH + 15) / 16;
    const int grid = N * tilesX * tilesY;
    last_kernel_tag = "dwpw_kernel";
    const size_t lds = (size_t)(32 * 256 + 4 * DwGeom<K, S>::LDS_FLOATS) * sizeof(float);
#ifdef LP_DIAG_BUILD
    if constexpr (K == 3) {
        if (diag && !res) {                                   // the stem's dw3 + 1x1 with the self-checking bias fetch
            LP_LAUNCH((dwpw_kernel<K, S, NB, false, true>), dim3(grid), dim3(256), lds, s, in, wdw, bdw, wp,
                               bias, res, out, C, H, W, OH, OW, tilesX, tilesY, Cout, xcd_remap_mode() | (diag << 8));
            return;
        }
    }
#else
    (void)diag;                                               // rejected by lp_net_set_option in the product library
#endif
    if (res)
        LP_LAUNCH((dwpw_kernel<K, S, NB, true>), dim3(grid), dim3(256), lds, s, in, wdw, bdw, wp,
                           bias, res, out, C, H, W, OH, OW, tilesX, tilesY, Cout, xcd_remap_mode());
    else
        LP_LAUNCH((dwpw_kernel<K, S, NB, false>), dim3(grid), dim3(256), lds, s, in, wdw, bdw, wp,
                           bias, res, out, C, H, W, OH, OW, tilesX, tilesY, Cout, xcd_remap_mode());
}

// NOT during a stream capture: the symbol copies are synchronous runtime calls and would invalidate it.
int dwpw_diag_read(unsigned* host, int cap_words, bool clear) {
#ifndef LP_DIAG_BUILD
    (void)host; (void)cap_words; (void)clear;
    return -2;                                                // no diagnostic variant in this library
#else
    unsigned n = 0;
    if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(lp_dwpw_diag_log), 4, 0, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    const int words = 1 + 16 * (int)(n < 256u ? n : 256u);
    if (host && cap_words > 0 &&
        hipMemcpyFromSymbol(host, HIP_SYMBOL(lp_dwpw_diag_log), 4 * (size_t)(words < cap_words ? words : cap_words), 0,
                            hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
    if (clear) {
        const unsigned z = 0;
        if (hipMemcpyToSymbol(HIP_SYMBOL(lp_dwpw_diag_log), &z, 4, 0, hipMemcpyHostToDevice) != hipSuccess) return -1;
    }
    return (int)n;
#endif
}

bool launch_dwpw(const float* in, const float* wdw, const float* bdw, const float* wp, const float* bias,
                 const float* res, float* out, int N, int C, int H, int W, int K, int S, int Cout,
                 hipStream_t s, int diag) {
    // preconditions of the fused kernel; the caller falls back to dw + pw otherwise
    if ((K != 7 && K != 3) || (C & 31) || (W & 3) || Cout > 96) return false;
    if (K == 3 && (S != 1 || Cout > 32)) return false;        // the stem's dw3 + 1x1
    // measured on MI355X (profiles/r01_fused_dwpw.txt): with one workgroup per 16x16 tile the fused
    // form wins on >= 64x64 output planes; smaller planes do not fill the chip with tiles yet
    {
        const int OHt = (H + 2 * (K / 2) - K) / S + 1, OWt = (W + 2 * (K / 2) - K) / S + 1;
        if ((long)OHt * OWt < 4096) return false;
    }
    const int nb = (Cout + 31) / 32;
    if (K == 3) {
        launch_dwpw_t<3, 1, 1>(in, wdw, bdw, wp, bias, res, out, N, C, H, W, Cout, s, diag);
        return true;
    }
#define LP_F(SV, NBV) launch_dwpw_t<7, SV, NBV>(in, wdw, bdw, wp, bias, res, out, N, C, H, W, Cout, s)
    if (S == 1) { if (nb == 1) LP_F(1, 1); else if (nb == 2) LP_F(1, 2); else LP_F(1, 3); }
    else { if (nb == 1) LP_F(2, 1); else if (nb == 2) LP_F(2, 2); else LP_F(2, 3); }
#undef LP_F
    return true;
}


// =====================================================================================
// Fused output head (layers.py:120-133 SepConv2d x2, pose_mobilenet.py:150-153): per 16x16 tile of one image
//   out = Wr . relu(dw5(refined) + b_r) + Wx . relu(dw5(raw) + b_x)
// in ONE launch: the two depthwise results (Ca + Cb <= 64 channels) exist only in a 16-row ring of a [.][256] LDS slab, so HBM
// sees refined + raw in and the J / 2J maps out (452 MB instead of 1.12 GB per 128 images at 128x128).
//   phase 1  wave w runs the LDS-tiled 5x5 for channel PAIRS w, w+4, ... of the CONCATENATED sources: the two
//            halo tiles are interleaved per cell, so every tap of both channels is one v_pk_fma_f32 against an
//            SGPR weight pair ([C/2][26][2]: 25 taps + bias); next pair's tiles in flight under the FMAs
//   phase 2  wave w owns tile pixels [64w, 64w+64): D[NB*32 co][64 px] = W . slab on the fp32 matrix cores
//            (two-source A fragments of pack_pw), 8-byte stores
// DUAL = false (plain head, pose_simplenet.py:134-135):  out = Wr . relu(dw5(refined) + b_r)  -- one source, no raw operand.
// That form restates the unfused chain it replaces bit for bit: the depthwise sums its taps from ZERO in dw_pair_kernel's
// order (ky, kx) and adds the bias last, the 1x1 accumulates the k-pairs in ascending order from zero like pw2_kernel
// =====================================================================================
__device__ __forceinline__ int quad_row_of_lane(int lane) {
    // quad -> tile row such that the ds_read_b128 lane groups hold rows {a, a+1, a+8, a+9}: with a row stride of
    // 13 sixteen-byte slots their four strips (2 slots apart) land on 16 distinct slots (the table of mbconv_kernel)
    return (int)((0xFDCE5764B98A1320ull >> (4 * (lane >> 2))) & 15);
}

template <int NB, bool DUAL>
__global__ __launch_bounds__(256) void headfuse_kernel(const float* __restrict__ inA, int Ca,
                                                       const float* __restrict__ inB, int Cb,
                                                       const float* __restrict__ wpairA,   // [Ca/2][K*K + 1][2] taps, bias
                                                       const float* __restrict__ wpairB,   // [Cb/2][K*K + 1][2]
                                                       const float* __restrict__ wp,       // A frags [cblocks][C/2][64]
                                                       float* __restrict__ out, int H, int W, int tilesX, int tilesY,
                                                       int Cout, int xcd_remap) {
    constexpr int K = 5;                                  // both heads of every published network: SepConv2d(k5)
    constexpr int HALO = K / 2;
    constexpr int IH = 16 + K - 1;                        // input rows per tile
    constexpr int QPR = 6;                                // float4 staged per row and channel: columns -4 .. 19
    constexpr int RS = 13;                                // row stride in 16-byte slots (2 cells x 2 ch each; 12 used)
    constexpr int TILE_SLOTS = IH * RS;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int C = DUAL ? Ca + Cb : Ca;
    // Round 5: the slab is a RING of 16 channel rows: round u parks its 8 channels in rows 8 (u & 1) .. + 7, the next round's
    // MFMAs read them, and the round after that overwrites them behind the barrier in between -- 16 KB instead of C KB, so
    // the kernel's LDS footprint (33 KB) no longer caps it at two workgroups per CU
    float* slab = smem;                                   // [16][256]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    f32x4* tile = reinterpret_cast<f32x4*>(smem + 16 * 256) + wave * TILE_SLOTS;  // [IH][RS] slots = (cell, ch pair) x 2
    const int unit = xcd_remap ? xcd_contiguous_id(blockIdx.x, gridDim.x) : blockIdx.x;
    const int tq = unit / tilesX;
    const int tx = unit - tq * tilesX;
    const int n = tq / tilesY;
    const int ty = tq - n * tilesY;
    const int ix0 = tx * 16 - 4, iy0 = ty * 16 - HALO;
    constexpr int NQ = IH * QPR, NLD = (NQ + 63) / 64;
    const int row = quad_row_of_lane(lane), strip = lane & 3;
    const int half = lane >> 5, pl = lane & 31;
    const int KP = C >> 1;
    const int cblocks = (Cout + 31) >> 5;
    int st_off[NLD], st_lds[NLD];                         // per-lane staging coordinates, the same for every channel
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
        const int e = lane + 64 * i;
        const int r = e / QPR, q = e - r * QPR;
        const int iy = iy0 + r, ix = ix0 + 4 * q;
        const bool ok = e < NQ && iy >= 0 && iy < H && ix >= 0 && ix < W;
        st_off[i] = ok ? iy * W + ix : -1;
        st_lds[i] = e < NQ ? r * RS + 2 * q : -1;          // 4 cells = 2 slots
    }
    const long HW = (long)H * W;
    const float* imgA = inA + (long)n * Ca * HW;
    const float* imgB = DUAL ? inB + (long)n * Cb * HW : imgA;
    float afr[NB][32];                                     // the 1x1's A fragments (C <= 64 -> <= 32 k-pairs)
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int kp = 0; kp < 32; ++kp)
            afr[i][kp] = wp[((long)min(i, cblocks - 1) * KP + min(kp, KP - 1)) * 64 + lane];
    // The halo tiles are requested ONE channel pair ahead of the FMAs: with the ring slab four workgroups fit a CU (33 KB of
    // LDS, 88 + 34 registers), and sixteen resident waves hide the loads better than fewer waves with more in flight
    f32x4 pre[2][NLD];
    auto issue = [&](int cp) {                             // channel pair cp of the concatenated sources -> pre
        const int c = 2 * cp;
        const float* plane = (!DUAL || c < Ca) ? imgA + (long)c * HW : imgB + (long)(c - Ca) * HW;
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
            for (int i = 0; i < NLD; ++i) {
                f32x4 v = *reinterpret_cast<const f32x4*>(plane + h2 * HW + max(st_off[i], 0));
                if (st_off[i] < 0) v = f32x4{0.f, 0.f, 0.f, 0.f};
                pre[h2][i] = v;
            }
    };
    issue(wave);
    // Rounds: in round u wave w runs the depthwise of channel pair 4u + w and parks it in the slab; a workgroup barrier
    // later the four k-pairs of that round are complete for all 256 pixels.  Their 1x1 MFMAs are NOT issued as one
    // block at the end (a wave issues in order: 40 back-to-back 64-cycle MFMAs were a quarter of the kernel with the
    // packed-FMA pipe idle) but inside the NEXT round's depthwise, one k-pair after each of its first four filter rows.
    f32x16 acc[NB][2];
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int v = 0; v < 2; ++v)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][v][r] = 0.f;
    const float* bsrc = slab + half * 256 + wave * 64 + 2 * pl;
    auto kpair_mfma = [&](int kp) {                        // D[co][this wave's 64 px] += W[:, kp] . slab[kp]
        const f32x2 bv = *reinterpret_cast<const f32x2*>(bsrc + (kp & 7) * 512);
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(afr[i][kp], bv[0], acc[i][0], 0, 0, 0);
            acc[i][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(afr[i][kp], bv[1], acc[i][1], 0, 0, 0);
        }
    };
    const int NR = (KP + 3) >> 2;                          // rounds (<= 8)
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        if (u >= NR) break;                                // workgroup-uniform
        const int cp = wave + 4 * u;
        const bool has = cp < KP;                          // wave-uniform
        const int c = 2 * cp;
        f32x2 dacc[4];
        f32x2 dbias = {0.f, 0.f};
        const float* wc = wpairA;
        if (has) {
            // registers -> pair-interleaved tile: slot = (cell 2m: ch0, ch1 | cell 2m+1: ch0, ch1)
#pragma unroll
            for (int i = 0; i < NLD; ++i)
                if (st_lds[i] >= 0) {
                    const f32x4 a = pre[0][i], b = pre[1][i];
                    tile[st_lds[i]] = f32x4{a[0], b[0], a[1], b[1]};
                    tile[st_lds[i] + 1] = f32x4{a[2], b[2], a[3], b[3]};
                }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (cp + 4 < KP) issue(cp + 4);
            wc = (!DUAL || c < Ca) ? wpairA + (long)cp * (K * K + 1) * 2 : wpairB + (long)(cp - (Ca >> 1)) * (K * K + 1) * 2;
            dbias = f32x2{wc[2 * K * K], wc[2 * K * K + 1]};                                    // bias pair
#pragma unroll
            for (int i = 0; i < 4; ++i) dacc[i] = DUAL ? dbias : f32x2{0.f, 0.f};               // one source: bias last
        }
#pragma unroll
        for (int ky = 0; ky < K; ++ky) {
            if (has) {
                // lane's 4 outputs start at tile column 4 + 4*strip; taps reach columns 4*strip + 4 - HALO .. + 7 + HALO
                const f32x4* lr = tile + (row + ky) * RS + 2 * strip;
                f32x2 v[12];
#pragma unroll
                for (int q = 0; q < 6; ++q) {
                    const f32x4 tt = lr[q];
                    v[2 * q] = f32x2{tt[0], tt[1]};
                    v[2 * q + 1] = f32x2{tt[2], tt[3]};
                }
#pragma unroll
                for (int kx = 0; kx < K; ++kx) {
                    const f32x2 w2 = {wc[2 * (ky * K + kx)], wc[2 * (ky * K + kx) + 1]};
#pragma unroll
                    for (int i = 0; i < 4; ++i) dacc[i] = __builtin_elementwise_fma(v[(4 - HALO) + kx + i], w2, dacc[i]);
                }
            }
            if (u > 0 && ky < 4) {                         // the previous round's k-pair ky, under this row's FMAs
                const int kp = 4 * (u - 1) + ky;
                if (kp < KP) {
                    __builtin_amdgcn_sched_barrier(0);
                    kpair_mfma(kp);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        if (has) {
            f32x4 o0, o1;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                o0[i] = fmaxf(DUAL ? dacc[i][0] : dacc[i][0] + dbias[0], 0.f);
                o1[i] = fmaxf(DUAL ? dacc[i][1] : dacc[i][1] + dbias[1], 0.f);
            }
            *reinterpret_cast<f32x4*>(slab + (2 * (cp & 7)) * 256 + row * 16 + strip * 4) = o0;
            *reinterpret_cast<f32x4*>(slab + (2 * (cp & 7) + 1) * 256 + row * 16 + strip * 4) = o1;
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)                            // the last round's k-pairs (compile-time register indices)
        if (u == NR - 1) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * u + j < KP) kpair_mfma(4 * u + j);
        }
    const int p0 = wave * 64 + 2 * pl;
    const int oy = ty * 16 + (p0 >> 4), ox = tx * 16 + (p0 & 15);
    if (oy >= H || ox >= W) return;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        if (i >= cblocks) break;
        const int cob = i * 32 + 4 * half;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = cob + (r & 3) + 8 * (r >> 2);
            if (co < Cout)
                *reinterpret_cast<f32x2*>(out + ((long)n * Cout + co) * HW + (long)oy * W + ox) =
                    f32x2{acc[i][0][r], acc[i][1][r]};
        }
    }
}

bool launch_headfuse(const float* inA, int Ca, const float* inB, int Cb, const float* wpairA, const float* wpairB,
                     const float* wp, float* out, int N, int H, int W, int K, int Cout, hipStream_t s) {
    const int C = Ca + Cb;
    // the rule depends on the layer shape only (batched == per-image bitwise); small planes do not fill the
    // chip with one workgroup per 16x16 tile.  inB == nullptr: the one-source head (plain head, Cb = 0)
    const bool dual = inB != nullptr;
    if (!wpairA || (dual ? (!wpairB || (Cb & 1)) : Cb != 0) || K != 5 || (Ca & 1) || C > 64 || (W & 15) || (H & 15) ||
        Cout > 64 || (long)H * W < 4096)
        return false;
    const int tilesX = W / 16, tilesY = H / 16;
    const int grid = N * tilesX * tilesY;
    const size_t lds = (size_t)(16 * 256 + 4 * (16 + 5 - 1) * 13 * 4) * sizeof(float);
    static_assert((16 * 256 + 4 * (16 + 5 - 1) * 13 * 4) * sizeof(float) <= 64 * 1024,
                  "33 KB: below the default dynamic-LDS limit, no per-device attribute call needed (ADVICE r05)");
    last_kernel_tag = "headfuse_kernel";
#define LP_HF(NBV, DV) LP_LAUNCH((headfuse_kernel<NBV, DV>), dim3(grid), dim3(256), lds, s, inA, Ca, inB, Cb, \
                                 wpairA, wpairB, wp, out, H, W, tilesX, tilesY, Cout, xcd_remap_mode())
    if (dual) { if (Cout <= 32) LP_HF(1, true); else LP_HF(2, true); }
    else { if (Cout <= 32) LP_HF(1, false); else LP_HF(2, false); }
#undef LP_HF
    return true;
}

// =====================================================================================
// Whole InvBottleneck in ONE kernel (stride 1, 7x7, Cout <= 32): the 6x expanded tensor
// lives only in LDS and registers, so HBM sees  x (with a 3-px halo) in  ->  block output
// out: B_blk instead of B_op, a ~7x cut of the block's traffic.
//
// One workgroup (4 waves) owns a 16x16 output tile of one image and walks the expanded
// channels in chunks of 32:
//   expand   E[32 ch][22x22 halo cells] = relu6(W1 . x + b1) on the fp32 matrix cores; the x halo
//            tile of a wave's four 32-cell groups is loaded once per tile (registers) and re-used by
//            every chunk; the D fragment goes to LDS as 8-byte (channel pair) writes into the
//            pair-interleaved tile [16 pairs][22 rows][26 cells][2]; cells outside the image are
//            forced to 0 (the depthwise pads the EXPANDED tensor)
//   dw+proj  wave w takes channel pairs kp = w, w+4, .. of the chunk.  The LDS-tiled 7x7 runs BOTH
//            channels of a pair in one packed FMA per tap (pair-interleaved SGPR weights, 4 px / lane,
//            conflict-free quad->row table), then v_permlane32_swap turns the two 64-lane results into
//            the two MFMA B operands "[ch 2kp | ch 2kp+1] x 32 pixel columns" WITHOUT touching LDS,
//            and 8 MFMAs accumulate the 1x1 projection
//   reduce   the 4 waves hold K-slices of the projection: summed through the (now free) E
//            buffer so that every lane ends with 4 consecutive pixels -> 16-byte stores,
//            + bias (+ residual x)
// =====================================================================================
constexpr int MB_RS = 24, MB_ROWS = 22, MB_PLANE = MB_RS * MB_ROWS;       // 528 floats / channel

// pair-interleaved E tile of mbconv_kernel: 26 cells (13 sixteen-byte slots) per row
constexpr int MB2_RS = 26, MB2_PAIR = MB_ROWS * MB2_RS * 2;               // floats per channel pair

__device__ __forceinline__ int mb2_row_of_lane(int lane) {
    // quad -> tile row such that the ds_read_b128 lane groups hold rows {a, a+1, a+8, a+9}: with a row
    // stride of 13 slots their four strips land on 16 distinct slots (same table as dw_pair_kernel)
    return (int)((0xFDCE5764B98A1320ull >> (4 * (lane >> 2))) & 15);
}

template <bool RES>
__global__ __launch_bounds__(256, 2) void mbconv_kernel(
    const float* __restrict__ x,        // [N, Cin, H, W]
    const float* __restrict__ w1p,      // expand A frags [Cexp/32][Cin/2][64]
    const float* __restrict__ b1f,      // expand bias, D-frag order [Cexp/32][2][16]
    const float* __restrict__ wdwp,     // depthwise weights, channel-pair interleaved [Cexp/2][49][2]
    const float* __restrict__ bdw,      // [Cexp]
    const float* __restrict__ w2p,      // project A frags [1][Cexp/2][64]
    const float* __restrict__ b2f,      // project bias, D-frag order [2][16]
    float* __restrict__ out,            // [N, Cout, H, W]
    int Cin, int Cexp, int Cout, int H, int W, int tilesX, int tilesY, int xcd_remap) {
    // E tile, channel-pair interleaved: [16 pairs][22 rows][26 cells][2 channels]: a 16-byte slot is two
    // cells of both channels of a pair, every depthwise tap is one packed FMA for the pair (196 instead of
    // 2x126), the expand writes 8-byte pairs.  Row stride 13 slots + the quad->row table of the pair kernel
    // keep every ds_read_b128 lane group on 16 distinct slots.
    extern __shared__ __attribute__((aligned(16))) float E[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int half = lane >> 5, pl = lane & 31;
    const int unit = xcd_remap ? xcd_contiguous_id(blockIdx.x, gridDim.x) : blockIdx.x;
    const int tq = unit / tilesX;
    const int tx = unit - tq * tilesX;
    const int n = tq / tilesY;
    const int ty = tq - n * tilesY;
    const int x0 = tx * 16, y0 = ty * 16;
    const long HW = (long)H * W;
    const float* xin = x + (long)n * Cin * HW;
    const int nchunks = Cexp >> 5;

    // ---- expand geometry: this wave's halo-cell groups g = wave, wave+4, .. (17 groups) ----
    // the depthwise reads columns 1..22 of the 24-column halo tile (cells 0 and 23 only pad the 16-byte
    // reads), so the expand enumerates 22x22 = 484 cells: 16 groups of 32, exactly four per wave
    constexpr int NCOL = 22, CELLS = MB_ROWS * NCOL;
    constexpr int NG = (CELLS + 31) / 32;
    // ---- depthwise geometry --------------------------------------------------------------
    const int drow = mb2_row_of_lane(lane), strip = lane & 3;
    const float* e_lane = E + (drow * MB2_RS + strip * 4) * 2;   // + pair*MB2_PAIR + ky*MB2_RS*2

    f32x16 acc[2][4];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int v = 0; v < 4; ++v)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[h][v][r] = 0.f;

    // ---- the x halo tile of this wave's cell groups, loaded ONCE: every 32-channel chunk of the
    //      expand re-uses it (it used to be re-fetched per chunk: 3x the loads and their latency)
    constexpr int NGW = (NG + 3) / 4;                          // groups per wave (4)
    constexpr int KP1 = 12;                                    // input channel pairs: Cin = 24 (fp32 expand, 32x32x2 MFMAs)
    float xv[NGW][KP1];
    bool xok[NGW];
#pragma unroll
    for (int gi = 0; gi < NGW; ++gi) {
        const int g = wave + 4 * gi;
        const int hp0 = g * 32 + pl;
        const int hy = hp0 / NCOL, hx = 1 + hp0 - hy * NCOL;
        const int yy = y0 - 3 + hy, xx = x0 - 4 + hx;
        xok[gi] = g < NG && hp0 < CELLS && yy >= 0 && yy < H && xx >= 0 && xx < W;
        const float* sp = xin + (long)half * HW + (xok[gi] ? yy * W + xx : 0);
#pragma unroll
        for (int kp = 0; kp < KP1; ++kp) {
            const float t = sp[(long)(2 * kp) * HW];
            xv[gi][kp] = xok[gi] ? t : 0.f;
        }
    }

    for (int ch = 0; ch < nchunks; ++ch) {
        // ================= expand: E = relu6(W1[chunk] . x + b1) on the halo tile =========
        {
            float a1[KP1];
#pragma unroll
            for (int kp = 0; kp < KP1; ++kp) a1[kp] = w1p[((long)ch * KP1 + kp) * 64 + lane];
            const f32x4* bp = reinterpret_cast<const f32x4*>(b1f + ((long)ch * 2 + half) * 16);
            f32x4 b1v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) b1v[q] = bp[q];
#pragma unroll
            for (int gi = 0; gi < NGW; ++gi) {
                const int g = wave + 4 * gi;
                if (g >= NG) break;                                // wave-uniform
                f32x16 d;
#pragma unroll
                for (int r = 0; r < 16; ++r) d[r] = 0.f;
#pragma unroll
                for (int kp = 0; kp < KP1; ++kp) d = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[kp], xv[gi][kp], d, 0, 0, 0);
                const int hp = g * 32 + pl;
                if (hp < CELLS) {
                    const int hy = hp / NCOL, hx = 1 + hp - hy * NCOL;
                    float* ecell = E + (hy * MB2_RS + hx) * 2;
#pragma unroll
                    for (int r = 0; r < 16; r += 2) {                  // registers r, r+1 = channels cc, cc+1
                        const int cc = 4 * half + (r & 3) + 8 * (r >> 2);
                        const float v0 = fminf(fmaxf(d[r] + b1v[r >> 2][r & 3], 0.f), 6.f);
                        const float v1 = fminf(fmaxf(d[r + 1] + b1v[r >> 2][(r & 3) + 1], 0.f), 6.f);
                        const f32x2 pv = {xok[gi] ? v0 : 0.f, xok[gi] ? v1 : 0.f};
                        *reinterpret_cast<f32x2*>(ecell + (cc >> 1) * MB2_PAIR) = pv;
                    }
                }
            }
        }
        __syncthreads();
        // ================= depthwise pairs -> permlane swap -> project MFMAs ================
#pragma unroll 1
        for (int u = 0; u < 4; ++u) {
            const int kp = wave + 4 * u;                        // pair inside the chunk
            // project weights of this pair: requested now, consumed after ~250 packed FMAs (hipcc otherwise
            // sinks the load to just before the MFMAs and waits for it there)
            const float av = w2p[((long)(ch * 16 + kp)) * 64 + lane];
            __builtin_amdgcn_sched_barrier(0);
            float res2[2][4];
            {
                const int c = ch * 32 + 2 * kp;                    // first channel of the pair
                const f32x2* wc = reinterpret_cast<const f32x2*>(wdwp) + (long)(c >> 1) * 49;
                const float* ep = e_lane + kp * MB2_PAIR;
                f32x2 a4[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
                // the next row's six ds_read_b128 are issued before this row's 28 packed FMAs
                f32x4 rn[6], rc[6];
#pragma unroll
                for (int q = 0; q < 6; ++q) rn[q] = *reinterpret_cast<const f32x4*>(ep + 4 * q);
                keep_b128(rn[0]); keep_b128(rn[5]);                 // half-used outer slots stay ds_read_b128 (split3.h)
#pragma unroll
                for (int ky = 0; ky < 7; ++ky) {
#pragma unroll
                    for (int q = 0; q < 6; ++q) rc[q] = rn[q];
                    if (ky < 6) {
#pragma unroll
                        for (int q = 0; q < 6; ++q)
                            rn[q] = *reinterpret_cast<const f32x4*>(ep + (ky + 1) * (MB2_RS * 2) + 4 * q);
                        keep_b128(rn[0]); keep_b128(rn[5]);
                    }
                    f32x2 P[12];                                    // cells x-4 .. x+7: (ch a, ch b)
#pragma unroll
                    for (int q = 0; q < 6; ++q) {
                        P[2 * q] = f32x2{rc[q][0], rc[q][1]};
                        P[2 * q + 1] = f32x2{rc[q][2], rc[q][3]};
                    }
#pragma unroll
                    for (int kx = 0; kx < 7; ++kx) {
                        const f32x2 w2 = wc[ky * 7 + kx];           // wave-uniform: an SGPR pair
#pragma unroll
                        for (int i = 0; i < 4; ++i) a4[i] = __builtin_elementwise_fma(P[1 + kx + i], w2, a4[i]);
                    }
                }
                const float b0 = bdw[c], b1 = bdw[c + 1];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    res2[0][i] = fminf(fmaxf(a4[i][0] + b0, 0.f), 6.f);
                    res2[1][i] = fminf(fmaxf(a4[i][1] + b1, 0.f), 6.f);
                }
            }
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                // lanes 0-31 keep channel 2kp, lanes 32-63 receive channel 2kp+1 (and vice versa)
                const unsigned ua = __float_as_uint(res2[0][v]), ub = __float_as_uint(res2[1][v]);
                const auto sw = __builtin_amdgcn_permlane32_swap(ua, ub, false, false);
                const float lo = __uint_as_float(sw[0]);       // [ch a rows 0-7 | ch b rows 0-7]
                const float hi = __uint_as_float(sw[1]);       // [ch a rows 8-15 | ch b rows 8-15]
                acc[0][v] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, lo, acc[0][v], 0, 0, 0);
                acc[1][v] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, hi, acc[1][v], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // ================= cross-wave reduction of the K-slices + epilogue =======================
    // round h: every wave parks acc[h][0..3] in LDS; wave w then sums co-registers 4w..4w+3
    const f32x4* bp2 = reinterpret_cast<const f32x4*>(b2f + half * 16);
    const f32x4 b2v = bp2[wave];                                // regs 4w..4w+3 of this half
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int v = 0; v < 4; ++v)
#pragma unroll
            for (int r = 0; r < 16; ++r) E[((wave * 4 + v) * 16 + r) * 64 + lane] = acc[h][v][r];
        __syncthreads();
        // column j = lane&31 of round h is tile lane L = j + 32h
        const int L = pl + 32 * h;
        const int oy = y0 + mb2_row_of_lane(L), ox = x0 + (L & 3) * 4;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int r = 4 * wave + rr;
            const int co = 4 * half + (r & 3) + 8 * (r >> 2);
            f32x4 sum = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                float t = 0.f;
#pragma unroll
                for (int w = 0; w < 4; ++w) t += E[((w * 4 + v) * 16 + r) * 64 + lane];
                sum[v] = t + b2v[rr];
            }
            if (co < Cout && oy < H && ox < W) {
                const long o = ((long)n * Cout + co) * HW + (long)oy * W + ox;
                if (RES) {
                    const f32x4 rx = *reinterpret_cast<const f32x4*>(x + o);   // Cin == Cout
                    sum[0] += rx[0]; sum[1] += rx[1]; sum[2] += rx[2]; sum[3] += rx[3];
                }
                *reinterpret_cast<f32x4*>(out + o) = sum;
            }
        }
        __syncthreads();
    }
}

// -------------------------------------------------------------------------------------
// mbconv2_kernel: the same block with the depthwise -> project half rebuilt around the two things the first
// form is bound by (profiles/README.md: its LDS, matrix-core and VALU times ADD UP; LDS reads are the largest):
//   * a lane owns a 2 x 4 output block of a channel pair and the wave runs TWO pairs per pass (quad ->
//     (pair, row pair) table below): input rows are read once for two output rows, 48 instead of 84
//     ds_read_b128 per two pairs; pairs start an odd number of 16-byte slots apart, so the lane groups of a
//     ds_read_b128 (rows {g, g+4} of pair A and of pair B) land on 16 distinct slots
//   * the per-lane filter rows cannot be SGPR operands any more (two pairs per wave); they come through the
//     vector memory path (idle in this phase; L1-resident: 7 KB per chunk, same for every workgroup), two rows
//     ahead, as ONE stream across passes and chunks, so no pass starts by waiting for its first row
//   * project on v_mfma_f32_16x16x4_f32: v_permlane32_swap of (channel-0 results, channel-1 results) IS its B
//     operand -- rows k = (pair A ch0, pair B ch0, pair A ch1, pair B ch1) of the same 16 pixels -- so a 16-filter
//     block takes 16 MFMAs of 32 cycles per two pairs instead of 16 of 64 (the 32x32x2 form computed 32 output
//     channels whatever Cout is) and 64 accumulator registers instead of 128
// Expand and depthwise arithmetic are those of mbconv_kernel bit for bit; the project sums the same products
// in a different order (K = 4 per MFMA, other K-slices per wave).
// -------------------------------------------------------------------------------------
constexpr int MB3_PAIR = MB2_PAIR + 4;                                    // 287 slots: odd

__device__ __forceinline__ int mb3_rp_of_quad(int q) {
    // quad -> row pair: quads 0-3 / 8-11 = pair A, 4-7 / 12-15 = pair B, and quad q + 4 owns the pixels of quad q
    return (int)((0x6732673245104510ull >> (4 * q)) & 15);
}

template <bool RES>
__global__ __launch_bounds__(256, 2) void mbconv2_kernel(
    const float* __restrict__ x,        // [N, Cin, H, W]
    const f32x4* __restrict__ wrow,     // depthwise filter rows [Cexp/2][7][7 taps x 2 ch, bias pair in row 0's pad]
    const u32x4* __restrict__ w1s,      // expand weights as bf16x3 A fragments [Cexp/32][Cin/16][3][64]
    const float* __restrict__ b1f,      // expand bias, D-frag order [Cexp/32][2][16]
    const float* __restrict__ w2p,      // project weights, 32x32x2 A-fragment order [Cexp/2][64]
    const float* __restrict__ b2f,      // project bias, 32x32 D-frag order [2][16]
    float* __restrict__ out,            // [N, Cout, H, W]
    int Cin, int Cexp, int Cout, int H, int W, int tilesX, int tilesY, int xcd_remap) {
    extern __shared__ __attribute__((aligned(16))) float E[];   // [16 pairs][22 rows][26 cells][2 ch] (+4 per pair)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int half = lane >> 5, pl = lane & 31;
    const int unit = xcd_remap ? xcd_contiguous_id(blockIdx.x, gridDim.x) : blockIdx.x;
    const int tq = unit / tilesX;
    const int tx = unit - tq * tilesX;
    const int img = tq / tilesY;
    const int ty = tq - img * tilesY;
    const int x0 = tx * 16, y0 = ty * 16;
    const long HW = (long)H * W;
    const float* xin = x + (long)img * Cin * HW;
    const int nchunks = Cexp >> 5;

    constexpr int NCOL = 22, CELLS = MB_ROWS * NCOL;
    constexpr int NG = (CELLS + 31) / 32, NGW = (NG + 3) / 4;
    constexpr int KS1 = 1;                                       // k-steps of 16 input channels: Cin = 16
    constexpr int NBLK = 1;                                      // blocks of 16 filters: Cout <= 16
    // ---- depthwise geometry ------------------------------------------------------------------
    const int dwq = lane >> 2, strip = lane & 3;
    const int dwpair = (dwq >> 2) & 1;
    const int rp = mb3_rp_of_quad(dwq);
    const int dwoff = (2 * rp * MB2_RS + strip * 4) * 2;         // first cell this lane reads (input row R = 0)

    f32x4 acc[NBLK][16];                                         // [(r*2 + S)*4 + i]: 16 filters x 16 pixels each
#pragma unroll
    for (int b = 0; b < NBLK; ++b)
#pragma unroll
        for (int c = 0; c < 16; ++c) acc[b][c] = f32x4{0.f, 0.f, 0.f, 0.f};

    // ---- the x halo tile of this wave's cell groups as bf16x3 B fragments, split ONCE per tile ----
    u32x4 xh[NGW][KS1], xm[NGW][KS1], xl[NGW][KS1];
    bool xok[NGW];
#pragma unroll
    for (int gi = 0; gi < NGW; ++gi) {
        const int g = wave + 4 * gi;
        const int hp0 = g * 32 + pl;
        const int hy = hp0 / NCOL, hx = 1 + hp0 - hy * NCOL;
        const int yy = y0 - 3 + hy, xx = x0 - 4 + hx;
        xok[gi] = g < NG && hp0 < CELLS && yy >= 0 && yy < H && xx >= 0 && xx < W;
        const float* sp = xin + (long)(8 * half) * HW + (xok[gi] ? yy * W + xx : 0);
#pragma unroll
        for (int ks = 0; ks < KS1; ++ks) {
            float v[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const float t = sp[(long)(16 * ks + c) * HW];
                v[c] = xok[gi] ? t : 0.f;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const Split3 p3 = split3_pair(v[2 * j], v[2 * j + 1]);
                xh[gi][ks][j] = p3.h; xm[gi][ks][j] = p3.m; xl[gi][ks][j] = p3.l;
            }
        }
    }

    // ---- filter rows: one stream over (chunk, pass, row), two rows ahead of their use --------------
    auto rows_of = [&](int ch, int u) {
        return wrow + ((long)(ch * 16 + 2 * (wave + 4 * u) + dwpair) * 7) * 4;
    };
    f32x4 wa[4], wn[4];
    {
        const f32x4* w0 = rows_of(0, 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) { wa[q] = w0[q]; wn[q] = w0[4 + q]; }
    }
    const int kperm = ((lane >> 4) & 1) * 2 + (lane >> 5);       // MFMA k row -> channel of the four: 0, 2, 1, 3

    for (int ch = 0; ch < nchunks; ++ch) {
        // ================= expand: E = relu6(W1[chunk] . x + b1) on the halo tile =========
        {
            u32x4 a3[KS1][3];
#pragma unroll
            for (int ks = 0; ks < KS1; ++ks)
#pragma unroll
                for (int t = 0; t < 3; ++t) a3[ks][t] = w1s[(((long)ch * KS1 + ks) * 3 + t) * 64 + lane];
            const f32x4* bp = reinterpret_cast<const f32x4*>(b1f + ((long)ch * 2 + half) * 16);
            f32x4 b1v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) b1v[q] = bp[q];
#pragma unroll
            for (int gi = 0; gi < NGW; ++gi) {
                const int g = wave + 4 * gi;
                if (g >= NG) break;                                // wave-uniform
                f32x16 d;
#pragma unroll
                for (int r = 0; r < 16; ++r) d[r] = 0.f;
#pragma unroll
                for (int ks = 0; ks < KS1; ++ks) d = mma6(a3[ks], xh[gi][ks], xm[gi][ks], xl[gi][ks], d);
                const int hp = g * 32 + pl;
                if (hp < CELLS) {
                    const int hy = hp / NCOL, hx = 1 + hp - hy * NCOL;
                    float* ecell = E + (hy * MB2_RS + hx) * 2;
#pragma unroll
                    for (int r = 0; r < 16; r += 2) {                  // registers r, r+1 = channels cc, cc+1
                        const int cc = 4 * half + (r & 3) + 8 * (r >> 2);
                        const float v0 = fminf(fmaxf(d[r] + b1v[r >> 2][r & 3], 0.f), 6.f);
                        const float v1 = fminf(fmaxf(d[r + 1] + b1v[r >> 2][(r & 3) + 1], 0.f), 6.f);
                        const f32x2 pv = {xok[gi] ? v0 : 0.f, xok[gi] ? v1 : 0.f};
                        *reinterpret_cast<f32x2*>(ecell + (cc >> 1) * MB3_PAIR) = pv;
                    }
                }
            }
        }
        __syncthreads();
        // ================= depthwise of two pairs per pass -> permlane swap -> project MFMAs ===========
#pragma unroll 1
        for (int u = 0; u < 2; ++u) {
            const int kpA = 2 * (wave + 4 * u);                    // pairs kpA (lanes of pair A), kpA + 1 (pair B)
            // filter rows that follow this pass in the stream
            const int un = u ^ 1, chn = u ? min(ch + 1, nchunks - 1) : ch;
            const f32x4* wnext = rows_of(chn, un);
            const f32x4* wcur = rows_of(ch, u);
            // project A operands: filter 16 blk + (lane & 15), channel 32 ch + 2 kpA + kperm
            float av[NBLK];
            {
                const int c = ch * 32 + 2 * kpA + kperm;
#pragma unroll
                for (int b = 0; b < NBLK; ++b) av[b] = w2p[(long)(c >> 1) * 64 + (c & 1) * 32 + 16 * b + (lane & 15)];
            }
            const float* ep = E + (kpA + dwpair) * MB3_PAIR + dwoff;
            f32x2 a0[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};   // output row 2rp
            f32x2 a1[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};   // output row 2rp + 1
            f32x4 rn[6], rc[6], wb[4];
#pragma unroll
            for (int q = 0; q < 6; ++q) rn[q] = *reinterpret_cast<const f32x4*>(ep + 4 * q);
            const float b0 = wa[3][2], b1 = wa[3][3];              // the pair's bias rides in row 0's pad
#pragma unroll
            for (int R = 0; R < 8; ++R) {                          // tile row 2rp + R
#pragma unroll
                for (int q = 0; q < 6; ++q) rc[q] = rn[q];
                // half-used outer slots stay ds_read_b128 (split3.h); the asm needs the data, so it sits where the
                // row is USED, and the requests of the next row are pinned between it and this row's FMAs (dw7.h)
                keep_b128(rc[0]); keep_b128(rc[5]);
                __builtin_amdgcn_sched_barrier(0);
                if (R < 7) {
#pragma unroll
                    for (int q = 0; q < 6; ++q)
                        rn[q] = *reinterpret_cast<const f32x4*>(ep + (R + 1) * (MB2_RS * 2) + 4 * q);
                }
                __builtin_amdgcn_sched_barrier(0);
                f32x2 P[12];                                       // cells x-4 .. x+7: (ch a, ch b)
#pragma unroll
                for (int q = 0; q < 6; ++q) {
                    P[2 * q] = f32x2{rc[q][0], rc[q][1]};
                    P[2 * q + 1] = f32x2{rc[q][2], rc[q][3]};
                }
                if (R >= 1) {                                      // output row 1, filter row R-1 (= wb)
#pragma unroll
                    for (int kx = 0; kx < 7; ++kx) {
                        const f32x2 w2 = {wb[kx >> 1][2 * (kx & 1)], wb[kx >> 1][2 * (kx & 1) + 1]};
#pragma unroll
                        for (int i = 0; i < 4; ++i) a1[i] = __builtin_elementwise_fma(P[1 + kx + i], w2, a1[i]);
                    }
                }
                if (R <= 6) {                                      // output row 0, filter row R (= wa)
#pragma unroll
                    for (int kx = 0; kx < 7; ++kx) {
                        const f32x2 w2 = {wa[kx >> 1][2 * (kx & 1)], wa[kx >> 1][2 * (kx & 1) + 1]};
#pragma unroll
                        for (int i = 0; i < 4; ++i) a0[i] = __builtin_elementwise_fma(P[1 + kx + i], w2, a0[i]);
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q) { wb[q] = wa[q]; wa[q] = wn[q]; }
                    // stream position R + 2: rows 2..6 of this pass, then rows 0, 1 of the next one
                    const f32x4* src = R + 2 <= 6 ? wcur + (R + 2) * 4 : wnext + (R + 2 - 7) * 4;
#pragma unroll
                    for (int q = 0; q < 4; ++q) wn[q] = src[q];
                }
            }
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const f32x2 a = r ? a1[i] : a0[i];
                    const unsigned ua = __float_as_uint(fminf(fmaxf(a[0] + b0, 0.f), 6.f));
                    const unsigned ub = __float_as_uint(fminf(fmaxf(a[1] + b1, 0.f), 6.f));
                    // rows of 16 lanes: ua = (A ch0 | B ch0 | A ch0' | B ch0'), ub the same for channel 1 ->
                    // sw[0] = (A ch0 | B ch0 | A ch1 | B ch1) of pixel set S = 0, sw[1] of pixel set S = 1
                    const auto sw = __builtin_amdgcn_permlane32_swap(ua, ub, false, false);
                    const float s0 = __uint_as_float(sw[0]), s1 = __uint_as_float(sw[1]);
#pragma unroll
                    for (int b = 0; b < NBLK; ++b) {
                        acc[b][(r * 2 + 0) * 4 + i] =
                            __builtin_amdgcn_mfma_f32_16x16x4f32(av[b], s0, acc[b][(r * 2 + 0) * 4 + i], 0, 0, 0);
                        acc[b][(r * 2 + 1) * 4 + i] =
                            __builtin_amdgcn_mfma_f32_16x16x4f32(av[b], s1, acc[b][(r * 2 + 1) * 4 + i], 0, 0, 0);
                    }
                }
        }
        __syncthreads();
    }
    // ================= cross-wave reduction of the K-slices + epilogue =======================
    // every wave parks its 16 accumulator tiles of a filter block in LDS; wave w = 2r + S then sums the four
    // tiles (r, S, i = 0..3): a lane ends with 4 consecutive pixels of 4 filters -> 16-byte stores
    const int er = wave >> 1, eS = wave & 1, en = lane & 15;
    const int oy = y0 + 2 * mb3_rp_of_quad(8 * eS + (en >> 2)) + er, ox = x0 + 4 * (en & 3);
#pragma unroll
    for (int b = 0; b < NBLK; ++b) {
#pragma unroll
        for (int c = 0; c < 16; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j) E[((wave * 16 + c) * 4 + j) * 64 + lane] = acc[b][c][j];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int co = 16 * b + 4 * (lane >> 4) + j;
            const float bias = b2f[((co >> 2) & 1) * 16 + (co & 3) + 4 * (co >> 3)];
            f32x4 sum;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = (er * 2 + eS) * 4 + i;
                float t = 0.f;
#pragma unroll
                for (int w = 0; w < 4; ++w) t += E[((w * 16 + c) * 4 + j) * 64 + lane];
                sum[i] = t + bias;
            }
            if (co < Cout && oy < H && ox < W) {
                const long o = ((long)img * Cout + co) * HW + (long)oy * W + ox;
                if (RES) {
                    const f32x4 rx = *reinterpret_cast<const f32x4*>(x + o);   // Cin == Cout
                    sum[0] += rx[0]; sum[1] += rx[1]; sum[2] += rx[2]; sum[3] += rx[3];
                }
                *reinterpret_cast<f32x4*>(out + o) = sum;
            }
        }
        if (b + 1 < NBLK) __syncthreads();
    }
}

// -------------------------------------------------------------------------------------
// Stride-2 form of the fused block (the first block of a stage: no residual).  An 8x8 OUTPUT tile
// needs input rows 2*oy0-3 .. 2*oy0+17 and columns 2*ox0-4 .. 2*ox0+19: exactly the 22x24 halo tile of
// the stride-1 kernel, so the expand phase and the E layout are shared verbatim.  The depthwise
// takes ONE output per lane (lane = 8*row + col; taps at tile cell (2*row + ky, 2*col + 1 + kx), four
// ds_read_b64 per row, conflict-free at stride 24), v_permlane32_swap turns a channel pair into the
// B operands of the two 32-pixel halves, and the four waves' K-slices are summed through LDS.
// The 6x expanded tensor of the block (the largest tensor of the network) never leaves the CU.
// -------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void mbconv_s2_kernel(
    const float* __restrict__ x,        // [N, Cin, H, W]
    const void*, const void*,           // two unused slots, always null: this kernel keeps more scalars live than there are
                                        // SGPRs, and where its other arguments sit in the kernarg segment decides how their
                                        // loads merge and which scalars spill to VGPR lanes -- without the slots the same
                                        // vector work comes with six more lane moves
    const float* __restrict__ w1p,      // expand A frags [Cexp/32][Cin/2][64]
    const float* __restrict__ b1f,      // expand bias, D-frag order [Cexp/32][2][16]
    const float* __restrict__ wdwp,     // depthwise weights, channel-pair interleaved [Cexp/2][49][2]
    const float* __restrict__ bdw,      // [Cexp]
    const float* __restrict__ w2p,      // project A frags [1][Cexp/2][64]
    const float* __restrict__ b2f,      // project bias, D-frag order [2][16]
    float* __restrict__ out,            // [N, Cout, OH, OW]
    int Cin, int Cexp, int Cout, int H, int W, int OH, int OW, int tilesX, int tilesY, int xcd_remap) {
    // E tile, channel-pair interleaved: [16 pairs][528 cells][2 channels] -- a 16-byte read is two cells
    // of both channels of a pair, so every depthwise tap is one packed FMA for the pair
    extern __shared__ __attribute__((aligned(16))) float E[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int half = lane >> 5, pl = lane & 31;
    const int unit = xcd_remap ? xcd_contiguous_id(blockIdx.x, gridDim.x) : blockIdx.x;
    const int tq = unit / tilesX;
    const int tx = unit - tq * tilesX;
    const int n = tq / tilesY;
    const int ty = tq - n * tilesY;
    const int ox0 = tx * 8, oy0 = ty * 8;
    const int x0 = 2 * ox0, y0 = 2 * oy0;                      // tile origin at the input resolution
    const long HW = (long)H * W;
    const float* xin = x + (long)n * Cin * HW;
    const int nchunks = Cexp >> 5;
    // an 8x8 stride-2 tile reads rows 0..20 and columns 1..21 of the halo tile: the expand enumerates just
    // those 441 cells (14 groups of 32; the stride-1 kernel's full 528 would be 17)
    constexpr int NROW = 21, NCOL = 21, CELLS = NROW * NCOL;
    constexpr int NG = (CELLS + 31) / 32;
    constexpr int NGW = (NG + 3) / 4;                          // groups per wave (4)
    const int orow = lane >> 3, ocol = lane & 7;               // this lane's output inside the tile
    const float* e_lane = E + ((2 * orow) * MB_RS + 2 * ocol) * 2;   // + pair*1056 + ky*48; taps at cells 1..7

    f32x16 acc[2];                                             // pixels 0-31 / 32-63 of the tile
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[h][r] = 0.f;

    // the x halo tile of this wave's cell groups, loaded once for all expand chunks
    constexpr int KP1 = 12;                                    // input channel pairs: Cin = 24 (fp32 expand, 32x32x2 MFMAs)
    float xv[NGW][KP1];
    bool xok[NGW];
#pragma unroll
    for (int gi = 0; gi < NGW; ++gi) {
        const int g = wave + 4 * gi;
        const int hp0 = g * 32 + pl;
        const int hy = hp0 / NCOL, hx = 1 + hp0 - hy * NCOL;
        const int yy = y0 - 3 + hy, xx = x0 - 4 + hx;
        xok[gi] = g < NG && hp0 < CELLS && yy >= 0 && yy < H && xx >= 0 && xx < W;
        const float* sp = xin + (long)half * HW + (xok[gi] ? yy * W + xx : 0);
#pragma unroll
        for (int kp = 0; kp < KP1; ++kp) {
            const float t = sp[(long)(2 * kp) * HW];
            xv[gi][kp] = xok[gi] ? t : 0.f;
        }
    }

    for (int ch = 0; ch < nchunks; ++ch) {
        // ================= expand: E = relu6(W1[chunk] . x + b1) on the halo tile =========
        {
            float a1[KP1];
#pragma unroll
            for (int kp = 0; kp < KP1; ++kp) a1[kp] = w1p[((long)ch * KP1 + kp) * 64 + lane];
            const f32x4* bp = reinterpret_cast<const f32x4*>(b1f + ((long)ch * 2 + half) * 16);
            f32x4 b1v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) b1v[q] = bp[q];
#pragma unroll
            for (int gi = 0; gi < NGW; ++gi) {
                const int g = wave + 4 * gi;
                if (g >= NG) break;                                // wave-uniform
                f32x16 d;
#pragma unroll
                for (int r = 0; r < 16; ++r) d[r] = 0.f;
#pragma unroll
                for (int kp = 0; kp < KP1; ++kp) d = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[kp], xv[gi][kp], d, 0, 0, 0);
                const int hp = g * 32 + pl;
                if (hp < CELLS) {
                    const int hy = hp / NCOL, hx = 1 + hp - hy * NCOL;
                    float* ecell = E + (hy * MB_RS + hx) * 2;
#pragma unroll
                    for (int r = 0; r < 16; r += 2) {                  // registers r, r+1 = channels cc, cc+1
                        const int cc = 4 * half + (r & 3) + 8 * (r >> 2);
                        const float v0 = fminf(fmaxf(d[r] + b1v[r >> 2][r & 3], 0.f), 6.f);
                        const float v1 = fminf(fmaxf(d[r + 1] + b1v[r >> 2][(r & 3) + 1], 0.f), 6.f);
                        const f32x2 pv = {xok[gi] ? v0 : 0.f, xok[gi] ? v1 : 0.f};
                        *reinterpret_cast<f32x2*>(ecell + (cc >> 1) * (2 * MB_PLANE)) = pv;
                    }
                }
            }
        }
        __syncthreads();
        // ================= stride-2 depthwise pairs -> permlane swap -> project MFMAs =========
        // A wave issues in order, so the two 64-cycle project MFMAs of pair u-1 are placed INSIDE the depthwise of
        // pair u (after filter rows 2 and 5, pinned by sched_barrier): the matrix pipe works under the packed FMAs
        // instead of parking the wave at the end of every pair; the last pair of a chunk pays the tail.
        float pav = 0.f, plo = 0.f, phi = 0.f;
        auto dw_pair = [&](int u, auto PENDING) {
            constexpr bool pending = decltype(PENDING)::value;
            const int kp = wave + 4 * u;                        // pair inside the chunk
            const float av = w2p[((long)(ch * 16 + kp)) * 64 + lane];
            __builtin_amdgcn_sched_barrier(0);
            float res2[2];
            {
                const int c = ch * 32 + 2 * kp;                    // first channel of the pair
                const f32x2* wc = reinterpret_cast<const f32x2*>(wdwp) + (long)(c >> 1) * 49;
                const float* ep = e_lane + kp * (2 * MB_PLANE);
                f32x2 a = {0.f, 0.f};
#pragma unroll
                for (int ky = 0; ky < 7; ++ky) {
                    f32x2 P[8];                                     // cells 0..7 of the row: (ch a, ch b)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        f32x4 t = *reinterpret_cast<const f32x4*>(ep + ky * (2 * MB_RS) + 4 * q);
                        keep_b128(t);                               // a half-used slot stays ds_read_b128 (split3.h)
                        P[2 * q] = f32x2{t[0], t[1]};
                        P[2 * q + 1] = f32x2{t[2], t[3]};
                    }
#pragma unroll
                    for (int kx = 0; kx < 7; ++kx) a = __builtin_elementwise_fma(P[1 + kx], wc[ky * 7 + kx], a);   // SGPR pair
                    if constexpr (pending) {
                        if (ky == 2) {
                            __builtin_amdgcn_sched_barrier(0);
                            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(pav, plo, acc[0], 0, 0, 0);   // px 0-31
                            __builtin_amdgcn_sched_barrier(0);
                        }
                        if (ky == 5) {
                            __builtin_amdgcn_sched_barrier(0);
                            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(pav, phi, acc[1], 0, 0, 0);   // px 32-63
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    }
                }
                res2[0] = fminf(fmaxf(a[0] + bdw[c], 0.f), 6.f);
                res2[1] = fminf(fmaxf(a[1] + bdw[c + 1], 0.f), 6.f);
            }
            // lanes 0-31 keep channel 2kp, lanes 32-63 receive channel 2kp+1 (and vice versa)
            const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(res2[0]), __float_as_uint(res2[1]),
                                                             false, false);
            pav = av;
            plo = __uint_as_float(sw[0]);
            phi = __uint_as_float(sw[1]);
        };
        dw_pair(0, std::false_type());
#pragma unroll 1
        for (int u = 1; u < 4; ++u) dw_pair(u, std::true_type());
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(pav, plo, acc[0], 0, 0, 0);   // the last pair's products
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(pav, phi, acc[1], 0, 0, 0);
        __syncthreads();
    }
    // ================= cross-wave reduction of the K-slices + epilogue =======================
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int r = 0; r < 16; ++r) E[((wave * 2 + h) * 16 + r) * 64 + lane] = acc[h][r];
    __syncthreads();
    const f32x4* bp2 = reinterpret_cast<const f32x4*>(b2f + half * 16);
    const f32x4 b2v = bp2[wave];                                // regs 4w..4w+3 of this half
    const long OHW = (long)OH * OW;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int px = h * 32 + pl;                             // D column = tile pixel
        const int oy = oy0 + (px >> 3), ox = ox0 + (px & 7);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int r = 4 * wave + rr;
            const int co = 4 * half + (r & 3) + 8 * (r >> 2);
            float t = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) t += E[((w * 2 + h) * 16 + r) * 64 + lane];
            if (co < Cout && oy < OH && ox < OW) out[((long)n * Cout + co) * OHW + (long)oy * OW + ox] = t + b2v[rr];
        }
    }
}

// The three first-generation fused-block kernels serve the blocks no later kernel covers:
//   mbconv2_kernel<RES>    16-channel stride-1 blocks of up to 16 filters (stage 1 of XS / S), bf16x3 expand
//   mbconv_kernel<RES>     24-channel stride-1 blocks of up to 32 filters (stage 1 of M / L: Cin % 16 != 0, fp32 expand)
//   mbconv_s2_kernel       the stride-2 entry block of those
// Every other block shape runs in mbt_kernel / mbt_s2_kernel / mb16_kernel or as the unfused chain.
static bool launch_mbconv_s2(const float* x, const float* w1p, const float* b1f, const float* wdwp, const float* bdw,
                             const float* w2p, const float* b2f, float* out, int N, int Cin, int Cexp, int Cout, int H,
                             int W, hipStream_t s) {
    if (!wdwp || Cout > 32 || Cin != 24 || (Cexp & 31) || (H & 1) || (W & 1)) return false;
    const int OH = H / 2, OW = W / 2;
    if ((long)OH * OW < 1024) return false;
    const int tilesX = (OW + 7) / 8, tilesY = (OH + 7) / 8;
    const size_t lds = (size_t)(32 * MB_PLANE) * sizeof(float);
    dim3 grid(N * tilesX * tilesY), block(256);
    last_kernel_tag = "mbconv_s2_kernel";
    if (!kernel_ready(reinterpret_cast<const void*>(mbconv_s2_kernel), lds)) return false;
    LP_LAUNCH(mbconv_s2_kernel, grid, block, lds, s, x, (const void*)nullptr, (const void*)nullptr, w1p, b1f, wdwp, bdw,
              w2p, b2f, out, Cin, Cexp, Cout, H, W, OH, OW, tilesX, tilesY, xcd_remap_mode());
    return true;
}

bool launch_mbconv(const float* x, const float* w1p, const float* b1f, const float* wdw,
                   const float* bdw, const float* w2p, const float* b2f, const float* res, float* out,
                   int N, int Cin, int Cexp, int Cout, int H, int W, int K, int S, hipStream_t s,
                   const float* wdw_pair, const void* w1s, const void* wrow, int mbconv2) {
    if (K == 7 && S == 2 && !res)
        return launch_mbconv_s2(x, w1p, b1f, wdw_pair, bdw, w2p, b2f, out, N, Cin, Cexp, Cout, H, W, s);
    if (K != 7 || S != 1 || Cout > 32 || (Cin != 16 && Cin != 24) || (Cexp & 31) || (W & 3)) return false;
    if (res && res != x) return false;
    // measured (profiles/README.md): 0.17 vs 0.22 ms per block on 64x64 planes, 0.116 vs 0.125 ms on
    // 32x32 ones at 128 images (bench 5.64 -> 5.57 ms/step); 16x16 planes have Cin > 32
    if ((long)H * W < 1024 || !wdw_pair) return false;
    const int tilesX = (W + 15) / 16, tilesY = (H + 15) / 16;
    dim3 grid(N * tilesX * tilesY), block(256);
    if (Cin == 16) {
        // mbconv2_kernel (2 x 4 depthwise blocks, 16x16x4 project); option "mbconv2" = 0 -> the unfused chain
        if (!mbconv2 || !wrow || !w1s || Cout > 16) return false;
        const size_t lds2 = (size_t)16 * MB3_PAIR * sizeof(float);
        last_kernel_tag = "mbconv2_kernel";
        const auto kern = res ? mbconv2_kernel<true> : mbconv2_kernel<false>;
        if (!kernel_ready(reinterpret_cast<const void*>(kern), lds2)) return false;
        LP_LAUNCH(kern, grid, block, lds2, s, x, (const f32x4*)wrow, (const u32x4*)w1s, b1f, w2p, b2f, out, Cin, Cexp,
                  Cout, H, W, tilesX, tilesY, xcd_remap_mode());
        return true;
    }
    const size_t lds = (size_t)(16 * MB2_PAIR) * sizeof(float);
    last_kernel_tag = "mbconv_kernel";
    const auto kern = res ? mbconv_kernel<true> : mbconv_kernel<false>;
    if (!kernel_ready(reinterpret_cast<const void*>(kern), lds)) return false;
    LP_LAUNCH(kern, grid, block, lds, s, x, w1p, b1f, wdw_pair, bdw, w2p, b2f, out, Cin, Cexp, Cout, H, W, tilesX, tilesY,
              xcd_remap_mode());
    return true;
}

// =====================================================================================
// Fusion Deconv Head step: ConvT(refined) + ConvT(raw), k4 s2 p1, summed, + folded BN,
// ReLU (pose_mobilenet.py:147-149).  Sub-pixel form: each lane owns one INPUT grid cell
// (iy, ix) and produces the 2x2 output quad (2iy+a, 2ix+b); per input channel it reads
// the 3x3 input neighbourhood once and applies the 16 taps as wave-uniform scalars:
//   a=0: (dy= 0,ky=1) (dy=-1,ky=3)      a=1: (dy=+1,ky=0) (dy= 0,ky=2)   (same in x)
// =====================================================================================
// DUAL = false (plain head, pose_simplenet.py:133): ConvT(refined) alone -- the raw operand is absent at compile time
constexpr int COT = 8;                                    // output channels per workgroup row (grid.y) of deconv_pair_kernel
template <bool DUAL>
__global__ __launch_bounds__(256) void deconv_pair_kernel(const float* __restrict__ inA, int Ca,
                                                          const float* __restrict__ inB, int Cb,
                                                          const float* __restrict__ w,
                                                          const float* __restrict__ b,
                                                          float* __restrict__ out, int N, int h,
                                                          int w_, int Cout) {
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

    for (int src = 0; src < (DUAL ? 2 : 1); ++src) {
        const float* in = src == 0 ? inA : inB;
        const int Cs = src == 0 ? Ca : Cb;
        const int cbase = src == 0 ? 0 : Ca;
        for (int ci = 0; ci < Cs; ++ci) {
            const float* plane = in + ((long)n * Cs + ci) * h * w_;
            float v[3][3];
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    const int y = iy + dy, x = ix + dx;
                    v[dy + 1][dx + 1] =
                        (y >= 0 && y < h && x >= 0 && x < w_) ? plane[(long)y * w_ + x] : 0.f;
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
                            // taps for output parity (a, bb)
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
            const float bias = b[co];
            float* o = out + ((long)n * Cout + co) * OH * OW + (long)(2 * iy) * OW + 2 * ix;
            float2 r0 = {fmaxf(acc[c][0] + bias, 0.f), fmaxf(acc[c][1] + bias, 0.f)};
            float2 r1 = {fmaxf(acc[c][2] + bias, 0.f), fmaxf(acc[c][3] + bias, 0.f)};
            *reinterpret_cast<float2*>(o) = r0;
            *reinterpret_cast<float2*>(o + OW) = r1;
        }
    }
}

// -------------------------------------------------------------------------------------
// MFMA form of the same step (used whenever Cout <= 32, i.e. every published arch up to
// deconv_setting 32; wider layers fall back to the VALU kernel above).  Per output parity
// (a, b) the transposed conv is a 1x1 conv over K = 4 taps x (Ca + Cb) channels of SHIFTED
// input views:  out[co][2iy+a][2ix+b] = sum_{t, ci} Wd[a,b][co][t, ci] * X[ci][iy+dy_t][ix+dx_t]
// so it runs on the pw structure: A fragments packed per parity on the host, B fragment =
// 32 consecutive input cells of channel 2kp+half read at a per-lane tap offset (zero outside
// the image).  blockIdx.y = parity.  DUAL = false: the refined source only (plain head).
// -------------------------------------------------------------------------------------
template <bool DUAL>
__global__ __launch_bounds__(256) void deconv_mfma_kernel(const float* __restrict__ inA, int Ca,
                                                          const float* __restrict__ inB, int Cb,
                                                          const float* __restrict__ wp,   // [4][KP][64]
                                                          const float* __restrict__ bias, // D-frag order
                                                          float* __restrict__ out, long NP, int h, int w_,
                                                          int Cout) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const long px0 = ((long)blockIdx.x * 4 + wave) * 32;
    if (px0 >= NP) return;
    const int half = lane >> 5, pl = lane & 31;
    const long g = px0 + pl;
    const bool valid = g < NP;
    const long gc = valid ? g : NP - 1;
    const int hw = h * w_;
    const int n = (int)(gc / hw);
    const int p = (int)(gc - (long)n * hw);
    const int iy = p / w_, ix = p - iy * w_;
    const int par = blockIdx.y, a = par >> 1, b = par & 1;
    // pack_deconv: per tap the k-pairs of each source, an odd source padded to a whole pair
    const int KP = 4 * (((Ca + 1) >> 1) + (DUAL ? (Cb + 1) >> 1 : 0));
    // taps: a=0: (dy 0, ky 1), (dy -1, ky 3);  a=1: (dy +1, ky 0), (dy 0, ky 2)   (same in x)
    int toff[4];
    bool tok[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int tyi = t >> 1, txi = t & 1;
        const int dy = a == 0 ? (tyi == 0 ? 0 : -1) : (tyi == 0 ? 1 : 0);
        const int dx = b == 0 ? (txi == 0 ? 0 : -1) : (txi == 0 ? 1 : 0);
        const int y = iy + dy, x = ix + dx;
        tok[t] = y >= 0 && y < h && x >= 0 && x < w_;
        toff[t] = tok[t] ? y * w_ + x : p;
    }
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const f32x4* bp = reinterpret_cast<const f32x4*>(bias + half * 16);
    f32x4 bfr[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) bfr[q] = bp[q];
    const float* wl = wp + (long)par * KP * 64 + lane;
    int kbase = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll 1
        for (int srcsel = 0; srcsel < (DUAL ? 2 : 1); ++srcsel) {
            const int C = srcsel == 0 ? Ca : Cb;
            const float* sp = (srcsel == 0 ? inA : inB) + ((long)n * C + half) * hw + toff[t];
            const int nkp = C >> 1;
#pragma unroll 8
            for (int kp = 0; kp < nkp; ++kp) {
                float bv = sp[(long)(2 * kp) * hw];
                bv = tok[t] ? bv : 0.f;
                const float av = wl[(long)(kbase + kp) * 64];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
            }
            if (C & 1) {                                     // the last channel alone; its absent partner is never loaded
                float bv = 0.f;
                if (half == 0 && tok[t]) bv = sp[(long)(2 * nkp) * hw];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wl[(long)(kbase + nkp) * 64], bv, acc, 0, 0, 0);
            }
            kbase += (C + 1) >> 1;
        }
    }
    if (!valid) return;
    const int OW = 2 * w_;
    float* ob = out + (long)n * Cout * 4 * hw + (long)(2 * iy + a) * OW + 2 * ix + b;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = 4 * half + (r & 3) + 8 * (r >> 2);
        if (co < Cout) ob[(long)co * 4 * hw] = fmaxf(acc[r] + bfr[r >> 2][r & 3], 0.f);
    }
}

// -------------------------------------------------------------------------------------
// deconv4: the same MFMA form with ALL FOUR output parities in one wave.  A wave owns 32 input
// cells; per channel pair it loads the 9 shifted input views (dy, dx in {-1,0,1}) ONCE and feeds
// the 16 MFMAs (4 parities x 4 taps, four independent accumulator chains) from them: 9 + 4 loads
// per 16 MFMAs instead of 32, the input is read 9x instead of 16x, and every lane owns the 2x2
// output quad of its cell, so the stores are 8-byte pairs forming full 256-byte rows (the
// per-parity kernel wrote every other float).  Weights: [parity][channel pair][lane] x 4 taps.
// DUAL = false (plain head): the refined source only; no raw pointer, no raw pairs in the weights.
// -------------------------------------------------------------------------------------
template <int NB, bool DUAL>
__global__ __launch_bounds__(256) void deconv4_kernel(const float* __restrict__ inA, int Ca,
                                                      const float* __restrict__ inB, int Cb,
                                                      const f32x4* __restrict__ wq,   // [NB][4][Ct/2][64] x 4 taps
                                                      const float* __restrict__ bias, // [NB][2][16], D-frag order
                                                      float* __restrict__ out, long NP, int h, int w_,
                                                      int Cout, int xcd_remap) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    // neighbouring 128-cell strips share their +-1 halo rows: keep them on one XCD (see xcd_contiguous_id)
    const int bid = xcd_remap ? xcd_contiguous_id(blockIdx.x, gridDim.x) : blockIdx.x;
    const long px0 = ((long)bid * 4 + wave) * 32;
    if (px0 >= NP) return;
    const int half = lane >> 5, pl = lane & 31;
    const long g = px0 + pl;
    const bool valid = g < NP;
    const long gc = valid ? g : NP - 1;
    const int hw = h * w_;
    const int n = (int)(gc / hw);
    const int p = (int)(gc - (long)n * hw);
    const int iy = p / w_, ix = p - iy * w_;
    int voff[9];
    bool vok[9];
#pragma unroll
    for (int v = 0; v < 9; ++v) {
        const int y = iy + v / 3 - 1, x = ix + v % 3 - 1;
        vok[v] = y >= 0 && y < h && x >= 0 && x < w_;
        voff[v] = vok[v] ? y * w_ + x : p;
    }
    f32x16 acc[NB][4];
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][q][r] = 0.f;
    f32x4 bfr[NB][4];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const f32x4* bp = reinterpret_cast<const f32x4*>(bias + (i * 2 + half) * 16);
#pragma unroll
        for (int q = 0; q < 4; ++q) bfr[i][q] = bp[q];
    }
    const int CP = (DUAL ? Ca + Cb : Ca) >> 1, CPA = Ca >> 1;
    const f32x4* wl = wq + lane;
    const float* spA = inA + ((long)n * Ca + half) * hw;
    const float* spB = DUAL ? inB + ((long)n * Cb + half) * hw : spA;
    // channel pair cp (A channels first, then B): 9 raw views + the weight quads of every (block, parity)
    auto fetch = [&](int cp, float (&bv)[9], f32x4 (&av)[NB][4]) {
        const int c = min(cp, CP - 1);                   // the tail prefetch re-loads the last pair (unused)
        const float* cpn = (!DUAL || c < CPA) ? spA + (long)(2 * c) * hw : spB + (long)(2 * (c - CPA)) * hw;
#pragma unroll
        for (int v = 0; v < 9; ++v) bv[v] = cpn[voff[v]];     // raw; masked where it is consumed
#pragma unroll
        for (int i = 0; i < NB; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) av[i][q] = wl[((long)(i * 4 + q) * CP + c) * 64];
    };
    // taps: a=0: (dy 0, ky 1), (dy -1, ky 3);  a=1: (dy +1, ky 0), (dy 0, ky 2)   (same in x)
    auto mma = [&](const float (&raw)[9], const f32x4 (&av)[NB][4]) {
        float bv[9];
#pragma unroll
        for (int v = 0; v < 9; ++v) bv[v] = vok[v] ? raw[v] : 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int tyi = t >> 1, txi = t & 1;
#pragma unroll
            for (int i = 0; i < NB; ++i)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int a = q >> 1, b = q & 1;
                    const int dy = a == 0 ? (tyi == 0 ? 0 : -1) : (tyi == 0 ? 1 : 0);
                    const int dx = b == 0 ? (txi == 0 ? 0 : -1) : (txi == 0 ? 1 : 0);
                    acc[i][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i][q][t], bv[(dy + 1) * 3 + dx + 1], acc[i][q],
                                                                     0, 0, 0);
                }
        }
    };
    // two register sets, loop unrolled by two (CP is even): the loads of pair cp+1 are in flight
    // under the 16*NB MFMAs of pair cp
    float bv0[9], bv1[9];
    f32x4 av0[NB][4], av1[NB][4];
    fetch(0, bv0, av0);
#pragma unroll 1
    for (int cp = 0; cp < CP; cp += 2) {
        fetch(cp + 1, bv1, av1);
        __builtin_amdgcn_sched_barrier(0);               // loads first, then the MFMAs they hide under
        mma(bv0, av0);
        __builtin_amdgcn_sched_barrier(0);
        fetch(cp + 2, bv0, av0);
        __builtin_amdgcn_sched_barrier(0);
        mma(bv1, av1);
        __builtin_amdgcn_sched_barrier(0);
    }
    if (!valid) return;
    const int OW = 2 * w_;
    float* ob = out + (long)n * Cout * 4 * hw + (long)(2 * iy) * OW + 2 * ix;
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = i * 32 + 4 * half + (r & 3) + 8 * (r >> 2);
            if (co < Cout) {
                const float bb = bfr[i][r >> 2][r & 3];
                float* o = ob + (long)co * 4 * hw;
                const float2 top = {fmaxf(acc[i][0][r] + bb, 0.f), fmaxf(acc[i][1][r] + bb, 0.f)};
                const float2 bot = {fmaxf(acc[i][2][r] + bb, 0.f), fmaxf(acc[i][3][r] + bb, 0.f)};
                *reinterpret_cast<float2*>(o) = top;
                *reinterpret_cast<float2*>(o + OW) = bot;
            }
        }
}

void launch_deconv4(const float* inA, int Ca, const float* inB, int Cb, const float* wq, const float* bias,
                    float* out, int N, int h, int w_, int Cout, hipStream_t s) {
    const long NP = (long)N * h * w_;
    dim3 grid((unsigned)((NP + 127) / 128)), block(256);
#define LP_D4(NBV, DV) LP_LAUNCH((deconv4_kernel<NBV, DV>), grid, block, 0, s, inA, Ca, inB, Cb, (const f32x4*)wq, bias, \
                                 out, NP, h, w_, Cout, xcd_remap_mode())
    if (inB) { if (Cout <= 32) LP_D4(1, true); else LP_D4(2, true); }
    else { if (Cout <= 32) LP_D4(1, false); else LP_D4(2, false); }        // plain head: the one-source form
#undef LP_D4
    last_kernel_tag = "deconv4_kernel";
}


// -------------------------------------------------------------------------------------
// deconv4x3: deconv4 on the exact bf16x3 split (split3.h).  The fp32 form is matrix-core bound
// (16 v_mfma_f32_32x32x2_f32 = 1024 cycles per channel PAIR and wave); here a k-step is 16 channels
// (lanes 0-31: channels 16ks..16ks+7, lanes 32-63: 16ks+8..15 of the concatenated sources) and a
// (parity, tap) product is six v_mfma_f32_32x32x16_bf16 = 192 cycles per 16 channels -- 2.67x fewer
// matrix-core cycles at fp32 accuracy.
//
// A workgroup owns a 2-D tile of ONE image: 4 waves x 32 cells, TW = 32 or 16 columns wide (D4X3 below).  The tile
// plus a one-cell halo is staged ONCE: every input value is loaded once (dword loads, lanes along the rows of the halo
// tile), split once into hi / mid / lo and stored as the 16-byte B-fragment record the MFMA reads (8 channels of one
// cell, one record per piece, the three pieces of a cell side by side: 48 B per cell and channel group).  Cells
// outside the image are stored as zeros.  The nine shifted views of a k-step are then three ds_read_b128 each at a cell
// offset; a view feeds every (parity, tap) that reads it (centre 4, edges 2, corners 1).  The 48-byte cell stride puts
// the 16 lanes of every ds_read_b128 lane group on 16 distinct 16-byte slots and the 8 lanes of every ds_write_b128
// group on disjoint banks (tools/lds_model.py, deconv4x3).
// K is staged in equal slabs of at most D4X3::slab_groups() channel groups (48 channels at TW = 32: 58.75 KB, below the
// 64 KB that need an attribute; the launcher sizes them); one slab holds all of K <= 48.  The workgroups that share a
// CU (3 at K = 40) cover each other's staging.  Raw fp32 records (32 B per cell and group instead of 48) would keep
// the split on the nine views' side, 9x the VALU work, for a third less LDS: not taken.
// Each accumulator receives the sequence of the first form of this kernel (views fetched from global memory one at a
// time): k-steps ascending, views 0..8, the (q, t) order below, mma6's piece order; a cell's result does not depend on
// which cells share its wave, so the output is bit-identical to that form on every shape.
// Weights: [block][parity][tap][ks][piece hi,mid,lo][64 lanes] x 16 B.  DUAL = false (plain head): the refined source only.
// Bound: no longer the input side.  deconv.2 of XS runs at ~40 % of its MFMA floor (launcher comment); the 48 KB of A
// fragments per wave and k-step (64 B/clk per CU at the MFMA rate, from L2: 144 KB of weights do not fit L1) is the
// candidate, not yet measured.
// -------------------------------------------------------------------------------------
struct D4X3 {
    // tile geometry as a function of the plane width alone: 32 columns x 4 rows, or 16 columns x 8 rows for planes
    // <= 16 wide.  A wave owns 32 cells: one row of 32 or two rows of 16.  Halo rows are RS cells apart: 34 at TW = 32;
    // 32 at TW = 16 (18 used), so that a wave's second row starts a multiple of 16 cells after its first and the
    // 16-lane groups of ds_read_b128 stay on distinct slots.
    __host__ __device__ static constexpr int twl(int w) { return w <= 16 ? 4 : 5; }
    __host__ __device__ static constexpr int rows(int twl) { return 4 * (32 >> twl); }
    __host__ __device__ static constexpr int rs(int twl) { return twl == 5 ? 34 : 32; }
    __host__ __device__ static constexpr int cells(int twl) { return (rows(twl) + 2) * rs(twl); }   // 204 / 320
    __host__ __device__ static constexpr int slab_groups(int twl) { return twl == 5 ? 6 : 4; }      // 58 752 / 61 440 B
    static constexpr int REC = 48;                       // bytes per cell and channel group: hi, mid, lo records
};

// p-th (view, parity, tap) product of a k-step: views 0..8 ascending, within a view the parities, then the taps
// taps: a=0: (dy 0, ky 1), (dy -1, ky 3);  a=1: (dy +1, ky 0), (dy 0, ky 2)   (same in x)
struct D4Prod { int v, q, t; };
__host__ __device__ constexpr D4Prod d4x3_prod(int p) {
    int k = 0;
    for (int v = 0; v < 9; ++v)
        for (int q = 0; q < 4; ++q)
            for (int t = 0; t < 4; ++t) {
                const int a = q >> 1, b = q & 1, tyi = t >> 1, txi = t & 1;
                const int dy = a == 0 ? (tyi == 0 ? 0 : -1) : (tyi == 0 ? 1 : 0);
                const int dx = b == 0 ? (txi == 0 ? 0 : -1) : (txi == 0 ? 1 : 0);
                if (dy == v / 3 - 1 && dx == v % 3 - 1) {
                    if (k == p) return {v, q, t};
                    ++k;
                }
            }
    return {0, 0, 0};
}
template <class F, int... U>
__device__ __forceinline__ void d4x3_units(F&& f, std::integer_sequence<int, U...>) {
    (f(std::integral_constant<int, U>{}), ...);
}

template <int NB, bool DUAL>
__global__ __launch_bounds__(256, NB == 1 ? 3 : 2) void deconv4x3_kernel(
    const float* __restrict__ inA, int Ca, const float* __restrict__ inB, int Cb, const u32x4* __restrict__ ws,
    const float* __restrict__ bias, float* __restrict__ out, int tilesX, int tilesY, int h, int w_, int Cout,
    int SG, int xcd_remap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char d4s[];   // [slab group][halo cell][hi, mid, lo] x 16 B
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    // neighbouring tiles share their halo: keep them on one XCD (see xcd_contiguous_id)
    const int bid = xcd_remap ? xcd_contiguous_id(blockIdx.x, gridDim.x) : blockIdx.x;
    const int twl = D4X3::twl(w_), TW = 1 << twl, RS = D4X3::rs(twl), HW2 = TW + 2;
    const int NCELL = D4X3::cells(twl);
    const int CPG = (D4X3::rows(twl) + 2) * HW2;          // cells of the halo tile that are staged (per group)
    const int tpi = tilesX * tilesY;
    const int n = bid / tpi, t = bid - n * tpi;
    const int ty = t / tilesX, tx = t - ty * tilesX;
    const int y0 = ty * D4X3::rows(twl), x0 = tx * TW;
    const int half = lane >> 5, pl = lane & 31;
    const int ry = wave * (32 >> twl) + (pl >> twl), cx = pl & (TW - 1);
    const int iy = y0 + ry, ix = x0 + cx;
    const bool valid = iy < h && ix < w_;
    const bool wave_live = y0 + wave * (32 >> twl) < h;   // wave-uniform: a wave below the image runs no MFMA
    const int hw = h * w_;
    f32x16 acc[NB][4];
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][q][r] = 0.f;
    const int Ga = Ca >> 3, G8 = (DUAL ? Ca + Cb : Ca) >> 3, KS = (G8 + 1) >> 1;
    const float* baseA = inA + (long)n * Ca * hw;
    const float* baseB = DUAL ? inB + (long)n * Cb * hw : baseA;
    // this lane's cell in the halo tile is (ry + 1, cx + 1); view (dy, dx) is the record (dy * RS + dx) cells from it
    const unsigned char* cell = d4s + ((ry + 1) * RS + cx + 1) * D4X3::REC;
    // the 16 NB (view, parity, tap, block) products of a k-step in accumulation order; their A fragments go through a
    // ring of DEPTH register sets, loaded DEPTH - 1 products ahead (across k-steps and slabs: the weights are global)
    constexpr int UN = 16 * NB, DEPTH = NB == 1 ? 2 : 4;   // NB = 1: 168 registers (3 waves per SIMD) hold two sets
    u32x4 ar[DEPTH][3];
    auto fetch_a = [&](int ksn, auto uc) {
        constexpr int u = decltype(uc)::value, i = u % NB;
        constexpr D4Prod pr = d4x3_prod(u / NB);
        const u32x4* wp = ws + ((long)((i * 4 + pr.q) * 4 + pr.t) * KS + ksn) * 3 * 64;   // wave-uniform base + lane
        ar[u % DEPTH][0] = wp[lane];
        ar[u % DEPTH][1] = wp[64 + lane];
        ar[u % DEPTH][2] = wp[128 + lane];
    };
    constexpr int U = 4;                                  // (group, cell) items a thread has in flight while staging
#pragma unroll 1
    for (int g0 = 0; g0 < G8; g0 += SG) {
        const int ng = min(SG, G8 - g0), items = ng * CPG;
        if (g0) __syncthreads();                          // every wave is done reading the previous slab
#pragma unroll 1
        for (int it = threadIdx.x; it < items; it += 256 * U) {
            float raw[U][8];
            int dst[U];
            bool ok[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int e = min(it + 256 * u, items - 1);            // the tail re-does the last item (same values)
                const int gl = e / CPG, c = e - gl * CPG;
                const int r = c / HW2, x = c - r * HW2;
                const int gy = y0 - 1 + r, gx = x0 - 1 + x;
                ok[u] = gy >= 0 && gy < h && gx >= 0 && gx < w_;
                const int gq = g0 + gl;
                const float* sp = (!DUAL || gq < Ga) ? baseA + (long)(8 * gq) * hw : baseB + (long)(8 * (gq - Ga)) * hw;
                sp += ok[u] ? gy * w_ + gx : 0;                        // outside the image: any valid address, zeroed below
                dst[u] = (gl * NCELL + r * RS + x) * D4X3::REC;
#pragma unroll
                for (int ch = 0; ch < 8; ++ch) raw[u][ch] = sp[(long)ch * hw];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                u32x4 fh, fm, fl;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const Split3 s3 = split3_pair(ok[u] ? raw[u][2 * j] : 0.f, ok[u] ? raw[u][2 * j + 1] : 0.f);
                    fh[j] = s3.h;
                    fm[j] = s3.m;
                    fl[j] = s3.l;
                }
                u32x4* rec = reinterpret_cast<u32x4*>(d4s + dst[u]);
                rec[0] = fh;
                rec[1] = fm;
                rec[2] = fl;
            }
        }
        if (g0 == 0) {                                    // the ring's first sets, in flight across the barrier
            d4x3_units([&](auto uc) { fetch_a(0, uc); }, std::make_integer_sequence<int, DEPTH - 1>{});
        }
        __syncthreads();
        if (!wave_live) continue;
        const int ks1 = (g0 + ng + 1) >> 1;
#pragma unroll 1
        for (int ks = g0 >> 1; ks < ks1; ++ks) {
            // beyond the last group (odd group count): the last group's data again, against zero weights
            const int gl = min(2 * ks + half, G8 - 1) - g0;
            const unsigned char* kc = cell + gl * NCELL * D4X3::REC;
            const int ksn = min(ks + 1, KS - 1);          // the tail re-loads the last k-step's weights (unused)
            u32x4 bf[2][3];                               // views v, v + 1
            auto view = [&](int v, u32x4 (&b)[3]) {
                const u32x4* rec = reinterpret_cast<const u32x4*>(kc + ((v / 3 - 1) * RS + v % 3 - 1) * D4X3::REC);
                b[0] = rec[0];
                b[1] = rec[1];
                b[2] = rec[2];
            };
            view(0, bf[0]);
            d4x3_units([&](auto uc) {
                constexpr int u = decltype(uc)::value, pi = u / NB, i = u % NB;
                constexpr D4Prod pr = d4x3_prod(pi);
                constexpr bool first = i == 0 && (pi == 0 || d4x3_prod(pi - 1).v != pr.v);
                // the weights of the product DEPTH - 1 ahead and the next view's records are in flight under this one's MFMAs
                if constexpr (u + DEPTH - 1 < UN) fetch_a(ks, std::integral_constant<int, u + DEPTH - 1>{});
                else fetch_a(ksn, std::integral_constant<int, u + DEPTH - 1 - UN>{});
                if constexpr (first && pr.v < 8) view(pr.v + 1, bf[(pr.v + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
                acc[i][pr.q] = mma6(ar[u % DEPTH], bf[pr.v & 1][0], bf[pr.v & 1][1], bf[pr.v & 1][2], acc[i][pr.q]);
                __builtin_amdgcn_sched_barrier(0);
            }, std::make_integer_sequence<int, UN>{});
        }
    }
    if (!valid) return;
    const int OW = 2 * w_;
    float* ob = out + (long)n * Cout * 4 * hw + (long)(2 * iy) * OW + 2 * ix;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const f32x4* bp = reinterpret_cast<const f32x4*>(bias + (i * 2 + half) * 16);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = i * 32 + 4 * half + (r & 3) + 8 * (r >> 2);
            if (co < Cout) {
                const float bb = bp[r >> 2][r & 3];
                float* o = ob + (long)co * 4 * hw;
                const float2 top = {fmaxf(acc[i][0][r] + bb, 0.f), fmaxf(acc[i][1][r] + bb, 0.f)};
                const float2 bot = {fmaxf(acc[i][2][r] + bb, 0.f), fmaxf(acc[i][3][r] + bb, 0.f)};
                *reinterpret_cast<float2*>(o) = top;
                *reinterpret_cast<float2*>(o + OW) = bot;
            }
        }
    }
}

bool launch_deconv4x3(const float* inA, int Ca, const float* inB, int Cb, const void* ws, const float* bias,
                      float* out, int N, int h, int w_, int Cout, hipStream_t s) {
    if (!ws || (Ca & 7) || (Cb & 7) || Cout > 64) return false;
    // <= 16x16 input planes (deconv.0 at 256^2 / 512^2 inputs): with views fetched from global memory there were too few
    // waves for the longer per-wave chain (8-10 k-steps x 9 views in sequence) -- the fp32 kernel was faster there (48 vs
    // 79 us on XS, 116 vs 208 on M).  The LDS-staged body (8x16 tiles on such planes) has not been measured against it.
    // The rule depends on the LAYER SHAPE only, never on the batch size (batched == per-image bitwise, P4).
    // Measured, XS@256 64 + 64 images, one stream, same box (profiles/r09_deconv_kernel_stats_*.txt): global-memory views
    // 56.6 / 190.3 us (deconv.1 / deconv.2), LDS-staged 51.6 / 154.8 us; the MFMA floor of deconv.2 is 61 us.
    if (h * w_ <= 256) return false;
    const int twl = D4X3::twl(w_), G8 = (Ca + (inB ? Cb : 0)) >> 3;
    const int tilesX = (w_ + (1 << twl) - 1) >> twl, tilesY = (h + D4X3::rows(twl) - 1) / D4X3::rows(twl);
    // slabs of equal size (an even group count, so that a slab ends on a k-step): K = 56 is 4 + 3 groups, not 6 + 1
    const int nslab = (G8 + D4X3::slab_groups(twl) - 1) / D4X3::slab_groups(twl);
    const int SG = (((G8 + nslab - 1) / nslab) + 1) & ~1;
    const size_t lds = (size_t)(G8 < SG ? G8 : SG) * D4X3::cells(twl) * D4X3::REC;
    dim3 grid((unsigned)((long)N * tilesX * tilesY)), block(256);
#define LP_D4X3(NBV, DV) LP_LAUNCH((deconv4x3_kernel<NBV, DV>), grid, block, lds, s, inA, Ca, inB, Cb, (const u32x4*)ws, bias, \
                                   out, tilesX, tilesY, h, w_, Cout, SG, xcd_remap_mode())
    if (inB) { if (Cout <= 32) LP_D4X3(1, true); else LP_D4X3(2, true); }
    else { if (Cout <= 32) LP_D4X3(1, false); else LP_D4X3(2, false); }    // plain head: the one-source form
#undef LP_D4X3
    last_kernel_tag = "deconv4x3_kernel";
    return true;
}

void launch_deconv_mfma(const float* inA, int Ca, const float* inB, int Cb, const float* wp,
                        const float* bias, float* out, int N, int h, int w_, int Cout, hipStream_t s) {
    const long NP = (long)N * h * w_;
    dim3 grid((unsigned)((NP + 127) / 128), 4), block(256);
    if (inB)
        LP_LAUNCH(deconv_mfma_kernel<true>, grid, block, 0, s, inA, Ca, inB, Cb, wp, bias, out, NP, h, w_, Cout);
    else                                                                   // plain head: the one-source form
        LP_LAUNCH(deconv_mfma_kernel<false>, grid, block, 0, s, inA, Ca, inB, Cb, wp, bias, out, NP, h, w_, Cout);
    last_kernel_tag = "deconv_mfma_kernel";
}

void launch_deconv_pair(const float* inA, int Ca, const float* inB, int Cb, const float* w,
                        const float* b, float* out, int N, int h, int w_, int Cout, hipStream_t s) {
    const long total = (long)N * h * w_;
    dim3 grid((unsigned)((total + 255) / 256), (Cout + COT - 1) / COT), block(256);
    if (inB)
        LP_LAUNCH(deconv_pair_kernel<true>, grid, block, 0, s, inA, Ca, inB, Cb, w, b, out, N, h, w_, Cout);
    else                                                                   // plain head: the one-source form
        LP_LAUNCH(deconv_pair_kernel<false>, grid, block, 0, s, inA, Ca, inB, Cb, w, b, out, N, h, w_, Cout);
    last_kernel_tag = "deconv_pair_kernel";
}

}  // namespace lp
