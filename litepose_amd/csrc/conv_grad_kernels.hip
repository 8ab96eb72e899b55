// Backward of the two dense layers of the trainable module (lp_stem_* / lp_deconv_*, layer_api.cpp): the weight gradient
// of the 3x3 stride-2 stem convolution and both gradients of the ConvTranspose2d(k4, s2, p1) pair of the Fusion Deconv
// Head.  The forwards are launch_stem_raw / launch_deconv_raw (calib_kernels.hip).  fp32, planar NCHW, no atomics: every
// sum has one order that depends on the shapes only, so two calls (and a graph replay) give the same bits.
//
// All three are GEMMs on v_mfma_f32_32x32x2_f32 (A[row = l & 31][k = l >> 5], B[k = l >> 5][col = l & 31], D register i of
// lane l: row (i & 3) + 8 (i >> 2) + 4 (l >> 5), column l & 31) whose convolution operand is read from a patch staged in
// LDS, zeros where the plane ends: a term that meets padding is an exact zero product, a tap that only ever meets padding
// comes out exactly zero.
//
//   deconv weight gradient   dW[ci][co][ky][kx] = sum over cells of x[n][ci][iy][ix] * dY[n][co][2iy-1+ky][2ix-1+kx]:
//                            rows ci (both sources), columns (co, tap), reduction over the input cells.  The cells are
//                            taken in tiles of 8x8 (unit = n * tiles + tile); per tile the (2*8+2)^2 dY patch of 8 output
//                            channels and the 32 x 64 block of x are staged in LDS, a wave owns 32 rows x (2 channels x 16
//                            taps).  Slices of LP_DECONV_WGRAD_SLICE cells -> fp32 partials [slices][Ca+Cb][Cout][16] ->
//                            slice_sum_kernel (fp64, index order, one rounding)
//   deconv data gradient     dX[n][ci][iy][ix] = sum over (co, tap) of w[ci][co][tap] * dY[n][co][2iy-1+ky][2ix-1+kx]: rows
//                            ci, columns the 64 cells of a tile, reduction over 16 Cout in chunks of 8 output channels
//                            whose patch is staged as above; the weights are the concatenated copy launch_deconv_pack
//                            leaves in the workspace (64-byte rows: 16-byte loads).  A gather, no scatter.
//   stem weight gradient     dW[co][ci][ky][kx] = sum over (n, oy, ox) of dY[n][co][oy][ox] * x[n][ci][2oy-1+ky][2ox-1+kx]:
//                            one 32 x 27 tile (padded to 32 columns of zeros), reduction over the output pixels in tiles
//                            of 8 x 16 (unit = n * tiles + tile); the 3 x 17 x 33 input patch and the 32 x 128 block of dY
//                            are staged in LDS, the four waves take two tile rows each and are added pairwise.  Slices of
//                            LP_STEM_WGRAD_SLICE pixels -> fp32 partials [slices][32][27] -> slice_sum_kernel
#include "../../include/litepose_amd.h"
#include "kernels.h"

namespace lp {

typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));

// ====================================================================================== ConvTranspose2d(k4, s2, p1) pair
constexpr int DT = 8;                       // a tile is DT x DT input cells
constexpr int DP = 2 * DT + 2;              // its dY patch: rows / columns 2 iy0 - 1 .. 2 (iy0 + DT)
constexpr int DPS = DP * DP;
constexpr int DCO = 8;                      // output channels staged at a time
constexpr int DXS = DT * DT + 1;            // row stride of the staged x block: 32 rows read by 32 lanes, no bank shared
static_assert(LP_DECONV_WGRAD_SLICE % (DT * DT) == 0, "a slice is a whole number of tiles");

// wa [Ca][Cout][16] | wb [Cb][Cout][16] -> wp [Ca+Cb][Cout][16]
__global__ __launch_bounds__(256) void deconv_pack_kernel(const float* __restrict__ wa, int na, const float* __restrict__ wb,
                                                          int nb, float* __restrict__ wp) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx < na) wp[idx] = wa[idx];
    else if (idx < na + nb) wp[idx] = wb[idx - na];
}

// the dY patch of channels co0 .. co0 + DCO - 1 for the tile at (iy0, ix0) of image n: zeros outside the plane and beyond Cout
__device__ __forceinline__ void deconv_stage_patch(float* patch, const float* __restrict__ dy, int n, int Cout, int co0,
                                                   int OH, int OW, int iy0, int ix0) {
    const int oy0 = 2 * iy0 - 1, ox0 = 2 * ix0 - 1;
    for (int e = threadIdx.x; e < DCO * DPS; e += 256) {
        const int c = e / DPS, q = e - c * DPS;
        const int py = q / DP, px = q - py * DP;
        const int oy = oy0 + py, ox = ox0 + px, co = co0 + c;
        const bool ok = co < Cout && oy >= 0 && oy < OH && ox >= 0 && ox < OW;
        const float v = dy[ok ? ((long)n * Cout + co) * OH * OW + (long)oy * OW + ox : 0];
        patch[e] = ok ? v : 0.f;
    }
}

// grid (slices, ceil((Ca+Cb) / 32), ceil(Cout / DCO)); wave v of a workgroup owns channels co0 + 2 v, + 1
__global__ __launch_bounds__(256) void deconv_wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ xa,
                                                           const float* __restrict__ xb, float* __restrict__ part, int N,
                                                           int Ca, int Cb, int Cout, int h, int w, int tilesX, int tiles) {
    __shared__ float patch[DCO * DPS];
    __shared__ float xs[32 * DXS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int half = lane >> 5, r = lane & 31;
    const int slice = blockIdx.x, ci0 = blockIdx.y * 32, co0 = blockIdx.z * DCO;
    const int M = Ca + Cb, OH = 2 * h, OW = 2 * w;
    constexpr int UPS = LP_DECONV_WGRAD_SLICE / (DT * DT);
    const int units = N * tiles;
    const int u0 = slice * UPS, u1 = min(u0 + UPS, units);
    // B: column r = (channel 2 wave + (r >> 4), tap r & 15 = ky * 4 + kx); cell e + 32 half of the tile per MFMA e
    const float* bp = patch + (2 * wave + (r >> 4)) * DPS + ((r & 15) >> 2) * DP + (r & 3) + 8 * half * DP;
    const float* ap = xs + r * DXS + 32 * half;
    f32x16_t acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int u = u0; u < u1; ++u) {
        const int n = u / tiles, t = u - n * tiles;
        const int ty = t / tilesX, tx = t - ty * tilesX;
        const int iy0 = ty * DT, ix0 = tx * DT;
        deconv_stage_patch(patch, dy, n, Cout, co0, OH, OW, iy0, ix0);
        for (int e = threadIdx.x; e < 32 * DT * DT; e += 256) {
            const int row = e >> 6, c = e & 63;
            const int iy = iy0 + (c >> 3), ix = ix0 + (c & 7), ci = ci0 + row;
            const bool ok = ci < M && iy < h && ix < w;
            const bool fromb = ok && ci >= Ca;
            const float* src = fromb ? xb : xa;
            const long plane = fromb ? (long)n * Cb + (ci - Ca) : (long)n * Ca + ci;
            const float v = src[ok ? plane * h * w + (long)iy * w + ix : 0];
            xs[row * DXS + c] = ok ? v : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 32; ++e)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[e], bp[2 * (e >> 3) * DP + 2 * (e & 7)], acc, 0, 0, 0);
        __syncthreads();
    }
    const int co = co0 + 2 * wave + (r >> 4), tap = r & 15;
    float* pb = part + (long)slice * M * Cout * 16;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int ci = ci0 + (i & 3) + 8 * (i >> 2) + 4 * half;
        if (ci < M && co < Cout) pb[((long)ci * Cout + co) * 16 + tap] = acc[i];
    }
}

// grid (N * tiles, ceil(ceil((Ca+Cb) / 32) / 2)); wave v: cells 32 (v & 1) .. + 31 of the tile, row block 2 blockIdx.y + (v >> 1)
__global__ __launch_bounds__(256) void deconv_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ wp,
                                                           float* __restrict__ gxa, float* __restrict__ gxb, int Ca, int Cb,
                                                           int Cout, int h, int w, int tilesX, int tiles) {
    __shared__ float patch[DCO * DPS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int half = lane >> 5, r = lane & 31;
    const int n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
    const int ty = t / tilesX, tx = t - ty * tilesX;
    const int iy0 = ty * DT, ix0 = tx * DT;
    const int M = Ca + Cb, OH = 2 * h, OW = 2 * w;
    const int rb = 2 * blockIdx.y + (wave >> 1);
    const bool live = rb * 32 < M;                                  // wave-uniform; an idle wave still stages and waits
    const int ci = rb * 32 + r;
    const bool ci_ok = ci < M;
    const int cic = ci_ok ? ci : M - 1;
    const int cell = 32 * (wave & 1) + r;
    // B: column r = the wave's cell; k = (channel 4 half + q of the chunk, tap j) for MFMA 16 q + j
    const float* bp = patch + 4 * half * DPS + 2 * (cell >> 3) * DP + 2 * (cell & 7);
    f32x16_t acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int co0 = 0; co0 < Cout; co0 += DCO) {
        deconv_stage_patch(patch, dy, n, Cout, co0, OH, OW, iy0, ix0);
        __syncthreads();
        if (live) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int co = co0 + 4 * half + q;
                const bool ok = ci_ok && co < Cout;
                const f32x4_t* wr = reinterpret_cast<const f32x4_t*>(wp + ((long)cic * Cout + (co < Cout ? co : Cout - 1)) * 16);
                f32x4_t a[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    a[k] = wr[k];
                    if (!ok) a[k] = f32x4_t{0.f, 0.f, 0.f, 0.f};
                }
#pragma unroll
                for (int j = 0; j < 16; ++j)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j >> 2][j & 3], bp[q * DPS + (j >> 2) * DP + (j & 3)], acc, 0,
                                                               0, 0);
            }
        }
        __syncthreads();
    }
    const int iy = iy0 + (cell >> 3), ix = ix0 + (cell & 7);
    if (!live || iy >= h || ix >= w) return;
    const long o = (long)iy * w + ix;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int row = rb * 32 + (i & 3) + 8 * (i >> 2) + 4 * half;
        if (row < Ca) gxa[((long)n * Ca + row) * h * w + o] = acc[i];
        else if (row < M) gxb[((long)n * Cb + (row - Ca)) * h * w + o] = acc[i];
    }
}

static int deconv_tiles(int h, int w) { return ((h + DT - 1) / DT) * ((w + DT - 1) / DT); }

int deconv_wgrad_slices(int N, int h, int w) {
    const long cells = (long)N * deconv_tiles(h, w) * (DT * DT);
    return (int)((cells + LP_DECONV_WGRAD_SLICE - 1) / LP_DECONV_WGRAD_SLICE);
}

void launch_deconv_pack(const float* wa, const float* wb, float* wp, int Ca, int Cb, int Cout, hipStream_t s) {
    const int na = Ca * Cout * 16, nb = Cb * Cout * 16;
    LP_LAUNCH(deconv_pack_kernel, dim3((unsigned)((na + nb + 255) / 256)), dim3(256), 0, s, wa, na, wb, nb, wp);
}

void launch_deconv_backward(const float* dy, const float* xa, const float* xb, const float* wp, float* gxa, float* gxb,
                            float* part, float* gwa, float* gwb, int N, int Ca, int Cb, int Cout, int h, int w,
                            hipStream_t s) {
    const int tilesX = (w + DT - 1) / DT, tiles = deconv_tiles(h, w);
    const int M = Ca + Cb, rbs = (M + 31) / 32;
    if (gxa)
        LP_LAUNCH(deconv_dgrad_kernel, dim3((unsigned)(N * tiles), (rbs + 1) / 2), dim3(256), 0, s, dy, wp, gxa, gxb, Ca, Cb,
                  Cout, h, w, tilesX, tiles);
    if (gwa) {
        const int S = deconv_wgrad_slices(N, h, w);
        LP_LAUNCH(deconv_wgrad_kernel, dim3(S, rbs, (Cout + DCO - 1) / DCO), dim3(256), 0, s, dy, xa, xb, part, N, Ca, Cb,
                  Cout, h, w, tilesX, tiles);
        const int stride = M * Cout * 16, na = Ca * Cout * 16;
        launch_slice_sum(part, S, stride, na, gwa, s);
        if (Cb) launch_slice_sum(part + na, S, stride, stride - na, gwb, s);
    }
}

// ====================================================================================== stem: weight gradient
constexpr int STH = 8, STW = 16;            // a tile is STH x STW output pixels
constexpr int SPH = 2 * STH + 1, SPW = 2 * STW + 1, SPS = SPH * SPW;   // its input patch, per input channel
constexpr int SYS = STH * STW + 1;          // row stride of the staged dY block
static_assert(LP_STEM_WGRAD_SLICE % (STH * STW) == 0, "a slice is a whole number of tiles");
static_assert(32 * SYS >= 4 * 1024, "the staged dY block is reused for the four waves' tiles");

// grid (slices); wave v takes tile rows 2 v and 2 v + 1: MFMA e reduces the pixels (2 v, e) and (2 v + 1, e)
__global__ __launch_bounds__(256) void stem_wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                         float* __restrict__ part, int N, int H, int W, int tilesX,
                                                         int tiles) {
    __shared__ float xs[3 * SPS];
    __shared__ float dys[32 * SYS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int half = lane >> 5, r = lane & 31;
    const int slice = blockIdx.x;
    const int OH = H >> 1, OW = W >> 1;
    constexpr int UPS = LP_STEM_WGRAD_SLICE / (STH * STW);
    const int units = N * tiles;
    const int u0 = slice * UPS, u1 = min(u0 + UPS, units);
    // B: column r = ci * 9 + ky * 3 + kx below 27, zero above
    const bool col_ok = r < 27;
    const int j = col_ok ? r : 0;
    const int py = 2 * wave + half;
    const float* bp = xs + (j / 9) * SPS + ((j % 9) / 3) * SPW + (j % 3) + 2 * py * SPW;
    const float* ap = dys + r * SYS + py * STW;
    f32x16_t acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int u = u0; u < u1; ++u) {
        const int n = u / tiles, t = u - n * tiles;
        const int ty = t / tilesX, tx = t - ty * tilesX;
        const int oy0 = ty * STH, ox0 = tx * STW;
        for (int e = threadIdx.x; e < 3 * SPS; e += 256) {
            const int ci = e / SPS, q = e - ci * SPS;
            const int qy = q / SPW, qx = q - qy * SPW;
            const int iy = 2 * oy0 - 1 + qy, ix = 2 * ox0 - 1 + qx;
            const bool ok = iy >= 0 && iy < H && ix >= 0 && ix < W;
            const float v = x[ok ? ((long)n * 3 + ci) * H * W + (long)iy * W + ix : 0];
            xs[e] = ok ? v : 0.f;
        }
        for (int e = threadIdx.x; e < 32 * STH * STW; e += 256) {
            const int co = e >> 7, p = e & 127;
            const int oy = oy0 + (p >> 4), ox = ox0 + (p & 15);
            const bool ok = oy < OH && ox < OW;
            const float v = dy[ok ? ((long)n * 32 + co) * OH * OW + (long)oy * OW + ox : 0];
            dys[co * SYS + p] = ok ? v : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < STW; ++e) {
            const float b = bp[2 * e];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[e], col_ok ? b : 0.f, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    // the four waves' tiles, added pairwise in a fixed order
    float* red = dys;
#pragma unroll
    for (int i = 0; i < 16; ++i) red[wave * 1024 + ((i & 3) + 8 * (i >> 2) + 4 * half) * 32 + r] = acc[i];
    __syncthreads();
    for (int k = threadIdx.x; k < 1024; k += 256) {
        const int co = k >> 5, c = k & 31;
        if (c < 27) part[(long)slice * 864 + co * 27 + c] = (red[k] + red[1024 + k]) + (red[2048 + k] + red[3072 + k]);
    }
}

static int stem_tiles(int H, int W) { return ((H / 2 + STH - 1) / STH) * ((W / 2 + STW - 1) / STW); }

int stem_wgrad_slices(int N, int H, int W) {
    const long pixels = (long)N * stem_tiles(H, W) * (STH * STW);
    return (int)((pixels + LP_STEM_WGRAD_SLICE - 1) / LP_STEM_WGRAD_SLICE);
}

void launch_stem_wgrad(const float* dy, const float* x, float* part, float* dw, int N, int H, int W, hipStream_t s) {
    const int tilesX = (W / 2 + STW - 1) / STW, tiles = stem_tiles(H, W);
    const int S = stem_wgrad_slices(N, H, W);
    LP_LAUNCH(stem_wgrad_kernel, dim3(S), dim3(256), 0, s, dy, x, part, N, H, W, tilesX, tiles);
    launch_slice_sum(part, S, 864, 864, dw, s);
}

}  // namespace lp
