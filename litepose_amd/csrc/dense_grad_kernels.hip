// The dense K x K convolution as a training layer (lp_conv_*, layer_api.cpp): K in {3, 5, 7}, stride 1 / 2, pad K / 2, up to
// two channel-concatenated sources, optionally read through a nearest x2 upsample (UpConv), optionally biased -- every
// convolution of pose_resnet that is not 1x1.  fp32, planar NCHW, weights [Cout][C][K][K], no atomics: every sum has one
// order that depends on the shapes only, so two calls (and a graph replay) give the same bits.
//
//   forward           convk_pack_kernel turns the plain weights (+ bias, or zeros) into the bf16x3 A fragments convk3_kernel
//                     reads ([ceil(Cout/32)][K*K][ceil(Ct/16)][hi, mid, lo][64 lanes] x 16 B, plan.cpp pack_convk), then
//                     launch_convk3 (convk_kernels.hip), unchanged: the pattern of pw_pack_kernel -> launch_pw
//   data gradient     the same launch on dY with the flipped, transposed weights (convk_pack_kernel, transpose:
//                     w[co][ci][K-1-ky][K-1-kx] -> rows ci, reduction over co), one launch per source.
//                     stride 2: dY is first spread over the input plane (dilate2_kernel: Z[2oy][2ox] = dY[oy][ox], zeros
//                     elsewhere), so that the stride-1 launch is the gather over the taps of each cell's parity; the zero
//                     products are exact for finite operands (a non-finite weight tap poisons its whole input channel
//                     through them and through the staged halo: a known deviation).  ups: the launch writes the gradient of the upsampled plane into the workspace,
//                     pool2_kernel sums each 2x2 cell as (a + b) + (c + d)
//   weight gradient   dW_s[co][ci][ky][kx] = sum over (n, oy, ox) of dY[n][co][oy][ox] * X_s[n][ci][S oy - K/2 + ky][S ox - K/2 + kx]
//                     on v_mfma_f32_32x32x2_f32 (A[row = l & 31][k = l >> 5], B[k = l >> 5][col = l & 31], D register i of
//                     lane l: row (i & 3) + 8 (i >> 2) + 4 (l >> 5), column l & 31): rows co, columns (ci, tap) of a group of
//                     CG input channels, reduction over the output pixels in tiles of 8 x 16 (unit = n * tiles + tile).  Per
//                     tile the haloed input patch of the channel group (zeros outside the plane and beyond Ct, read
//                     through the upsample when ups) and the 32 x 128 block of dY are staged in LDS; a wave owns NCB column
//                     blocks of 32 and walks all 128 pixels; a pixel of the tile outside the output plane is SELECTED
//                     away (its partner is a real input cell wherever that cell lies in the plane, and 0 * NaN is a NaN).
//                     Slices of LP_CONV_WGRAD_SLICE pixels -> fp32 partials [slices][ Cout*Ca*K*K | Cout*Cb*K*K ] ->
//                     slice_sum_kernel (fp64, index order, one rounding).  A term that meets padding is a product with a
//                     staged zero -- an exact zero for finite operands, so that a tap that only ever meets padding comes
//                     out exactly zero; a non-finite dY at such a pixel poisons the tap, as torch's own padding does
//   bias gradient     per-channel sum of dY: fp64 partials of a fixed cut [Cout][SB], fixed tree per workgroup, added in
//                     index order, one rounding (the scheme of bn_bwd_stats_kernel)
#include "../../include/litepose_amd.h"
#include "kernels.h"
#include "split3.h"

namespace lp {

// ====================================================================================== packing for convk3_kernel
// One thread per (channel block, tap, k-step, lane): its 8 values, split exactly into hi / mid / lo.
// !transpose: rows co < Cout, k = ci over both sources.  transpose (one source, wa [Cout][Ca][KK]): rows ci < Ca, k = co,
// tap flipped.  bout: nb floats = bias (rows below M, when given) or zeros.
__global__ __launch_bounds__(256) void convk_pack_kernel(const float* __restrict__ wa, int Ca, const float* __restrict__ wb,
                                                         int Cb, int Cout, int KK, int transpose,
                                                         const float* __restrict__ bias, u32x4* __restrict__ ws,
                                                         float* __restrict__ bout, int nb, long total) {
    const int M = transpose ? Ca : Cout, Kt = transpose ? Cout : Ca + Cb;
    const int KS = (Kt + 15) >> 4;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx < nb) bout[idx] = (bias && idx < M) ? bias[idx] : 0.f;
    if (idx >= total) return;
    const int l = (int)(idx & 63);
    long q = idx >> 6;
    const int ks = (int)(q % KS);
    q /= KS;
    const int tap = (int)(q % KK), cb = (int)(q / KK);
    const int row = cb * 32 + (l & 31), k0 = ks * 16 + 8 * (l >> 5);
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int k = k0 + e;
        float x = 0.f;
        if (row < M && k < Kt) {
            if (transpose) x = wa[((long)k * Ca + row) * KK + (KK - 1 - tap)];
            else if (k < Ca) x = wa[((long)row * Ca + k) * KK + tap];
            else x = wb[((long)row * Cb + (k - Ca)) * KK + tap];
        }
        v[e] = x;
    }
    u32x4 fh, fm, fl;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const Split3 s3 = split3_pair(v[2 * j], v[2 * j + 1]);
        fh[j] = s3.h;
        fm[j] = s3.m;
        fl[j] = s3.l;
    }
    u32x4* d = ws + (((long)cb * KK + tap) * KS + ks) * 192 + l;
    d[0] = fh;
    d[64] = fm;
    d[128] = fl;
}

size_t convk_pack_bytes(int M, int Kt, int K) {
    return (size_t)((M + 31) / 32) * K * K * ((Kt + 15) / 16) * 192 * 16;
}

void launch_convk_pack(const float* wa, int Ca, const float* wb, int Cb, int Cout, int K, bool transpose, const float* bias,
                       void* ws, float* bout, hipStream_t s) {
    const int M = transpose ? Ca : Cout, Kt = transpose ? Cout : Ca + Cb;
    const int nb = ((M + 31) / 32) * 32;
    long total = (long)((M + 31) / 32) * K * K * ((Kt + 15) / 16) * 64;
    LP_LAUNCH(convk_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, wa, Ca, wb, Cb, Cout, K * K,
              transpose ? 1 : 0, bias, (u32x4*)ws, bout, nb, total);
}

// ====================================================================================== data gradient: helpers
// z [planes][2 OH][2 OW]: dY at the even cells, zeros elsewhere
__global__ __launch_bounds__(256) void dilate2_kernel(const float* __restrict__ dy, float* __restrict__ z, long total, int OH,
                                                      int OW) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int W = 2 * OW, H = 2 * OH;
    const int x = (int)(idx % W);
    const long q = idx / W;
    const int y = (int)(q % H);
    const long pl = q / H;
    const bool live = !((x | y) & 1);
    const float v = dy[live ? (pl * OH + (y >> 1)) * OW + (x >> 1) : 0];
    z[idx] = live ? v : 0.f;
}

// gx [planes][H][W] = the 2x2 cell sums of g [planes][2H][2W], (a + b) + (c + d)
__global__ __launch_bounds__(256) void pool2_kernel(const float* __restrict__ g, float* __restrict__ gx, long total, int H,
                                                    int W) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int x = (int)(idx % W);
    const long q = idx / W;
    const int y = (int)(q % H);
    const long pl = q / H;
    const float* r0 = g + ((pl * 2 * H + 2 * y) * 2 * W + 2 * x);
    const float* r1 = r0 + 2 * W;
    gx[idx] = (r0[0] + r0[1]) + (r1[0] + r1[1]);
}

void launch_dilate2(const float* dy, float* z, long planes, int OH, int OW, hipStream_t s) {
    const long total = planes * 4 * OH * OW;
    LP_LAUNCH(dilate2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, dy, z, total, OH, OW);
}

void launch_pool2(const float* g, float* gx, long planes, int H, int W, hipStream_t s) {
    const long total = planes * H * W;
    LP_LAUNCH(pool2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, g, gx, total, H, W);
}

// ====================================================================================== weight gradient
constexpr int WTH = 8, WTW = 16, WPIX = WTH * WTW;     // a tile is WTH x WTW output pixels
constexpr int WYS = WPIX + 1;                           // row stride of the staged dY block: 64 lanes, 64 banks
static_assert(LP_CONV_WGRAD_SLICE % WPIX == 0, "a slice is a whole number of tiles");

// input channels per workgroup and column blocks of 32 per wave: 4 waves x NCB x 32 columns >= CG * K * K
template <int K> struct WgCut;
template <> struct WgCut<3> { static constexpr int CG = 14, NCB = 1; };     // 126 of 128 columns
template <> struct WgCut<5> { static constexpr int CG = 10, NCB = 2; };     // 250 of 256
template <> struct WgCut<7> { static constexpr int CG = 10, NCB = 4; };     // 490 of 512

static int conv_wgrad_group(int K) { return K == 3 ? WgCut<3>::CG : K == 5 ? WgCut<5>::CG : WgCut<7>::CG; }

// grid (slices, ceil(Cout / 32), ceil((Ca + Cb) / CG)); H, W: the source plane, CH, CW = (H, W) << ups the convolved one
template <int K, int S>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ xa,
                                                         const float* __restrict__ xb, float* __restrict__ part, int N, int Ca,
                                                         int Cb, int Cout, int H, int W, int ups, int OH, int OW, int tilesX,
                                                         int tiles) {
    constexpr int CG = WgCut<K>::CG, NCB = WgCut<K>::NCB, KK = K * K;
    constexpr int PH = (WTH - 1) * S + K, PW = (WTW - 1) * S + K, PS = PH * PW;
    static_assert(4 * NCB * 32 >= CG * KK, "the four waves cover every column");
    __shared__ float xs[CG * PS];
    __shared__ float dys[32 * WYS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int half = lane >> 5, r = lane & 31;
    const int slice = blockIdx.x, co0 = blockIdx.y * 32, ci0 = blockIdx.z * CG;
    const int Ct = Ca + Cb, CH = H << ups, CW = W << ups;
    constexpr int UPS = LP_CONV_WGRAD_SLICE / WPIX;
    const int units = N * tiles;
    const int u0 = slice * UPS, u1 = min(u0 + UPS, units);
    // B: column (wave NCB + j) 32 + r = (channel of the group, tap); MFMA e reduces the pixels (e & 31) + 64 (e >> 5) of the
    // tile (half 0) and 32 further on, two tile rows below (half 1)
    const float* bp[NCB];
    bool cok[NCB];
    int ccol[NCB];
#pragma unroll
    for (int j = 0; j < NCB; ++j) {
        const int col = (wave * NCB + j) * 32 + r;
        cok[j] = col < CG * KK;
        ccol[j] = cok[j] ? col : 0;
        const int c = ccol[j] / KK, tap = ccol[j] - c * KK;
        bp[j] = xs + c * PS + (tap / K + 2 * half * S) * PW + tap % K;
    }
    const float* ap = dys + r * WYS + 32 * half;
    f32x16 acc[NCB];
#pragma unroll
    for (int j = 0; j < NCB; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;
    for (int u = u0; u < u1; ++u) {
        const int n = u / tiles, t = u - n * tiles;
        const int ty = t / tilesX, tx = t - ty * tilesX;
        const int oy0 = ty * WTH, ox0 = tx * WTW;
        const int iy0 = oy0 * S - K / 2, ix0 = ox0 * S - K / 2;
        for (int e = threadIdx.x; e < CG * PS; e += 256) {
            const int c = e / PS, q = e - c * PS;
            const int qy = q / PW, qx = q - qy * PW;
            const int gy = iy0 + qy, gx = ix0 + qx, ci = ci0 + c;
            const bool ok = ci < Ct && gy >= 0 && gy < CH && gx >= 0 && gx < CW;
            const bool fromb = ok && ci >= Ca;
            const float* src = fromb ? xb : xa;
            const long plane = fromb ? (long)n * Cb + (ci - Ca) : (long)n * Ca + ci;
            const float v = src[ok ? plane * H * W + (long)(gy >> ups) * W + (gx >> ups) : 0];
            xs[e] = ok ? v : 0.f;
        }
        for (int e = threadIdx.x; e < 32 * WPIX; e += 256) {
            const int row = e >> 7, p = e & 127;
            const int oy = oy0 + (p >> 4), ox = ox0 + (p & 15), co = co0 + row;
            const bool ok = co < Cout && oy < OH && ox < OW;
            const float v = dy[ok ? ((long)n * Cout + co) * OH * OW + (long)oy * OW + ox : 0];
            dys[row * WYS + p] = ok ? v : 0.f;
        }
        __syncthreads();
        // A pixel of the tile outside the plane contributes nothing, by selection: its staged dY is zero, but its B operand
        // is a real input cell wherever that cell lies in the plane, and 0 * NaN is a NaN.  The row limit of this lane's
        // half (zero for a column beyond the group) and the tile-uniform column limit:
        int ly[NCB];
#pragma unroll
        for (int j = 0; j < NCB; ++j) ly[j] = cok[j] ? OH - oy0 - 2 * half : 0;
        const int lx = OW - ox0;
#pragma unroll
        for (int e = 0; e < 64; ++e) {
            const int pix = (e & 31) + 64 * (e >> 5);              // + 32 half: in ap / bp
            const float a = ap[pix];
            const int boff = (pix >> 4) * S * PW + (pix & 15) * S;
#pragma unroll
            for (int j = 0; j < NCB; ++j) {
                const float b = bp[j][boff];
                const bool in = (pix >> 4) < ly[j] && (pix & 15) < lx;
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, in ? b : 0.f, acc[j], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    float* pa = part + (long)slice * Cout * Ct * KK;
    float* pb = pa + (long)Cout * Ca * KK;
#pragma unroll
    for (int j = 0; j < NCB; ++j) {
        const int c = ccol[j] / KK, tap = ccol[j] - c * KK, ci = ci0 + c;
        if (!cok[j] || ci >= Ct) continue;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int co = co0 + (i & 3) + 8 * (i >> 2) + 4 * half;
            if (co >= Cout) continue;
            if (ci < Ca) pa[((long)co * Ca + ci) * KK + tap] = acc[j][i];
            else pb[((long)co * Cb + (ci - Ca)) * KK + tap] = acc[j][i];
        }
    }
}

static int conv_tiles(int OH, int OW) { return ((OH + WTH - 1) / WTH) * ((OW + WTW - 1) / WTW); }

int conv_wgrad_slices(int N, int OH, int OW) {
    const long pixels = (long)N * conv_tiles(OH, OW) * WPIX;
    return (int)((pixels + LP_CONV_WGRAD_SLICE - 1) / LP_CONV_WGRAD_SLICE);
}

void launch_conv_wgrad(const float* dy, const float* xa, const float* xb, float* part, float* gwa, float* gwb, int N, int Ca,
                       int Cb, int Cout, int H, int W, int K, int S, int ups, hipStream_t s) {
    const int CH = H << ups, CW = W << ups;
    const int OH = (CH - 1) / S + 1, OW = (CW - 1) / S + 1;
    const int tilesX = (OW + WTW - 1) / WTW, tiles = conv_tiles(OH, OW);
    const int SL = conv_wgrad_slices(N, OH, OW), Ct = Ca + Cb, CG = conv_wgrad_group(K);
    dim3 grid(SL, (Cout + 31) / 32, (Ct + CG - 1) / CG), block(256);
#define LP_WG(KV, SV)                                                                                                    \
    LP_LAUNCH((conv_wgrad_kernel<KV, SV>), grid, block, 0, s, dy, xa, xb, part, N, Ca, Cb, Cout, H, W, ups, OH, OW, tilesX, \
              tiles)
    if (K == 7) { if (S == 1) LP_WG(7, 1); else LP_WG(7, 2); }
    else if (K == 5) { if (S == 1) LP_WG(5, 1); else LP_WG(5, 2); }
    else { if (S == 1) LP_WG(3, 1); else LP_WG(3, 2); }
#undef LP_WG
    const int stride = Cout * Ct * K * K, na = Cout * Ca * K * K;
    if (gwa) launch_slice_sum(part, SL, stride, na, gwa, s);
    if (Cb && gwb) launch_slice_sum(part + na, SL, stride, stride - na, gwb, s);
}

// ====================================================================================== bias gradient
constexpr long BIAS_CHUNK = 8192;           // values of a channel per workgroup

int conv_bias_slices(int N, int HW) {
    const long cnt = (long)N * HW;
    return (int)((cnt + BIAS_CHUNK - 1) / BIAS_CHUNK);
}

// grid (SB, Cout): the values g = n * HW + p in [s * BIAS_CHUNK, + BIAS_CHUNK) of channel c; thread t takes g = t mod 256
// in ascending order, then the 256 sums fold in halves
__global__ __launch_bounds__(256) void conv_bias_part_kernel(const float* __restrict__ dy, double* __restrict__ part, int N,
                                                             int Cout, int HW) {
    __shared__ double red[256];
    const int s = blockIdx.x, c = blockIdx.y, SB = gridDim.x;
    const long cnt = (long)N * HW, g0 = (long)s * BIAS_CHUNK, g1 = min(g0 + BIAS_CHUNK, cnt);
    double a = 0.0;
    for (long g = g0 + threadIdx.x; g < g1; g += 256) {
        const long n = g / HW, p = g - n * HW;
        a += (double)dy[(n * Cout + c) * HW + p];
    }
    red[threadIdx.x] = a;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[(long)c * SB + s] = red[0];
}

__global__ __launch_bounds__(256) void conv_bias_sum_kernel(const double* __restrict__ part, int SB, int Cout,
                                                            float* __restrict__ out) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= Cout) return;
    double a = 0.0;
    for (int i = 0; i < SB; ++i) a += part[(long)c * SB + i];
    out[c] = (float)a;
}

void launch_conv_bias_grad(const float* dy, double* part, float* gbias, int N, int Cout, int HW, hipStream_t s) {
    const int SB = conv_bias_slices(N, HW);
    LP_LAUNCH(conv_bias_part_kernel, dim3(SB, Cout), dim3(256), 0, s, dy, part, N, Cout, HW);
    LP_LAUNCH(conv_bias_sum_kernel, dim3((Cout + 255) / 256), dim3(256), 0, s, (const double*)part, SB, Cout, gbias);
}

}  // namespace lp
