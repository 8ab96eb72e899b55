// Whole InvBottlenecks (stride 1, 7x7) on a 16x16 plane, ONE workgroup per image for a RUN of consecutive blocks:
// stages 3-4 of LitePose at 256x256 input (lib/models/layers/layers.py:90-118).  The plane IS the tile, so there is
// no halo to recompute, and the 6x expanded tensor (288 / 480 channels) never leaves the CU:
//
//   x [Cin][256] --expand (bf16x3 MFMA)--> E chunk (32 ch, LDS) --dw7x7 (packed FMA, in place)--> D chunk
//     --project (bf16x3 MFMA, accumulated over the chunks in registers)--> + bias (+ x) --> out [Cout][256]
//
// mb16_kernel: 512 threads = 8 waves in lock-step phases, two workgroup barriers per chunk.
//   * wave w owns pixel tile w (rows 2w, 2w+1: 32 pixels = one MFMA column block) for both 1x1
//     convolutions, and channel pairs 2w, 2w+1 of every 32-channel chunk for the depthwise
//   * the block input is split ONCE into exact bf16x3 B fragments that stay in registers for all chunks
//     (pw3_kernel re-split it once per consuming channel block: 7.4 k VALU per wave)
//   * E chunk = [16 pairs][22 rows][22 cells][2 ch] fp32: a zero frame of 3 rows / 3+3 columns written
//     once; the right halo of row r and the left halo of row r+1 are the same six cells, so a row costs
//     22 cells and the odd row stride (11 sixteen-byte slots) keeps every ds_read_b128 lane group of the
//     quad->row table on 16 distinct slots
//   * the depthwise writes its result over its own input (a pair is read and written by one wave only,
//     LDS operations of a wave execute in order), so D needs no second buffer, and the cells wave w
//     reads for the project are exactly the cells it overwrites with the next chunk's expand
//   * everything a chunk needs besides x -- the A fragments of its two 1x1 slices, the expand bias and the
//     49 x 2 depthwise taps (+ bias) of its 16 pairs -- is fetched ONCE per workgroup: LDS-DMA issued at
//     the top of the depthwise phase, landed when the barrier that ends it is passed
//   * arithmetic is bit-identical to pw3_kernel -> dw_pair16_kernel -> pw3_kernel (same fragment layouts,
//     same six-product order per k-step, same tap order), which the parity tests use
//
// Round 4: a RUN of blocks per launch.  The residual blocks of a stage (XS: stage.2.1-9, 48 -> 288 -> 48, and
// stage.3.1-9, 80 -> 480 -> 80) have one shape, and the output of a block in this kernel's register layout is one
// v_permlane32_swap away from the next block's input fragments: the D fragment of the project holds channels
// 8q + 4*half + 0..3 of the lane's pixel, the B fragment of the next expand wants channels 16ks + 8*half + 0..7, and
// swap(registers of q = 2ks | registers of q = 2ks + 1) between the wave halves is exactly that regrouping.  The
// residual x is rebuilt from the three bf16 pieces the lane already holds (the split is exact: h + m + l == x), so a
// block boundary inside a run is: + bias, swap, + x, store (block outputs stay tappable and feed the deconv head),
// split -- ~110 VALU per 16 channels -- instead of a kernel boundary with an 80 KB strided reload, a zeroed tile, an
// exposed first weight transfer and the tail of the slowest workgroup (profiles/r04_mb16_ablation.txt: 14.5 us of an
// 83 us block).  Same adds in the same order as the one-block form: the outputs of every block are bit-identical.
//
// What was tried and removed: an antiphase form (round 2; packed FMAs and MFMAs do not overlap on a SIMD), two
// workgroups per image with a partial-sum exchange (round 3: +44 % CU time), and mb16p_kernel (round 4: matrix work
// and depthwise of different half-chunks in one barrier phase; bit-identical, 25 % slower -- an MFMA parks its wave
// for 32 cycles and a lone wave issues one VALU instruction per ~5 cycles, so at two waves per SIMD there is no idle
// issue slot to win; profiles/r04_phase_mix.txt).
#include "kernels.h"
#include "fused_common.h"
#include "dw7.h"
#include "split3.h"

#include <cstdlib>

namespace lp {

constexpr int M16_RS = 22;                               // cells per tile row
constexpr int M16_PAIR = 22 * M16_RS * 2 + 4;            // floats per channel pair: 968 + one zero 16-byte slot, so that
                                                         // consecutive pairs start an ODD number of slots apart (see the
                                                         // depthwise lane mapping)
constexpr int M16_LDS_FLOATS = 16 * M16_PAIR + 8;        // + the two cells strip 3 reads past the last row
// weight stage behind the E chunk (fused_common.h): bf16x3 pieces, 512 threads
template <int CK, int NMT> using M16W = StageLayout<CK, NMT, 3, 512, (size_t)M16_LDS_FLOATS * 4>;

// bf16 piece (low / high half of a dword) -> the fp32 value it stands for
__device__ __forceinline__ float bf_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }

template <int CK, int NMT, bool RES>
__global__ __launch_bounds__(512, 2) void mb16_kernel(
    const float* __restrict__ x,        // [N, Cin, 256]: input of the first block
    const Mb16Run run,                  // per block: bf16x3 A fragments, biases, filter rows, output (kernels.h)
    int Cexp, int Cout) {
    extern __shared__ __attribute__((aligned(16))) float E[];
    LP_OWN_CU();                                                      // kernels.h
    constexpr int Cin = CK * 16;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int half = lane >> 5, pl = lane & 31;
    const int n = blockIdx.x;
    const int px = wave * 32 + pl;                                   // this lane's MFMA column
    const int cell = (((px >> 4) + 3) * M16_RS + (px & 15) + 4) * 2; // its cell in a pair plane (floats)
    const int nchunks = Cexp >> 5, KS2 = Cexp >> 4;
    const int nblocks = RES ? run.nblocks : 1;                       // a run is residual blocks of one shape
    const int gtotal = nblocks * nchunks;                            // chunks of the whole run
    using WG = M16W<CK, NMT>;
    u32x4* W1 = reinterpret_cast<u32x4*>(E + M16_LDS_FLOATS);         // [CK][3][64]
    u32x4* W2 = W1 + WG::N1;                                          // [NMT][2][3][64]
    u32x4* WD = W2 + WG::N2 + WG::N3;                                 // [2 chunk parities][16 pairs][28]

    // weight stage (fused_common.h: layout, protocol, LP_STAGE_*) with this kernel's own chunk map -- the standard one with
    // g counting the chunks of the whole run, so that the first chunk of the next block is staged under the last depthwise of
    // this one -- and its own copy of the two loops (stage_load = stage_issue, stage_store = stage_land): the CK = 6 variant
    // sits at the register budget, and its code depends on how deep these lambdas nest.  Calling the shared loops, or
    // writing stage_load's loop into stage_now, gives <6, 3, *> another register allocation (235 -> 234, waits moved).
    constexpr bool PIPE = CK < 6;                                    // (the 96-channel variant sits at the register budget)
    u32x4 stg[WG::NLD];
    auto stage_addr = [&](int g, int j, const u32x4*& src, u32x4*& dst) -> bool {
        const int e0 = 64 * wave + 512 * j;                          // wave-uniform
        if (e0 >= WG::NTOT) return false;
        const int ga = max(g, 0), gb = min(g + 1, gtotal - 1), dpar = (g + 1) & 1;
        const int ba = ga / nchunks, ca = ga - ba * nchunks;         // block / chunk of the project slice
        const int bb = gb / nchunks, cb = gb - bb * nchunks;         // block / chunk of everything else
        dst = W1 + e0;
        if (e0 < WG::N1) src = reinterpret_cast<const u32x4*>(run.w1s[bb]) + (long)cb * WG::N1 + e0 + lane;
        else if (e0 < WG::N1 + WG::N2) {
            const int f0 = e0 - WG::N1, seg = f0 / 192, within = f0 - seg * 192;
            src = reinterpret_cast<const u32x4*>(run.w2s[ba]) + ((long)(seg >> 1) * KS2 + 2 * ca + (seg & 1)) * 192 + within + lane;
        } else if (e0 < WG::N1 + WG::N2 + WG::N3) {
            src = reinterpret_cast<const u32x4*>(run.b1f[bb]) + (long)cb * 8 + min(lane, 7);
        } else {
            src = reinterpret_cast<const u32x4*>(run.wrow[bb]) + (long)cb * WG::N4 + (e0 - WG::N1 - WG::N2 - WG::N3) + lane;
            dst += dpar * WG::N4;
        }
        return true;
    };
    auto stage_load = [&](int g) {
#pragma unroll
        for (int j = 0; j < WG::NLD; ++j) {
            const u32x4* src;
            u32x4* dst;
            if (stage_addr(g, j, src, dst)) LP_STAGE_LOAD(stg[j], src, dst);
        }
    };
    auto stage_store = [&](int g) {
#pragma unroll
        for (int j = 0; j < WG::NLD; ++j) {
            const u32x4* src;
            u32x4* dst;
            if (stage_addr(g, j, src, dst)) LP_STAGE_STORE(stg[j], dst, lane);
        }
        LP_STAGE_DRAIN();
    };
    auto stage_now = [&](int g) {                                    // !PIPE: every transfer written as soon as it has arrived
#ifndef LP_NO_LDS_DMA
        stage_load(g);
#else
#pragma unroll
        for (int j = 0; j < WG::NLD; ++j) {
            const u32x4* src;
            u32x4* dst;
            if (stage_addr(g, j, src, dst)) {
                const u32x4 t = *src;
                asm volatile("" ::: "memory");                       // one transfer at a time: 4 registers, not 4 NLD
                dst[lane] = t;
            }
        }
#endif
    };
    stage_load(-1);

    // ---- zero frame (and everything else) once ----------------------------------------------
    for (int i = threadIdx.x; i < M16_LDS_FLOATS / 4; i += 512)
        reinterpret_cast<f32x4*>(E)[i] = f32x4{0.f, 0.f, 0.f, 0.f};

    // ---- block input -> bf16x3 B fragments: channels 16ks + 8*half + 0..7 of pixel px ---------
    u32x4 xh[CK], xm[CK], xl[CK];
    {
        const float* xp = x + ((long)n * Cin + 8 * half) * 256 + px;
#pragma unroll
        for (int ks = 0; ks < CK; ++ks) {
            float v[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) v[c] = xp[(ks * 16 + c) * 256];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const Split3 p3 = split3_pair(v[2 * j], v[2 * j + 1]);
                xh[ks][j] = p3.h; xm[ks][j] = p3.m; xl[ks][j] = p3.l;
            }
        }
    }
    f32x16 acc[NMT];
#pragma unroll
    for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][r] = 0.f;

    // depthwise geometry: quad -> (pair of the wave, row pair), see the depthwise phase
    const int dwq = lane >> 2, strip = lane & 3;
    const int dwpair = (dwq >> 2) & 1;
    const int dwrp = (int)((0x7623673254014510ull >> (4 * dwq)) & 15);
    const int dwoff = (2 * dwrp * M16_RS + strip * 4) * 2;           // first cell this lane reads (input row R = 0)
    const int dwout = ((2 * dwrp + 3) * M16_RS + 4 + strip * 4) * 2; // its 2 x 4 output cells (second row: + M16_RS*2)

    stage_store(-1);                                                 // the first stage
    __syncthreads();
    int blk = 0, ch = 0;                                             // block of the run, chunk of the block
    for (int g = 0; g < gtotal; ++g) {
        // ================= expand: E[32 ch][this wave's 32 px] = relu6(W1[chunk] . x + b1) =========
        {
            f32x16 d;
#pragma unroll
            for (int r = 0; r < 16; ++r) d[r] = 0.f;
            const u32x4* wl = W1 + lane;
#pragma unroll
            for (int ks = 0; ks < CK; ++ks) {
                u32x4 a[3];
#pragma unroll
                for (int t = 0; t < 3; ++t) a[t] = wl[(ks * 3 + t) * 64];
                d = mma6(a, xh[ks], xm[ks], xl[ks], d);
            }
            const f32x4* bp = reinterpret_cast<const f32x4*>(W2 + WG::N2) + half * 4;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 bq = bp[q];
#pragma unroll
                for (int e = 0; e < 4; e += 2) {                     // registers 4q+e, 4q+e+1 = channels cc, cc+1
                    const int cc = 4 * half + e + 8 * q;
                    const f32x2 pv = {fminf(fmaxf(d[4 * q + e] + bq[e], 0.f), 6.f),
                                      fminf(fmaxf(d[4 * q + e + 1] + bq[e + 1], 0.f), 6.f)};
                    *reinterpret_cast<f32x2*>(E + (cc >> 1) * M16_PAIR + cell) = pv;
                }
            }
        }
        __syncthreads();
        // weights of the next two 1x1 slices (this chunk's project, the next chunk's expand): requested
        // now, parked in LDS after the depthwise (nobody reads the stage between the two barriers)
        if constexpr (PIPE) stage_load(g);
        else stage_now(g);                                           // CK = 6: no room for staging registers across the depthwise
        // ================= depthwise 7x7 + bias + relu6, in place: pairs 2w, 2w+1 in ONE pass ========
        // The depthwise is bound by LDS read bandwidth (tools/ubench, profiles/README.md: 42 x 1 KB of
        // ds_read_b128 per 196 packed FMAs when a lane owns 4 outputs of one row), so a lane owns a 2 x 4
        // output block instead: input rows 2rp .. 2rp+7 are read once and feed both output rows (48 reads per
        // 392 FMAs), and one filter-row read serves two output rows.  The wave covers both of its pairs at
        // once: quad q = lane >> 2 -> pair (q >> 2) & 1, row pair dwrp (table below), strip = lane & 3.  The
        // table puts row pairs {g, g+4} of pair A and of pair B into each ds_read_b128 lane group
        // ({q0,q3,q5,q6}, {q1,q2,q4,q7}, ...): with 11 slots per row and 243 per pair their four strips land
        // on 16 distinct 16-byte slots.  Tap order per output is unchanged (ky ascending, kx inside).
        {
            const int kp = wave * 2 + dwpair;
            const f32x4* wl = reinterpret_cast<const f32x4*>(WD + (g & 1) * WG::N4) + kp * 28;
            float* ep = E + kp * M16_PAIR;
            f32x2 a0[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};   // output row 2rp
            f32x2 a1[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};   // output row 2rp + 1
            dw7_s1_2x4<M16_RS * 2>(ep + dwoff, wl, a0, a1);          // dw7.h: LDS requests pinned ahead of the FMAs
            const f32x4 wbias = wl[3];                               // the pair's bias rides in the pad of filter row 0
            const float b0 = wbias[2], b1 = wbias[3];
            f32x4 o00, o01, o10, o11;
            o00[0] = fminf(fmaxf(a0[0][0] + b0, 0.f), 6.f); o00[1] = fminf(fmaxf(a0[0][1] + b1, 0.f), 6.f);
            o00[2] = fminf(fmaxf(a0[1][0] + b0, 0.f), 6.f); o00[3] = fminf(fmaxf(a0[1][1] + b1, 0.f), 6.f);
            o01[0] = fminf(fmaxf(a0[2][0] + b0, 0.f), 6.f); o01[1] = fminf(fmaxf(a0[2][1] + b1, 0.f), 6.f);
            o01[2] = fminf(fmaxf(a0[3][0] + b0, 0.f), 6.f); o01[3] = fminf(fmaxf(a0[3][1] + b1, 0.f), 6.f);
            o10[0] = fminf(fmaxf(a1[0][0] + b0, 0.f), 6.f); o10[1] = fminf(fmaxf(a1[0][1] + b1, 0.f), 6.f);
            o10[2] = fminf(fmaxf(a1[1][0] + b0, 0.f), 6.f); o10[3] = fminf(fmaxf(a1[1][1] + b1, 0.f), 6.f);
            o11[0] = fminf(fmaxf(a1[2][0] + b0, 0.f), 6.f); o11[1] = fminf(fmaxf(a1[2][1] + b1, 0.f), 6.f);
            o11[2] = fminf(fmaxf(a1[3][0] + b0, 0.f), 6.f); o11[3] = fminf(fmaxf(a1[3][1] + b1, 0.f), 6.f);
            // every lane's reads of both pairs precede these writes (one wave, in-order LDS queue)
            *reinterpret_cast<f32x4*>(ep + dwout) = o00;
            *reinterpret_cast<f32x4*>(ep + dwout + 4) = o01;
            *reinterpret_cast<f32x4*>(ep + dwout + M16_RS * 2) = o10;
            *reinterpret_cast<f32x4*>(ep + dwout + M16_RS * 2 + 4) = o11;
        }
        if constexpr (PIPE) stage_store(g);                          // the staged weights, in front of the barrier that
        else LP_STAGE_DRAIN();
        __syncthreads();                                             // publishes them together with the depthwise result
        // ================= project: acc += W2[:, chunk] . D[chunk][this wave's 32 px] ================
#pragma unroll
        for (int ks2 = 0; ks2 < 2; ++ks2) {
            u32x4 fh, fm, fl;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x2 v = *reinterpret_cast<const f32x2*>(E + (8 * ks2 + 4 * half + j) * M16_PAIR + cell);
                const Split3 p3 = split3_pair(v[0], v[1]);
                fh[j] = p3.h; fm[j] = p3.m; fl[j] = p3.l;
            }
#pragma unroll
            for (int mt = 0; mt < NMT; ++mt) {
                const u32x4* wl = W2 + (mt * 2 + ks2) * 3 * 64 + lane;
                u32x4 a[3];
#pragma unroll
                for (int t = 0; t < 3; ++t) a[t] = wl[t * 64];
                acc[mt] = mma6(a, fh, fm, fl, acc[mt]);
            }
        }
        // no barrier: the cells read above are the cells this wave overwrites in the next expand
        if (++ch < nchunks) continue;
        ch = 0;
        // ================= end of a block ============================================================
        float* ob = run.out[blk] + (long)n * Cout * 256 + px;
        const float* b2f = run.b2f[blk];
        if constexpr (!RES) {
            // + bias, 128-byte rows per half-wave (a block that changes the channel count ends its launch)
#pragma unroll
            for (int mt = 0; mt < NMT; ++mt) {
                const f32x4* bp = reinterpret_cast<const f32x4*>(b2f + (mt * 2 + half) * 16);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (mt * 32 + 8 * q >= Cout) break;              // wave-uniform: Cout is a multiple of 8
                    const f32x4 bq = bp[q];
#pragma unroll
                    for (int e = 0; e < 4; ++e) ob[(mt * 32 + 4 * half + e + 8 * q) * 256] = acc[mt][4 * q + e] + bq[e];
                }
            }
        } else {
            // + bias in the D-fragment layout, regroup to the B-fragment channels (16ks + 8*half + 0..7) with one
            // v_permlane32_swap per register pair, + x (rebuilt from its exact bf16 pieces), store, and -- when
            // another block follows -- split the sum into the next block's input fragments.  Cin == Cout == 16 CK.
            const bool more = blk + 1 < nblocks;
#pragma unroll
            for (int ks = 0; ks < CK; ++ks) {
                const int mt = ks >> 1, qa = 2 * (ks & 1), qb = qa + 1;
                const f32x4 ba = reinterpret_cast<const f32x4*>(b2f + (mt * 2 + half) * 16)[qa];
                const f32x4 bb = reinterpret_cast<const f32x4*>(b2f + (mt * 2 + half) * 16)[qb];
                float y[8];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float va = acc[mt][4 * qa + e] + ba[e];    // channel 16ks + 4*half + e
                    const float vb = acc[mt][4 * qb + e] + bb[e];    // channel 16ks + 8 + 4*half + e
                    // upper half of va <-> lower half of vb: lanes 0-31 get (own a | upper a) = channels 16ks + 0..7,
                    // lanes 32-63 (lower b | own b) = channels 16ks + 8 + 0..7
                    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(va), __float_as_uint(vb), false, false);
                    y[e] = __uint_as_float(sw[0]);
                    y[4 + e] = __uint_as_float(sw[1]);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float x0 = (bf_lo(xh[ks][j]) + bf_lo(xm[ks][j])) + bf_lo(xl[ks][j]);   // exact: h + m + l == x
                    const float x1 = (bf_hi(xh[ks][j]) + bf_hi(xm[ks][j])) + bf_hi(xl[ks][j]);
                    const float o0 = y[2 * j] + x0, o1 = y[2 * j + 1] + x1;
                    ob[(ks * 16 + 8 * half + 2 * j) * 256] = o0;
                    ob[(ks * 16 + 8 * half + 2 * j + 1) * 256] = o1;
                    if (more) {
                        const Split3 p3 = split3_pair(o0, o1);
                        xh[ks][j] = p3.h; xm[ks][j] = p3.m; xl[ks][j] = p3.l;
                    }
                }
            }
            if (more) {
#pragma unroll
                for (int mt = 0; mt < NMT; ++mt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[mt][r] = 0.f;
            }
        }
        ++blk;
    }
}

bool uses_scratch(const void* kernel_fn) {
    // tiny cache: the set of kernel variants is small and fixed; queried on eager / capture launches only
    static thread_local const void* seen[256];
    static thread_local bool val[256];
    static thread_local int nseen = 0;
    for (int i = 0; i < nseen; ++i)
        if (seen[i] == kernel_fn) return val[i];
    hipFuncAttributes at;
    bool r = false;
    if (hipFuncGetAttributes(&at, kernel_fn) == hipSuccess) r = at.localSizeBytes > 0;
    else (void)hipGetLastError();
    if (nseen < 256) { seen[nseen] = kernel_fn; val[nseen] = r; ++nseen; }
    return r;
}

bool kernel_allow_lds(const void* kernel_fn, size_t dyn_lds) {
    // the same kind of cache, keyed by (device, kernel): the largest limit the runtime granted and the smallest it
    // refused, so that neither is asked for twice
    struct Entry { const void* fn; int dev; size_t granted, refused; };
    static thread_local Entry tab[512];
    static thread_local int ntab = 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return false; }
    Entry* e = nullptr;
    for (int i = 0; i < ntab && !e; ++i)
        if (tab[i].fn == kernel_fn && tab[i].dev == dev) e = &tab[i];
    if (e && dyn_lds <= e->granted) return true;
    if (e && e->refused && dyn_lds >= e->refused) return false;
    const bool ok = hipFuncSetAttribute(kernel_fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn_lds) == hipSuccess;
    if (!ok) (void)hipGetLastError();
    if (!e && ntab < 512) { e = &tab[ntab++]; *e = Entry{kernel_fn, dev, 0, 0}; }
    if (e) (ok ? e->granted : e->refused) = dyn_lds;
    return ok;
}

bool kernel_ready(const void* kernel_fn, size_t dyn_lds) {
    return !uses_scratch(kernel_fn) && kernel_allow_lds(kernel_fn, dyn_lds);
}

template <int CK, int NMT>
static bool launch_mb16_t(const float* x, const Mb16Run& run, bool res, int N, int Cexp, int Cout, hipStream_t s) {
    const size_t lds = M16W<CK, NMT>::LDS_BYTES;
    if (!kernel_ready(res ? (const void*)mb16_kernel<CK, NMT, true> : (const void*)mb16_kernel<CK, NMT, false>, lds))
        return false;
    if (res) LP_LAUNCH((mb16_kernel<CK, NMT, true>), dim3(N), dim3(512), lds, s, x, run, Cexp, Cout);
    else LP_LAUNCH((mb16_kernel<CK, NMT, false>), dim3(N), dim3(512), lds, s, x, run, Cexp, Cout);
    return true;
}

bool mb16_supported(int Cin, int Cexp, int Cout, int H, int W, int K, int S, bool res) {
    if (H != 16 || W != 16 || K != 7 || S != 1) return false;
    if ((Cout & 7) || (res && Cin != Cout) || (Cin & 15) || (Cexp & 31)) return false;
    const int nmt = (Cout + 31) >> 5, ck = Cin >> 4;
#define LP_GO(CKV, NMTV)                                                                                     \
    if (ck == CKV && nmt == NMTV)                                                                            \
        return !uses_scratch(res ? (const void*)mb16_kernel<CKV, NMTV, true> : (const void*)mb16_kernel<CKV, NMTV, false>);
    LP_GO(3, 2) LP_GO(3, 3) LP_GO(3, 4) LP_GO(5, 3) LP_GO(6, 3)
#undef LP_GO
    return false;
}

bool launch_mb16(const float* x, const Mb16Run& run, bool res, int N, int Cin, int Cexp, int Cout, int H, int W,
                 int K, int S, hipStream_t s) {
    if (run.nblocks < 1 || run.nblocks > MB16_MAX_RUN || (!res && run.nblocks != 1)) return false;
    if (!mb16_supported(Cin, Cexp, Cout, H, W, K, S, res)) return false;
    for (int b = 0; b < run.nblocks; ++b)
        if (!run.w1s[b] || !run.b1f[b] || !run.wrow[b] || !run.w2s[b] || !run.b2f[b] || !run.out[b]) return false;
    const int nmt = (Cout + 31) >> 5, ck = Cin >> 4;
    last_kernel_tag = "mb16_kernel";
#define LP_GO(CKV, NMTV) \
    if (ck == CKV && nmt == NMTV) return launch_mb16_t<CKV, NMTV>(x, run, res, N, Cexp, Cout, s);
    LP_GO(3, 2) LP_GO(3, 3) LP_GO(3, 4) LP_GO(5, 3) LP_GO(6, 3)
#undef LP_GO
    return false;
}

}  // namespace lp
