// Device-side pieces the tiled and fused kernels share: the XCD-contiguous workgroup order and the weight stage of the
// fused blocks (its layout, its chunk map and its two loops).  Constants and inline functions; every kernel stays in its
// own file.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "split3.h"                                       // u32x4

namespace lp {

// Workgroups are dealt to the 8 XCDs round-robin (id % 8) and every XCD has its own L2.  Tile kernels
// whose neighbouring tiles share halo rows / cache lines therefore remap the hardware id so that
// CONSECUTIVE logical tiles run on the SAME XCD (ids 8 apart, dispatched back to back) and their shared
// lines are L2 hits instead of a second fabric fetch.  Bijection on [0, n).
__device__ __forceinline__ int xcd_contiguous_id(int id, int n) {
    const int q = n >> 3, r = n & 7;
    const int xcd = id & 7, slot = id >> 3;
    return xcd * q + min(xcd, r) + slot;
}

// =====================================================================================
// Weight stage of a fused block kernel (mb16_kernel, mbt_kernel tile / strip, mbt_s2_kernel, mbtb_kernel, mbtb_s2_kernel,
// mbtd_kernel): everything a chunk of 32 expanded channels needs besides x is fetched ONCE per workgroup, 16 bytes per lane
// and transfer, global memory -> LDS.
//
// Layout, behind the kernel's activation tile of TILE_BYTES, in u32x4 elements (one per lane and transfer):
//   N1  the expand's A fragments: CK k-steps of 16 input channels x PIECES x 64 lanes (PIECES = 3: the exact bf16x3
//       split of fp32 weights; 1: bf16 / fp16 weights)
//   N2  the project's: NMT blocks of 32 filters x 2 k-steps x PIECES x 64 lanes
//   N3  the expand bias of the chunk (8 records used)
//   N4  the depthwise filter rows of the chunk's 16 pairs [16][7 rows][7 taps x 2 ch, bias pair in row 0's pad],
//       double-buffered by chunk parity (hence NTOT + N4 in LDS_BYTES)
// NTOT is what one staging pass moves, NLD the transfers per lane of a workgroup of THREADS.
//
// Who moves what: transfer j of wave w is elements [64 w + THREADS j, + 64) of the pass.  N1, N2, N3 and N4 are whole
// numbers of 64-element transfers, so a transfer never straddles two regions: its region -- and with it the source array
// and the chunk -- is wave-uniform, and only `+ lane` differs between the lanes.
//
// What a pass holds (stage_chunk_addr): issued in chunk c it is [expand slice of chunk c+1 | project slice of chunk c |
// expand bias of chunk c+1 | depthwise rows of chunk c+1 -> buffer (c+1) & 1]; pass -1 in the prologue brings chunk 0.
//
// Where the two halves sit: stage_issue(c) directly BEHIND the barrier that ends the expand of chunk c, at the top of its
// depthwise phase -- every wave is past the expand of c and the project of c-1, which read N1 / N3 / N2, and the
// depthwise in flight reads the OTHER N4 buffer, so nobody reads what the pass overwrites.  stage_land(c) directly IN
// FRONT of the barrier that ends the depthwise, which publishes the pass together with the depthwise result to the
// project of c and the expand of c+1.  Nothing may read the stage between the two.
//
// Default: LDS-DMA (global_load_lds_dwordx4: no staging registers, no ds_write pass; stage_land only drains vmcnt).
// -DLP_NO_LDS_DMA (the `regstage` flavour, python -m litepose_amd.build --flavour regstage): the same bytes through NLD
// staging registers per lane, loaded by stage_issue and written by stage_land -- built while round 4 suspected LDS-DMA of
// the rare wrong batch (it was the packed-fp32 op_sel erratum), kept because it is the A/B that cleared the
// instruction: mb16_kernel 1.15 -> 1.25 ms per forward of XS@256, bit-identical.
// =====================================================================================
#ifndef LP_NO_LDS_DMA
#define LP_STAGE_LOAD(reg, src, dst)                                                                  \
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src),           \
                                     (__attribute__((address_space(3))) void*)(dst), 16, 0, 0)
#define LP_STAGE_STORE(reg, dst, lane) ((void)0)
#define LP_STAGE_DRAIN() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#else
#define LP_STAGE_LOAD(reg, src, dst) ((reg) = *(src))
#define LP_STAGE_STORE(reg, dst, lane) ((dst)[lane] = (reg))
#define LP_STAGE_DRAIN() ((void)0)
#endif

template <int CK, int NMT, int PIECES_, int THREADS_, size_t TILE_BYTES> struct StageLayout {
    static constexpr int PIECES = PIECES_, THREADS = THREADS_;
    static constexpr int N1 = CK * PIECES * 64, N2 = NMT * 2 * PIECES * 64, N3 = 64, N4 = 16 * 28;
    static constexpr int NTOT = N1 + N2 + N3 + N4;
    static constexpr int NLD = (NTOT + THREADS - 1) / THREADS;
    static constexpr size_t LDS_BYTES = TILE_BYTES + (size_t)(NTOT + N4) * 16;
};

// The standard chunk map: source and destination of transfer j of this wave in the pass issued in chunk c, false when the
// pass has no such transfer.  W1 is the stage's first element in LDS; w1s / w2s / b1f / wrow are the packed arrays of the
// block ([chunk][N1], [filter block][KS2 k-steps][PIECES][64], [chunk][32 fp32], [chunk][N4]).  RAGGED: the expanded
// width may end in a half chunk (16-bit kernels), whose second project k-step does not exist and is never used.
template <class L, bool RAGGED>
__device__ __forceinline__ bool stage_chunk_addr(int wave, int lane, int j, int c, int nchunks, int KS2, const u32x4* w1s,
                                                 const u32x4* w2s, const float* b1f, const void* wrow, u32x4* W1,
                                                 const u32x4*& src, u32x4*& dst) {
    constexpr int SEG = 64 * L::PIECES;                              // one k-step of one filter block
    const int e0 = 64 * wave + L::THREADS * j;                       // wave-uniform
    if (e0 >= L::NTOT) return false;
    const int ca = max(c, 0), cb = min(c + 1, nchunks - 1), dpar = (c + 1) & 1;
    dst = W1 + e0;
    if (e0 < L::N1) src = w1s + (long)cb * L::N1 + e0 + lane;
    else if (e0 < L::N1 + L::N2) {
        const int f0 = e0 - L::N1, seg = f0 / SEG, within = f0 - seg * SEG;
        if constexpr (RAGGED) {
            const int ks = min(2 * ca + (seg & 1), KS2 - 1);
            src = w2s + ((long)(seg >> 1) * KS2 + ks) * SEG + within + lane;
        } else {
            src = w2s + ((long)(seg >> 1) * KS2 + 2 * ca + (seg & 1)) * SEG + within + lane;
        }
    } else if (e0 < L::N1 + L::N2 + L::N3) {
        src = reinterpret_cast<const u32x4*>(b1f) + (long)cb * 8 + min(lane, 7);
    } else {
        src = static_cast<const u32x4*>(wrow) + (long)cb * L::N4 + (e0 - L::N1 - L::N2 - L::N3) + lane;
        dst += dpar * L::N4;
    }
    return true;
}

// The two halves of a pass.  addr(c, j, src, dst) is the kernel's chunk map (stage_chunk_addr, or its own); stg are the
// staging registers of the regstage flavour (unused, and gone, with LDS-DMA).  Two kernels at the register budget
// (mbt_s2_kernel, mb16_kernel at CK = 6) have no room for them across the depthwise: there the regstage flavour writes
// every transfer to LDS as soon as it has arrived, in the place of stage_issue, and LP_STAGE_DRAIN() alone takes the place
// of stage_land.  mb16_kernel keeps its own copy of both loops (see there).
template <class L, class Addr>
__device__ __forceinline__ void stage_issue(u32x4 (&stg)[L::NLD], int c, const Addr& addr) {
#pragma unroll
    for (int j = 0; j < L::NLD; ++j) {
        const u32x4* src;
        u32x4* dst;
        if (addr(c, j, src, dst)) LP_STAGE_LOAD(stg[j], src, dst);
    }
}
template <class L, class Addr>
__device__ __forceinline__ void stage_land(u32x4 (&stg)[L::NLD], int c, int lane, const Addr& addr) {
#pragma unroll
    for (int j = 0; j < L::NLD; ++j) {
        const u32x4* src;
        u32x4* dst;
        if (addr(c, j, src, dst)) LP_STAGE_STORE(stg[j], dst, lane);
    }
    LP_STAGE_DRAIN();
}

}  // namespace lp
