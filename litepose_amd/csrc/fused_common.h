// Device-side pieces the tiled and fused kernels share: the XCD-contiguous workgroup order and the layout of the weight
// stage of the fused blocks.  Constants and one inline function; every kernel stays in its own file.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

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

// Weight stage of a fused block kernel, behind its activation tile of TILE_BYTES: what one chunk of 32 expanded channels
// needs besides x, in u32x4 elements (one per lane and transfer) --
//   N1  the expand's A fragments: CK k-steps of 16 input channels x PIECES x 64 lanes (PIECES = 3: the exact bf16x3
//       split of fp32 weights; 1: bf16 / fp16 weights)
//   N2  the project's: NMT blocks of 32 filters x 2 k-steps x PIECES x 64 lanes
//   N3  the expand bias of the chunk (8 used; every region is a whole number of waves)
//   N4  the depthwise filter rows of the chunk's 16 pairs [16][7 rows][7 taps x 2 ch, bias pair in row 0's pad],
//       double-buffered by chunk parity (hence NTOT + N4 in LDS_BYTES)
// NTOT is what one staging pass moves, NLD the transfers per lane of a workgroup of THREADS.
template <int CK, int NMT, int PIECES, int THREADS, size_t TILE_BYTES> struct StageLayout {
    static constexpr int N1 = CK * PIECES * 64, N2 = NMT * 2 * PIECES * 64, N3 = 64, N4 = 16 * 28;
    static constexpr int NTOT = N1 + N2 + N3 + N4;
    static constexpr int NLD = (NTOT + THREADS - 1) / THREADS;
    static constexpr size_t LDS_BYTES = TILE_BYTES + (size_t)(NTOT + N4) * 16;
};

}  // namespace lp
