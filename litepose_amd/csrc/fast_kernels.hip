// gfx950 kernels of the reference's real-time parser (nano_demo/fast_utils/parse): find_peaks.cpp -> fast_peaks_kernel,
// assign.cpp -> fast_assign_kernel (its arithmetic lives in fast_assign.h, shared with the host build of the tests).
// Compiled with -ffp-contract=off: every fp operation rounds like the reference's compiled C++.
#include "fast_assign.h"
#include "kernels.h"

namespace lp {

namespace {
constexpr int FP_THREADS = 256;
constexpr int FP_WAVES = FP_THREADS / 64;
constexpr int FP_BAND_FLOATS = 12288;     // 48 KB: the rows of one band with their halo (W <= 1024: at least 12 rows)
constexpr int FP_MAX_ENTRIES = 1024;      // 8 KB: one 64-bit ballot per (row, 64-column segment) of a band
}  // namespace

// find_peaks_out_hw (find_peaks.cpp:9-56) for one (image, joint) plane per workgroup.  The plane is walked in bands of R
// rows, staged in LDS with a halo of win rows on either side (rows outside the plane are never read: the window is
// clamped to it, :29-32).  Inside a band each wave takes a run of rows and, per 64-column segment, ballots
//   peak(y, x) = !(v < threshold) && no cell of the clamped window is > v        (:25, :38 -- a NaN is a peak, as there)
// into masks[row][segment].  Raster order is the order of that table, so the k-th peak of the plane is found without any
// atomic: wave 0 scans the popcounts of 64 entries at a time (prefix over entries = over segments, rows and waves) and
// each lane emits the bits of its mask (prefix over the lane mask) while the slot is below M.  The walk stops with the
// band in which the M-th peak was found, like the reference's `cnt < M` loops.
__global__ __launch_bounds__(FP_THREADS) void fast_peaks_kernel(
    const float* __restrict__ det, const float* __restrict__ tmap, long tstride, int H, int W, float threshold, int win,
    int M, int R, int* __restrict__ count, float* __restrict__ val, float* __restrict__ tag, int* __restrict__ ind) {
    __shared__ float band[FP_BAND_FLOATS];
    __shared__ unsigned long long masks[FP_MAX_ENTRIES];
    __shared__ int s_found;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t plane = blockIdx.x;
    const float* d = det + plane * H * W;
    const float* tm = tmap + plane * H * W * tstride;
    float* pval = val + plane * M;
    float* ptag = tag + plane * M;
    int* pind = ind + plane * M * 2;
    const int segs = (W + 63) >> 6;
    int found = 0;                                        // peaks seen so far in raster order (uniform)
    for (int r0 = 0; r0 < H && found < M; r0 += R) {
        const int rows = min(R, H - r0);
        const int lo = max(r0 - win, 0), hi = min(r0 + rows + win, H);
        const int cells = (hi - lo) * W;                  // <= FP_BAND_FLOATS by the choice of R
        for (int i = tid; i < cells; i += FP_THREADS) band[i] = d[(size_t)lo * W + i];
        __syncthreads();
        const int rpw = (rows + FP_WAVES - 1) / FP_WAVES;
        const int wr1 = min((wave + 1) * rpw, rows);
        for (int r = wave * rpw; r < wr1; ++r) {
            const int y = r0 + r;
            const int y0 = max(y - win, 0), y1 = min(y + win + 1, H);
            for (int sg = 0; sg < segs; ++sg) {
                const int x = sg * 64 + lane;
                bool peak = false;
                if (x < W) {
                    const float v = band[(y - lo) * W + x];
                    if (!(v < threshold)) {
                        peak = true;
                        const int x0 = max(x - win, 0), x1 = min(x + win + 1, W);
                        for (int yy = y0; yy < y1; ++yy)
                            for (int xx = x0; xx < x1; ++xx)
                                if (band[(yy - lo) * W + xx] > v) peak = false;
                    }
                }
                const unsigned long long m = __ballot(peak);
                if (lane == 0) masks[r * segs + sg] = m;
            }
        }
        __syncthreads();
        if (wave == 0) {
            const int E = rows * segs;                    // <= FP_MAX_ENTRIES by the choice of R
            int b = found;
            for (int e0 = 0; e0 < E && b < M; e0 += 64) {
                const int e = e0 + lane;
                unsigned long long m = e < E ? masks[e] : 0ull;
                const int c = __popcll(m);
                int incl = c;
                for (int s = 1; s < 64; s <<= 1) {
                    const int t = __shfl_up(incl, s);
                    if (lane >= s) incl += t;
                }
                int slot = b + incl - c;
                const int y = r0 + e / segs, xb = (e % segs) * 64;
                while (m != 0ull && slot < M) {
                    const int x = xb + __builtin_ctzll(m);
                    m &= m - 1;
                    pval[slot] = band[(y - lo) * W + x];
                    ptag[slot] = tm[((size_t)y * W + x) * tstride];
                    pind[2 * slot] = x;
                    pind[2 * slot + 1] = y;
                    ++slot;
                }
                b += __shfl(incl, 63);
            }
            if (lane == 0) s_found = b;
        }
        __syncthreads();
        found = s_found;
    }
    const int cnt = min(found, M);
    if (tid == 0) count[plane] = cnt;
    if (tid >= cnt && tid < M) {                          // unused slots: zero, as the reference's zero-allocated outputs
        pval[tid] = 0.f;
        ptag[tid] = 0.f;
        pind[2 * tid] = 0;
        pind[2 * tid + 1] = 0;
    }
}

namespace {
struct LdsMem {                                           // cell w of this lane's image: column `lane` of a [words][64] table
    fast::Cell* c;
    int lane;
    __device__ fast::Cell& operator[](int w) const { return c[w * 64 + lane]; }
};
}  // namespace

// assign_out (assign.cpp:65-122) for 64 images per workgroup, one lane each: a serial walk over joint_order whose
// Kuhn-Munkres state (fast_assign.h) sits in LDS columns, so lanes of the wave run different images without per-thread
// arrays.  The workgroup first zeroes its images' records together (the reference's zero-allocated ans); an image whose KM
// hits the round cap gets num = -1 and its record zeroed again.
__global__ __launch_bounds__(64) void fast_assign_kernel(
    const int* __restrict__ count, const float* __restrict__ val, const float* __restrict__ tag,
    const int* __restrict__ ind, int N, int J, int M, fast::JointOrder order, float tag_threshold, float* ans, int* num) {
    __shared__ fast::Cell cells[fast::C_WORDS * 64];
    const int lane = threadIdx.x;
    const int n0 = blockIdx.x * 64;
    const int nimg = min(64, N - n0);
    const size_t per = (size_t)M * J * 4;
    float* a0 = ans + n0 * per;
    for (size_t i = lane; i < nimg * per; i += 64) a0[i] = 0.f;
    __syncthreads();
    if (lane >= nimg) return;
    const size_t n = (size_t)n0 + lane;
    float* a = ans + n * per;
    const int r = fast::assign_image(LdsMem{cells, lane}, count + n * J, val + n * J * M, tag + n * J * M,
                                     ind + n * J * M * 2, order, J, M, tag_threshold, a);
    if (r < 0)
        for (size_t i = 0; i < per; ++i) a[i] = 0.f;
    num[n] = r;
}

void launch_fast_peaks(const float* det, const float* tmap, long tstride, int N, int J, int H, int W, float threshold,
                       int window, int M, int* count, float* val, float* tag, int* ind, hipStream_t s) {
    const int win = window / 2;
    const int segs = (W + 63) / 64;
    int R = FP_BAND_FLOATS / W - 2 * win;                 // W <= 1024, win <= 3: at least 6 rows
    R = R < FP_MAX_ENTRIES / segs ? R : FP_MAX_ENTRIES / segs;
    R = R < H ? R : H;
    fast_peaks_kernel<<<dim3((unsigned)(N * J)), dim3(FP_THREADS), 0, s>>>(det, tmap, tstride, H, W, threshold, win, M, R,
                                                                          count, val, tag, ind);
}

void launch_fast_assign(const int* count, const float* val, const float* tag, const int* ind, int N, int J, int M,
                        const int* joint_order, float tag_threshold, float* ans, int* num, hipStream_t s) {
    fast::JointOrder o;
    for (int i = 0; i < 32; ++i) o.v[i] = i < J ? joint_order[i] : 0;
    fast_assign_kernel<<<dim3((unsigned)((N + 63) / 64)), dim3(64), 0, s>>>(count, val, tag, ind, N, J, M, o,
                                                                            tag_threshold, ans, num);
}

}  // namespace lp
