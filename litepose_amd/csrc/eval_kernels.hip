// COCO keypoint evaluation on the records as lp_final_preds_v leaves them (include/litepose_amd.h, "evaluation"): per
// record row the OKS of every kept detection against every annotation of the row's image and the greedy matching at
// every (area range, threshold) -- the published COCOeval algorithm for iouType = 'keypoints' (computeOks + evaluateImg),
// restated in DESIGN.md 4b.  Every fp64 operation is one IEEE operation in the order of the protocol (this file is
// compiled without FMA contraction); exp is the device library's.
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include "kernels.h"

namespace lp {

namespace {
constexpr int KE_THREADS = 256;
constexpr int KE_MAXD = 32;                               // kept detections per image (maxDets)
constexpr int KE_MAXG = 64;                               // annotations per image: the matched set is one 64-bit mask

// descending score with NaN last: a total order, so the ranks of a row are a permutation
__device__ inline bool score_above(float w, float v) { return w > v || (v != v && w == w); }
__device__ inline bool score_equal(float w, float v) { return w == v || (w != w && v != v); }
}  // namespace

// One workgroup per record row.
//   phase 1  rank of a detection = #(greater score) + #(equal score with a lower index): the stable descending sort by
//            counting; ranks < max_dets are kept, their area_d = (max x - min x) * (max y - min y) over J_eval joints
//   phase 2  OKS [kept][G] in LDS, one (d, g) pair per thread and step, joints summed in joint order
//   phase 3  lane b = a * n_thr + t of wave 0 walks detections x annotations for area range a and threshold t: first the
//            annotations that a does not ignore, then -- only if none matched -- the ignored ones (COCOeval's sort by
//            _ignore plus its break); the matched set is a 64-bit mask in registers; a detection's bits of all lanes
//            are gathered with a ballot and lane 0 stores the two words
__global__ __launch_bounds__(KE_THREADS) void kpt_eval_kernel(
    const float* __restrict__ ans, const int* __restrict__ count, const float* __restrict__ scores, int pcap, int J, int D,
    int J_eval, const int* __restrict__ row_image, const double* __restrict__ gt_kpts, const double* __restrict__ gt_area,
    const double* __restrict__ gt_bbox, const int* __restrict__ gt_flags, const int* __restrict__ gt_first, int images,
    KptEvalTables tb, int nbits, int max_dets, float* __restrict__ score_out, int* __restrict__ num_out,
    int* __restrict__ src_out, unsigned* __restrict__ match_out, unsigned* __restrict__ ignore_out,
    double* __restrict__ oks_out) {
    __shared__ double s_oks[KE_MAXD * KE_MAXG];
    __shared__ double s_darea[KE_MAXD];
    __shared__ double s_garea[KE_MAXG];
    __shared__ float s_score[KE_MAXD];
    __shared__ int s_src[KE_MAXD];
    __shared__ int s_gflags[KE_MAXG];
    __shared__ int s_k1[KE_MAXG];
    const int tid = threadIdx.x;
    const size_t n = blockIdx.x;
    const int img = row_image[n];
    int c = 0, g0 = 0, G = 0;
    if (img >= 0 && img < images) {                       // any other slot: the row is skipped, its outputs are zero
        c = min(max(count[n], 0), pcap);
        g0 = gt_first[img];
        G = min(max(gt_first[img + 1] - g0, 0), KE_MAXG);
    }
    const int num = min(c, max_dets);
    const float* sc = scores + n * pcap;
    if (tid < KE_MAXD) {
        s_src[tid] = -1;
        s_score[tid] = 0.f;
        s_darea[tid] = 0.0;
    }
    __syncthreads();

    // ---- phase 1
    for (int p = tid; p < c; p += KE_THREADS) {
        const float v = sc[p];
        int rank = 0;
        for (int q = 0; q < c; ++q) {
            const float w = sc[q];
            rank += (score_above(w, v) || (score_equal(w, v) && q < p)) ? 1 : 0;
        }
        if (rank < max_dets) {
            s_src[rank] = p;
            s_score[rank] = v;
        }
    }
    if (tid < G) {
        const double* kg = gt_kpts + (size_t)(g0 + tid) * J_eval * 3;
        int k1 = 0;
        for (int j = 0; j < J_eval; ++j) k1 += kg[3 * j + 2] > 0.0 ? 1 : 0;
        s_k1[tid] = k1;
        s_garea[tid] = gt_area[g0 + tid];
        s_gflags[tid] = gt_flags[g0 + tid];
    }
    __syncthreads();
    if (tid < num && s_src[tid] >= 0) {
        const float* kd = ans + (n * pcap + s_src[tid]) * J * D;
        float x0 = kd[0], x1 = kd[0], y0 = kd[1], y1 = kd[1];
        for (int j = 1; j < J_eval; ++j) {
            const float x = kd[j * D], y = kd[j * D + 1];
            x0 = x < x0 ? x : x0;
            x1 = x > x1 ? x : x1;
            y0 = y < y0 ? y : y0;
            y1 = y > y1 ? y : y1;
        }
        s_darea[tid] = ((double)x1 - (double)x0) * ((double)y1 - (double)y0);
    }

    // ---- phase 2
    const int pairs = num * G;
    for (int idx = tid; idx < pairs; idx += KE_THREADS) {
        const int d = idx / G, g = idx - d * G;
        const int src = s_src[d];
        double o = 0.0;
        if (src >= 0) {
            const float* kd = ans + (n * pcap + src) * J * D;
            const double* kg = gt_kpts + (size_t)(g0 + g) * J_eval * 3;
            const int k1 = s_k1[g];
            const double ar = s_garea[g] + DBL_EPSILON;   // area + np.spacing(1)
            double sum = 0.0;
            if (k1 > 0) {
                for (int j = 0; j < J_eval; ++j) {
                    if (kg[3 * j + 2] > 0.0) {
                        const double dx = (double)kd[j * D] - kg[3 * j];
                        const double dy = (double)kd[j * D + 1] - kg[3 * j + 1];
                        const double e = (dx * dx + dy * dy) / tb.vars[j] / ar / 2.0;
                        sum += exp(-e);
                    }
                }
                o = sum / (double)k1;
            } else {                                      // no labelled joint: distance to the doubled box
                const double* bb = gt_bbox + (size_t)(g0 + g) * 4;
                const double bx0 = bb[0] - bb[2], bx1 = bb[0] + bb[2] * 2.0;
                const double by0 = bb[1] - bb[3], by1 = bb[1] + bb[3] * 2.0;
                for (int j = 0; j < J_eval; ++j) {
                    const double xd = (double)kd[j * D], yd = (double)kd[j * D + 1];
                    const double ax = bx0 - xd, bxx = xd - bx1, ay = by0 - yd, byy = yd - by1;
                    const double dx = (ax > 0.0 ? ax : 0.0) + (bxx > 0.0 ? bxx : 0.0);
                    const double dy = (ay > 0.0 ? ay : 0.0) + (byy > 0.0 ? byy : 0.0);
                    const double e = (dx * dx + dy * dy) / tb.vars[j] / ar / 2.0;
                    sum += exp(-e);
                }
                o = sum / (double)J_eval;
            }
        }
        s_oks[d * KE_MAXG + g] = o;
    }
    __syncthreads();

    // ---- phase 3 (wave 0; lanes >= nbits walk along with bit 0's tables and contribute nothing)
    const size_t row = n * max_dets;
    if (tid < 64) {
        const bool act = tid < nbits;
        const int b = act ? tid : 0;
        const double lo = tb.lo[b], hi = tb.hi[b], best0 = tb.best0[b];
        uint64_t ig = 0, crowd = 0;
        for (int g = 0; g < G; ++g) {
            const int f = s_gflags[g];
            const double a = s_garea[g];
            const bool i = (f & 2) != 0 || a < lo || a > hi;
            ig |= (uint64_t)(i ? 1 : 0) << g;
            crowd |= (uint64_t)(f & 1) << g;
        }
        uint64_t matched = 0;
        for (int d = 0; d < num; ++d) {
            double best = best0;
            int m = -1;
            for (int pass = 0; pass < 2; ++pass) {
                const uint64_t open = (pass ? ig : ~ig) & (~matched | crowd);
                if (pass == 0 || m < 0) {
                    for (int g = 0; g < G; ++g) {
                        const double o = s_oks[d * KE_MAXG + g];
                        if ((open >> g & 1) != 0 && !(o < best)) {
                            best = o;
                            m = g;
                        }
                    }
                }
            }
            const bool dm = m >= 0;
            bool di;
            if (dm) {
                di = (ig >> m & 1) != 0;
                matched |= (uint64_t)1 << m;
            } else {
                const double ad = s_darea[d];
                di = ad < lo || ad > hi;
            }
            const uint64_t mw = __ballot(act && dm);
            const uint64_t iw = __ballot(act && di);
            if (tid == 0) {
                match_out[row + d] = (unsigned)mw;
                ignore_out[row + d] = (unsigned)iw;
            }
        }
    }

    // ---- every other element of the outputs
    for (int i = tid; i < max_dets; i += KE_THREADS) {
        const bool used = i < num;
        score_out[row + i] = used ? s_score[i] : 0.f;
        src_out[row + i] = used ? max(s_src[i], 0) : 0;
        if (!used) {
            match_out[row + i] = 0u;
            ignore_out[row + i] = 0u;
        }
    }
    if (tid == 0) num_out[n] = num;
    if (oks_out) {
        double* po = oks_out + row * KE_MAXG;
        for (int i = tid; i < max_dets * KE_MAXG; i += KE_THREADS)
            po[i] = ((i >> 6) < num && (i & 63) < G) ? s_oks[i] : 0.0;
    }
}

void launch_kpt_eval(const float* ans, const int* count, const float* scores, int N, int pcap, int J, int T, int J_eval,
                     const int* row_image, const double* gt_kpts, const double* gt_area, const double* gt_bbox,
                     const int* gt_flags, const int* gt_first, int images, const KptEvalTables& tb, int nbits,
                     int max_dets, float* score_out, int* num_out, int* src_out, unsigned* match_out,
                     unsigned* ignore_out, double* oks_out, hipStream_t s) {
    kpt_eval_kernel<<<dim3((unsigned)N), dim3(KE_THREADS), 0, s>>>(
        ans, count, scores, pcap, J, 3 + T, J_eval, row_image, gt_kpts, gt_area, gt_bbox, gt_flags, gt_first, images, tb,
        nbits, max_dets, score_out, num_out, src_out, match_out, ignore_out, oks_out);
}

}  // namespace lp
