// The reference's real-time grouping (nano_demo/fast_utils/parse/assign.cpp: assign_out, KM, match, update) for ONE image,
// restated without recursion and without per-thread arrays: all state lives in `Mem`, an array of 4-byte cells the caller
// provides (LDS columns on the device, one lane per image; a plain array on the host, tests/fast_assign_host.cpp).
// Plain C++: the same text is compiled by hipcc for gfx950 and by the host compiler, and both must be built WITHOUT fp
// contraction -- every operation below is the reference's, in its order:
//   mean   = (float)((double)sum / nj)                    `1.0 * sum[j] / nj[j]` passed to a float parameter (:95)
//   dist   = sqrt((x - y) * (x - y))                      float product, ::sqrt(double), rounded back to float: the correctly
//                                                         rounded float square root (53 >= 2 * 24 + 2 bits)
//   G      = -(dist * 100 - val), -1e4 outside the real rows / columns
//   tight  = abs(t) < 1e-2 with t = Lx[u] + Ly[i] - G     AS THE COMPILED REFERENCE EVALUATES IT: assign.cpp includes <cmath> and
//                                                         calls the unqualified `abs` from inside its own namespace, where only
//                                                         ::abs(int) is visible, so t is converted to int first and the edge is
//                                                         tight iff -1 < t < 1.  (A t outside the int range, or NaN, is undefined
//                                                         there; the labels of ordinary tag maps stay far from it, and here
//                                                         such an edge is not tight.)
// tests/golden/gen_golden_fast.py asserts this text against the compiled reference on every scene it generates, with the
// round cap lifted (LP_FAST_KM_ROUND_CAP).
#pragma once

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define LP_FAST_HD __host__ __device__ __forceinline__
#else
#include <cmath>
#define LP_FAST_HD inline
#endif

namespace lp {
namespace fast {

constexpr int MAX_PEOPLE = 10;       // the reference's arrays are [10] (assign.cpp:44-46,74-75)
#ifndef LP_FAST_KM_ROUND_CAP
#define LP_FAST_KM_ROUND_CAP 4096    // a condition of the interface, not a tuning knob (only the golden generator lifts it)
#endif
constexpr int KM_ROUND_CAP = LP_FAST_KM_ROUND_CAP;   // match / update rounds of one KM call (one joint); the reference's loop has no bound

union Cell {
    float f;
    int i;
};

// cell indices of one image's state
enum {
    C_G = 0,          // [10][10] G of the current joint
    C_MEAN = 100,     // [10] person means the current joint was compared with (diff[j][k] is dist(mean[j], tag[k]))
    C_LX = 110,
    C_LY = 120,
    C_SLACK = 130,
    C_MAT = 140,
    C_CH = 150,
    C_NJ = 160,
    C_SUM = 170,
    C_STACK = 180,    // [10] frames of match(): u | i << 8
    C_WORDS = 190
};

struct JointOrder {
    int v[32];
};

LP_FAST_HD float sqrt_rn(float x) {
#ifdef __HIP_DEVICE_COMPILE__
    return __fsqrt_rn(x);
#else
    return sqrtf(x);
#endif
}

LP_FAST_HD float dist(float x, float y) {
    const float d = x - y;
    return sqrt_rn(d * d);
}

LP_FAST_HD bool tight_edge(float t) {
    return t > -1.0f && t < 1.0f;
}

// KM(ch, G, n) of assign.cpp:43-63 on mem[C_G ...]; false when the round cap is hit
template <class Mem>
LP_FAST_HD bool km(Mem mem, const int n) {
    for (int i = 0; i < n; ++i) {
        float lx = -1e6f;
        for (int j = 0; j < n; ++j) {
            const float g = mem[C_G + i * MAX_PEOPLE + j].f;
            lx = lx > g ? lx : g;
        }
        mem[C_LX + i].f = lx;
        mem[C_LY + i].f = 0.f;
        mem[C_MAT + i].i = -1;
    }
    int rounds = 0;
    for (int root = 0; root < n; ++root) {
        for (int j = 0; j < n; ++j) mem[C_SLACK + j].f = 1e6f;
        for (;;) {
            if (++rounds > KM_ROUND_CAP) return false;
            // match(root): the recursion as a stack of (u, i) frames; a frame is pushed only after a new T[i] was set, so
            // the depth never exceeds n
            unsigned S = 0, T = 0;
            int sp = 0, u = root, i = 0;
            bool found = false;
            S |= 1u << u;
            for (;;) {
                if (i >= n) {                        // this frame returns false: the caller goes on after its i
                    if (sp == 0) break;
                    const int fr = mem[C_STACK + --sp].i;
                    u = fr & 0xff;
                    i = (fr >> 8) + 1;
                    continue;
                }
                if (T >> i & 1u) {
                    ++i;
                    continue;
                }
                const float t = mem[C_LX + u].f + mem[C_LY + i].f - mem[C_G + u * MAX_PEOPLE + i].f;
                if (tight_edge(t)) {
                    T |= 1u << i;
                    const int m = mem[C_MAT + i].i;
                    if (m == -1) {                   // every frame returns true: mat[i] = u on the way up
                        mem[C_MAT + i].i = u;
                        while (sp > 0) {
                            const int fr = mem[C_STACK + --sp].i;
                            mem[C_MAT + (fr >> 8)].i = fr & 0xff;
                        }
                        found = true;
                        break;
                    }
                    mem[C_STACK + sp++].i = u | i << 8;
                    u = m;
                    S |= 1u << u;
                    i = 0;
                    continue;
                }
                const float s = mem[C_SLACK + i].f;
                mem[C_SLACK + i].f = s < t ? s : t;
                ++i;
            }
            if (found) break;
            float d = 1e8f;                          // update()
            for (int k = 0; k < n; ++k) {
                const float s = mem[C_SLACK + k].f;
                d = d < s ? d : s;
            }
            for (int k = 0; k < n; ++k) {
                if (S >> k & 1u) mem[C_LX + k].f -= d;
                if (T >> k & 1u) mem[C_LY + k].f += d;
            }
        }
    }
    for (int i = 0; i < n; ++i) mem[C_CH + mem[C_MAT + i].i].i = i;
    return true;
}

LP_FAST_HD void put(float* ans, int q, const int* ind, const float* val, const float* tag, int p) {
    ans[q] = (float)ind[2 * p];
    ans[q + 1] = (float)ind[2 * p + 1];
    ans[q + 2] = val[p];
    ans[q + 3] = tag[p];
}

// assign_out of assign.cpp:65-122 for one image: cnt [C], val / tag [C][M], ind [C][M][2] -> ans [M][C][4] (already zero),
// returns num, or -1 when a KM call hit the round cap (the caller zeroes ans again).  A count outside 0..M is clamped
// (the reference would index out of its arrays).
template <class Mem>
LP_FAST_HD int assign_image(Mem mem, const int* cnt, const float* val, const float* tag, const int* ind,
                            const JointOrder& order, const int C, const int M, const float threshold, float* ans) {
    int num = 0;
    for (int id = 0; id < C; ++id) {
        const int i = order.v[id];
        int c = cnt[i];
        c = c < 0 ? 0 : (c > M ? M : c);
        if (c == 0) continue;
        if (num == 0) {
            num = c;
            for (int j = 0; j < num; ++j) {
                put(ans, (j * C + i) * 4, ind, val, tag, i * M + j);
                mem[C_NJ + j].i = 1;
                mem[C_SUM + j].f = tag[i * M + j];
            }
            continue;
        }
        const int n = num > c ? num : c;
        for (int j = 0; j < num; ++j) mem[C_MEAN + j].f = (float)((double)mem[C_SUM + j].f / mem[C_NJ + j].i);
        for (int j = 0; j < n; ++j)
            for (int k = 0; k < n; ++k) {
                float g = -1e4f;
                if (j < num && k < c) g = -(dist(mem[C_MEAN + j].f, tag[i * M + k]) * 100 - val[i * M + k]);
                mem[C_G + j * MAX_PEOPLE + k].f = g;
            }
        if (!km(mem, n)) return -1;
        const int old_num = num;
        for (int j = 0; j < n; ++j) {
            const int k = mem[C_CH + j].i;
            if (k >= c) continue;
            const int p = i * M + k;
            if (j < old_num && dist(mem[C_MEAN + j].f, tag[p]) < threshold) {
                put(ans, (j * C + i) * 4, ind, val, tag, p);
                mem[C_NJ + j].i += 1;
                mem[C_SUM + j].f += tag[p];
            } else {
                if (num == M) continue;
                put(ans, (num * C + i) * 4, ind, val, tag, p);
                mem[C_NJ + num].i = 1;
                mem[C_SUM + num].f = tag[p];
                ++num;
            }
        }
    }
    return num;
}

}  // namespace fast
}  // namespace lp
