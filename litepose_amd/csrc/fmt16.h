// The two 16-bit storage formats of the reduced-precision network path (bf16_kernels.hip, mbtile_bf16.hip, the rounded
// forms of stem4_kernel).  Every kernel of that path is ONE __device__ body and ONE __global__ template, both with the
// format F as their leading template argument (lp::mbtb_kernel<lp::Bf16, 1, 1, true>, lp::mbtb_kernel<lp::F16, 1, 1, true>);
// the format-specific parts are the five operations below, everything else (octet-planar records, fragment layouts, fp32
// accumulation, bias / activation / residual in fp32, one rounding where a tensor is stored) is shared.  A launcher turns
// its `bool f16` into F once, through with_fmt, so every form exists in both formats with the same template list
// (tests/test_f16_cpu.py holds that against the build's resource report).
//   Bf16: v_cvt_pk_bf16_f32 (RNE), unpack = a shift, v_mfma_f32_*_bf16, v_dot2_f32_bf16.
//   F16:  IEEE half (the reference's network_to_half, fp16util.py:87-91): v_cvt_pk_f16_f32 (RNE, overflow to +-inf; never
//         v_cvt_pkrtz_f16_f32: toward zero), unpack = v_cvt_f32_f16, v_mfma_f32_*_f16, v_dot2c_f32_f16.  Subnormals KEPT by all
//         four, the dot2's operands included (measured: tests/test_gpu_f16_range.py): float_denorm_mode_16_64 = 3, never set.
// Products of two 16-bit values of either format are exact in fp32 (8 + 8 or 11 + 11 significant bits; an fp16 subnormal
// product is >= 2^-48, a normal fp32), so the MFMA and FMA chains keep the emulation's arithmetic.
#pragma once
#include "split3.h"

namespace lp {

typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));

struct Bf16 {
    __device__ static __forceinline__ unsigned pack(float lo, float hi) {     // RNE, lo in bits 0-15
        typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
        const f32x2 v = {lo, hi};
        return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
    }
    __device__ static __forceinline__ float lo(unsigned u) { return __uint_as_float(u << 16); }
    __device__ static __forceinline__ float hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }
    __device__ static __forceinline__ float round(float v) { return lo(pack(v, 0.f)); }
    __device__ static __forceinline__ f32x16 mfma32(u32x4 a, u32x4 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c,
                                                       0, 0, 0);
    }
    __device__ static __forceinline__ f32x4 mfma16(u32x4 a, u32x4 b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c,
                                                       0, 0, 0);
    }
    __device__ static __forceinline__ float dot2(unsigned a, unsigned b, float acc) {
        typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
        return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, a), __builtin_bit_cast(bf16x2, b), acc, false);
    }
};

struct F16 {
    __device__ static __forceinline__ unsigned pack(float lo, float hi) {     // RNE (v_cvt_pk_f16_f32), lo in bits 0-15
        typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
        const f32x2 v = {lo, hi};
        return __builtin_bit_cast(unsigned, __builtin_convertvector(v, f16x2));
    }
    __device__ static __forceinline__ float lo(unsigned u) {
        return (float)__builtin_bit_cast(_Float16, (unsigned short)(u & 0xffffu));
    }
    __device__ static __forceinline__ float hi(unsigned u) {
        return (float)__builtin_bit_cast(_Float16, (unsigned short)(u >> 16));
    }
    __device__ static __forceinline__ float round(float v) { return lo(pack(v, 0.f)); }
    __device__ static __forceinline__ f32x16 mfma32(u32x4 a, u32x4 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c,
                                                      0, 0, 0);
    }
    __device__ static __forceinline__ f32x4 mfma16(u32x4 a, u32x4 b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c,
                                                      0, 0, 0);
    }
    __device__ static __forceinline__ float dot2(unsigned a, unsigned b, float acc) {
        typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
        return __builtin_amdgcn_fdot2(__builtin_bit_cast(f16x2, a), __builtin_bit_cast(f16x2, b), acc, false);
    }
};

// fp32 storage: stem4_kernel's unrounded form (its planar fp32 output needs no pack)
struct F32 {
    __device__ static __forceinline__ float round(float v) { return v; }
};

// the one place a launcher's `bool f16` becomes a format: with_fmt(f16, [&](auto F) { ...<decltype(F), ...>... })
template <class Fn>
inline auto with_fmt(bool f16, Fn&& fn) {
    return f16 ? fn(F16{}) : fn(Bf16{});
}

}  // namespace lp
