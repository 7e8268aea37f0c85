// A float32 number as the exact sum of three bfloat16 pieces (csrc/gemm_f32x3.hip, csrc/winograd.hip variant 4): its 24-bit
// significand cut into 8 + 8 + 8 bits by truncation -- a1 = a with the low 16 bits cleared, r = a - a1, a2 = r with the low 16
// bits cleared, a3 = r - a2; every step exact, every piece representable (bf16 has float32's exponent range).
#pragma once

#include <hip/hip_runtime.h>

namespace opa {

typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2_t;

// four float32 -> their three bf16 pieces, packed pairwise (element e in the low half of word e / 2 ... K-major order)
__device__ __forceinline__ void split4(const f32x4_t a, u32x2_t& p1, u32x2_t& p2, u32x2_t& p3) {
    unsigned u[4], v[4], w[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
        u[e] = __float_as_uint(a[e]);
        const float r1 = a[e] - __uint_as_float(u[e] & 0xffff0000u);       // exact: the low 16 significand bits
        v[e] = __float_as_uint(r1);
        const float r2 = r1 - __uint_as_float(v[e] & 0xffff0000u);         // exact: at most 8 significant bits are left
        w[e] = __float_as_uint(r2);
    }
    // high halves of two words side by side: bytes {hi.3, hi.2, lo.3, lo.2}
    p1[0] = __builtin_amdgcn_perm(u[1], u[0], 0x07060302u); p1[1] = __builtin_amdgcn_perm(u[3], u[2], 0x07060302u);
    p2[0] = __builtin_amdgcn_perm(v[1], v[0], 0x07060302u); p2[1] = __builtin_amdgcn_perm(v[3], v[2], 0x07060302u);
    p3[0] = __builtin_amdgcn_perm(w[1], w[0], 0x07060302u); p3[1] = __builtin_amdgcn_perm(w[3], w[2], 0x07060302u);
}

}  // namespace opa
