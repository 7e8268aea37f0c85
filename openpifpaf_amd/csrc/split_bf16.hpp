// A float32 number as the exact sum of three bfloat16 pieces (csrc/gemm_f32x3.hip, csrc/winograd.hip variant 4): its 24-bit
// significand cut into 8 + 8 + 8 bits by truncation -- a1 = a with the low 16 bits cleared, r = a - a1, a2 = r with the low 16
// bits cleared, a3 = r - a2; every step exact, every piece representable (bf16 has float32's exponent range) for every finite
// |a| >= 2^-110 and for zero.  Below 2^-110 the low pieces are subnormal bf16 numbers and a has bits under 2^-133, the smallest
// of them: taking the high halves truncates those (a subnormal float32 a has an empty second piece and up to 16 bits in the
// third).  Measured (profiles/x3_edges/errors.log): v_mfma_f32_32x32x16_bf16 KEEPS subnormal bf16 inputs -- the elements of
// tests/test_gpu_x3_edges.py::test_subnormal_pieces that tell come out at 3-8e-8 of sum |a||w|, where a pipe that flushed them
// would leave 1e-6 and more (tests/test_x3_cases.py); an element loses less than 2^-125 sum_k (|a_mk| + |w_nk|) to the bits
// under 2^-133.
// +-Inf leaves as (+-Inf, NaN, NaN) -- a - a1 is Inf - Inf -- and NaN as NaN in every piece: a non-finite operand makes every
// product it enters NaN (its output row; for a weight its output channel), and only those (tests/test_gpu_x3_edges.py).
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
