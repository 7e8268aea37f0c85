// A 16-byte vector of float32, float16 or bfloat16 elements and its conversion to and from float32 (dtype codes of the C ABI:
// 0 = float32, 1 = float16, 2 = bfloat16): shared by the element-wise kernels (epilogue.hip, pool.hip).
#pragma once
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

namespace opa {

struct alignas(16) Vec16 { unsigned int w[4]; };

template <int DT> struct Elem;
template <> struct Elem<0> {   // f32
    static constexpr int kPerVec = 4;
    static __device__ __forceinline__ void unpack(const Vec16& v, float* f) {
        for (int i = 0; i < 4; i++) f[i] = __uint_as_float(v.w[i]);
    }
    static __device__ __forceinline__ void pack(const float* f, Vec16& v) {
        for (int i = 0; i < 4; i++) v.w[i] = __float_as_uint(f[i]);
    }
};
template <> struct Elem<1> {   // f16
    static constexpr int kPerVec = 8;
    static __device__ __forceinline__ void unpack(const Vec16& v, float* f) {
        for (int i = 0; i < 4; i++) {
            const __half2 h = *reinterpret_cast<const __half2*>(&v.w[i]);
            f[2 * i] = __low2float(h); f[2 * i + 1] = __high2float(h);
        }
    }
    static __device__ __forceinline__ void pack(const float* f, Vec16& v) {
        for (int i = 0; i < 4; i++) {
            const __half2 h = __floats2half2_rn(f[2 * i], f[2 * i + 1]);
            v.w[i] = *reinterpret_cast<const unsigned int*>(&h);
        }
    }
};
template <> struct Elem<2> {   // bf16
    static constexpr int kPerVec = 8;
    static __device__ __forceinline__ void unpack(const Vec16& v, float* f) {
        for (int i = 0; i < 4; i++) {
            f[2 * i] = __uint_as_float(v.w[i] << 16);
            f[2 * i + 1] = __uint_as_float(v.w[i] & 0xffff0000u);
        }
    }
    static __device__ __forceinline__ unsigned rne(float x) {      // float -> bf16 bits, round to nearest even
        unsigned u = __float_as_uint(x);
        if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;   // NaN
        u += 0x7fffu + ((u >> 16) & 1u);
        return u >> 16;
    }
    static __device__ __forceinline__ void pack(const float* f, Vec16& v) {
        for (int i = 0; i < 4; i++) v.w[i] = rne(f[2 * i]) | (rne(f[2 * i + 1]) << 16);
    }
};

}  // namespace opa
