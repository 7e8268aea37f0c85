// The shape of the 128-row tile of the three kernels on v_mfma_f32_32x32x16_bf16 (csrc/bf16_tile.hpp) and its staging map, free of HIP
// constructs outside the macros: the load plans (csrc/unit_bf16_plan.hpp, csrc/conv3x3_bf16_plan.hpp) are also compiled into
// stand-alone CPU programs (tests/host/), which enumerate the very accesses that the kernels make.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OPA_TILE_HD __host__ __device__ inline
#define OPA_TILE_UNROLL _Pragma("unroll")
#else
#define OPA_TILE_HD inline
#define OPA_TILE_UNROLL
#endif

namespace opa {

constexpr int kBf16BM = 128, kBf16BK = 64, kBf16Threads = 256;     // rows of A and columns of K per workgroup and K-step
constexpr int kBf16Passes = kBf16BM / 32;                          // row passes of the A staging map
constexpr int kBf16Pitch = kBf16BK + 8;                            // LDS row pitch in bf16

// staging map: a 64-wide bf16 row is 8 chunks of 16 B; 256 threads cover 32 rows per pass.  Thread t stages the chunk at column
// `col` of the rows p * 32 + `row`, p = 0 .. kBf16Passes - 1 (W: as many passes as the tile has 32-row blocks).
struct Bf16Stage {
    int row, col;
};
OPA_TILE_HD Bf16Stage bf16_tile_stage(int t) { return {t >> 3, (t & 7) * 8}; }

}  // namespace opa
