// The tile that the kernels on v_mfma_f32_32x32x16_bf16 share (csrc/gemm_epilogue.hip, csrc/gemm_unit_bf16.hip, csrc/conv3x3_bf16.hip):
//     acc[128, BN] = A[128, K] * W[BN, K]^T        (16-bit operands, float32 accumulation)
// The element type is a template parameter, the C ABI's dtype code DT (csrc/vec16.hpp): 2 = bfloat16, the default, which the kernels
// that exist in bfloat16 alone never name; 1 = float16 on v_mfma_f32_32x32x16_f16, the same fragment order at the same rate.  Only
// TileElem<DT> depends on it -- the fragment type, the MFMA, the decoding of an element to float32 and the rounding at the store; every
// operand travels as raw 16-bit words, so shape, LDS pitch, staging map, tile order and the patch epilogue are one for both.
// 128 x BN (BN = 128 or 64) per 256-thread workgroup, BK = 64; 4 waves as 2 (M) x 2 (N), each wave a 64 x BN/2 sub-tile of 32x32 MFMA
// blocks.  Both operands are K-major, the fragment order of the instruction (lane l holds 8 consecutive k of row l & 31, k-offset
// 8 * (l >> 5)); they are staged global -> registers -> LDS (row pitch 72 bf16 = 144 B keeps the ds_read_b128 fragment reads at
// <= 2-way bank conflicts), the next K-step travelling in registers while this one multiplies; several workgroups per CU overlap each
// other's loads and MFMAs.  A kernel supplies how A reaches the registers (a callable) and its epilogue; for the latter the
// accumulators (+ bias) go through a wave-private float32 LDS patch, one 32-row block at a time, so that what is combined with them
// and the output are reached by row-contiguous vectors.
//
// csrc/gemm_unit_bf16.hip takes shape, tile order, accumulator layout and fence from here and keeps the main loop written out in its
// own body (see there).
//
// Every function here takes the thread's place from threadIdx itself (bf16_tile_wave), never as an argument: the compiler optimises
// a function on its own before it inlines it, and without the lane's range in sight (0 .. 63) the index arithmetic takes forms that
// cost registers and the pairing of LDS stores later on.
#pragma once
#include "common.hpp"
#include "bf16_tile_shape.hpp"

namespace opa {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;

__device__ __forceinline__ float bf16_lo(unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf16_hi(unsigned w) { return __uint_as_float(w & 0xffff0000u); }
__device__ __forceinline__ unsigned bf16_rne(float x) {
    unsigned u = __float_as_uint(x);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
    u += 0x7fffu + ((u >> 16) & 1u);
    return u >> 16;
}

// What the tile's element type decides: the two elements of a 32-bit word as float32 (lo, hi), float32 -> element bits, round to
// nearest even (rne), the fragment type and the MFMA.
template <int DT> struct TileElem;
template <> struct TileElem<2> {   // bf16
    typedef bf16x8_t frag_t;
    static __device__ __forceinline__ float lo(unsigned w) { return bf16_lo(w); }
    static __device__ __forceinline__ float hi(unsigned w) { return bf16_hi(w); }
    static __device__ __forceinline__ unsigned rne(float x) { return bf16_rne(x); }
    static __device__ __forceinline__ f32x16_t mfma(frag_t a, frag_t b, f32x16_t c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    }
};
// f16: the conversions are the language's (v_cvt_f32_f16 / v_cvt_f16_f32, round to nearest even): what rounds beyond 65504 becomes
// +-inf, NaN stays NaN, a result below 2^-14 keeps its subnormal bits -- tensor.to(torch.float16) bit for bit.
template <> struct TileElem<1> {
    typedef f16x8_t frag_t;
    static __device__ __forceinline__ float lo(unsigned w) { return (float)__builtin_bit_cast(_Float16, (unsigned short)w); }
    static __device__ __forceinline__ float hi(unsigned w) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(w >> 16)); }
    static __device__ __forceinline__ unsigned rne(float x) { return __builtin_bit_cast(unsigned short, (_Float16)x); }
    static __device__ __forceinline__ f32x16_t mfma(frag_t a, frag_t b, f32x16_t c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
    }
};

template <int BN>
struct Bf16Tile {
    static constexpr int WN = BN / 2;                  // wave tile width
    static constexpr int NT = WN / 32;                 // 32-wide MFMA blocks per wave in N (2 or 1)
    static constexpr int LDS_A = kBf16BM * kBf16Pitch, LDS_B = BN * kBf16Pitch;
    static constexpr int STAGE_BYTES = (LDS_A + LDS_B) * 2;
    static constexpr int EPI_BYTES = 4 * 32 * WN * 4;  // per wave a 32 x WN f32 patch
    static constexpr int LDS_BYTES = STAGE_BYTES > EPI_BYTES ? STAGE_BYTES : EPI_BYTES;    // (the patches reuse the staging LDS)
    static constexpr int VEC_PER_ROW = WN / 8;         // 16-B output vectors per patch row
    static constexpr int VPL = 32 * VEC_PER_ROW / 64;  // epilogue vectors per lane and 32-row block
};

// the thread's place: its lane, and its wave's in the 2 (M) x 2 (N) arrangement
struct Bf16Wave {
    int lane, wave, wm, wn;
};
__device__ __forceinline__ Bf16Wave bf16_tile_wave() {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    return {lane, wave, wave >> 1, wave & 1};
}

// the workgroup's first row and column of the product [M][N]
struct Bf16TileOrigin {
    int m0, n0;
};
template <int BN>
__device__ __forceinline__ Bf16TileOrigin bf16_tile_origin(int N) {
    const int n_tiles = N / BN;
    // XCD-aware tile order: workgroup b runs on XCD b % 8 (each XCD has its own L2).  Give every XCD
    // a contiguous range of logical tile ids so that the N-tiles sharing one A row-block are
    // neighbours in time on ONE L2 instead of being fetched by eight (bijective for any grid size).
    const unsigned nwg = gridDim.x, xcd = blockIdx.x & 7u, in_xcd = blockIdx.x >> 3;
    const unsigned q = nwg >> 3, r8 = nwg & 7u;
    const unsigned logical = (xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q) + in_xcd;
    return {(int)(logical / n_tiles) * kBf16BM, (int)(logical % n_tiles) * BN};
}

// acc = A * W^T over K (a multiple of 64) for the tile whose first column is n0; W [N][K].  fetch_a(k0, ra): fill this thread's four
// staged 16-byte chunks of A for K-step k0 -- chunk column bf16_tile_stage(tid).col of the tile's rows p * 32 + bf16_tile_stage(tid).row.
// `smem`: Bf16Tile<BN>::LDS_BYTES, 16-byte aligned; free for the epilogue on return.
template <int BN, int DT = 2, typename FetchA>
__device__ __forceinline__ void bf16_tile_mainloop(unsigned char* smem, const unsigned short* W, int K, int n0,
                                                   f32x16_t (&acc)[2][Bf16Tile<BN>::NT], FetchA&& fetch_a) {
    constexpr int WN = Bf16Tile<BN>::WN, NT = Bf16Tile<BN>::NT;
    typedef typename TileElem<DT>::frag_t frag_t;
    unsigned short* sA = reinterpret_cast<unsigned short*>(smem);
    unsigned short* sB = sA + Bf16Tile<BN>::LDS_A;
    const int lane = bf16_tile_wave().lane, wm = bf16_tile_wave().wm, wn = bf16_tile_wave().wn;
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < NT; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0.0f;

    const int s_row = bf16_tile_stage(threadIdx.x).row, s_col = bf16_tile_stage(threadIdx.x).col;
    u32x4_t ra[kBf16Passes], rb[BN / 32];
    auto fetch = [&](int k0) {                 // global -> registers for K-step k0
        fetch_a(k0, ra);
#pragma unroll
        for (int p = 0; p < BN / 32; p++)
            rb[p] = *reinterpret_cast<const u32x4_t*>(W + (size_t)(n0 + p * 32 + s_row) * K + k0 + s_col);
    };
    fetch(0);
    for (int k0 = 0; k0 < K; k0 += kBf16BK) {
        __syncthreads();                       // previous step's fragment reads are done
#pragma unroll
        for (int p = 0; p < kBf16Passes; p++)
            *reinterpret_cast<u32x4_t*>(sA + (p * 32 + s_row) * kBf16Pitch + s_col) = ra[p];
#pragma unroll
        for (int p = 0; p < BN / 32; p++)
            *reinterpret_cast<u32x4_t*>(sB + (p * 32 + s_row) * kBf16Pitch + s_col) = rb[p];
        __syncthreads();
        if (k0 + kBf16BK < K) fetch(k0 + kBf16BK);   // the next K-step's operands travel while this one multiplies
#pragma unroll
        for (int kk = 0; kk < kBf16BK; kk += 16) {
            frag_t fa[2], fb[NT];
            const int kof = kk + (lane >> 5) * 8;
#pragma unroll
            for (int i = 0; i < 2; i++)
                fa[i] = *reinterpret_cast<const frag_t*>(sA + (wm * 64 + i * 32 + (lane & 31)) * kBf16Pitch + kof);
#pragma unroll
            for (int j = 0; j < NT; j++)
                fb[j] = *reinterpret_cast<const frag_t*>(sB + (wn * WN + j * 32 + (lane & 31)) * kBf16Pitch + kof);
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < NT; j++)
                    acc[i][j] = TileElem<DT>::mfma(fa[i], fb[j], acc[i][j]);
        }
    }
    __syncthreads();                           // staging LDS is free: reuse it for the epilogue
}

// this wave's 32 x WN float32 patch
template <int BN>
__device__ __forceinline__ float* bf16_tile_patch(unsigned char* smem) {
    return reinterpret_cast<float*>(smem) + bf16_tile_wave().wave * (32 * Bf16Tile<BN>::WN);
}

// C layout of a 32x32 accumulator block: element r of this lane is column lane & 31 of this row.  A kernel writes block j of a 32-row
// block of its wave tile, + its column's bias b, to the patch with
//     const int col = j * 32 + (lane & 31);
//     for (int r = 0; r < 16; r++) patch[bf16_tile_acc_row(r) * WN + col] = acc[i][j][r] + b;
// in its own body: there the sixteen stores compile to the very instructions they were before the kernels shared this header, which
// a function around the loop does not give (profiles/bf16_tile/README.md).
__device__ __forceinline__ int bf16_tile_acc_row(int r) { return (r & 3) + 8 * (r >> 2) + 4 * (bf16_tile_wave().lane >> 5); }

// between the patch's writes and its reads, and again before the next block's writes: the patch is the wave's own
__device__ __forceinline__ void bf16_tile_patch_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// The residual [M][N] of the i-th 32-row block of the wave tile, this lane's share: the vectors that bf16_tile_store_rows combines.
// It does not depend on the product, so a kernel fetches it early and its HBM latency hides behind the operand loads and the MFMAs.
template <int BN>
__device__ __forceinline__ void bf16_tile_fetch_residual(u32x4_t (&rpre)[Bf16Tile<BN>::VPL], const unsigned short* res, int M, int N,
                                                         int m0, int n0, int i) {
    constexpr int WN = Bf16Tile<BN>::WN, VEC_PER_ROW = Bf16Tile<BN>::VEC_PER_ROW;
    const int lane = bf16_tile_wave().lane, wm = bf16_tile_wave().wm, wn = bf16_tile_wave().wn;
#pragma unroll
    for (int t = 0; t < Bf16Tile<BN>::VPL; t++) {
        const int v = t * 64 + lane;
        const int row = v / VEC_PER_ROW, c8 = (v % VEC_PER_ROW) * 8;
        const int m = m0 + wm * 64 + i * 32 + row;
        rpre[t] = (u32x4_t){0u, 0u, 0u, 0u};
        if (m < M) rpre[t] = *reinterpret_cast<const u32x4_t*>(res + (size_t)m * N + n0 + wn * WN + c8);
    }
}

// The patch of the i-th 32-row block (+ the prefetched residual) -> relu -> the element type, round to nearest even -> out [M][N], in
// 16-byte vectors along the rows.  `relu` is the kernel's own form of max(x, 0); it is applied where RELU.
template <int BN, bool RES, bool RELU, int DT = 2, typename Relu>
__device__ __forceinline__ void bf16_tile_store_rows(const float* patch, const u32x4_t (&rpre)[Bf16Tile<BN>::VPL], unsigned short* out,
                                                     int M, int N, int m0, int n0, int i, Relu&& relu) {
    constexpr int WN = Bf16Tile<BN>::WN, VEC_PER_ROW = Bf16Tile<BN>::VEC_PER_ROW;
    typedef TileElem<DT> E;
    const int lane = bf16_tile_wave().lane, wm = bf16_tile_wave().wm, wn = bf16_tile_wave().wn;
#pragma unroll
    for (int t = 0; t < Bf16Tile<BN>::VPL; t++) {
        const int v = t * 64 + lane;
        const int row = v / VEC_PER_ROW, c8 = (v % VEC_PER_ROW) * 8;
        const int m = m0 + wm * 64 + i * 32 + row;
        if (m < M) {
            const size_t g = (size_t)m * N + n0 + wn * WN + c8;
            const float4 lo = *reinterpret_cast<const float4*>(patch + row * WN + c8);
            const float4 hi = *reinterpret_cast<const float4*>(patch + row * WN + c8 + 4);
            float f[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
            if (RES) {
                const u32x4_t rv = rpre[t];
#pragma unroll
                for (int q = 0; q < 4; q++) { f[2 * q] += E::lo(rv[q]); f[2 * q + 1] += E::hi(rv[q]); }
            }
            if (RELU) {
#pragma unroll
                for (int q = 0; q < 8; q++) f[q] = relu(f[q]);
            }
            u32x4_t ov;
#pragma unroll
            for (int q = 0; q < 4; q++) ov[q] = E::rne(f[2 * q]) | (E::rne(f[2 * q + 1]) << 16);
            *reinterpret_cast<u32x4_t*>(out + g) = ov;
        }
    }
}

}  // namespace opa
