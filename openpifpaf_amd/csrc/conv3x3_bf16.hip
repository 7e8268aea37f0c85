// The 3x3 convolutions of a ResNet cast to bfloat16 (reference network/basenetworks.py:71-150: torchvision's BasicBlock and Bottleneck
// through torch.nn.Conv2d) as an implicit GEMM on v_mfma_f32_32x32x16_bf16, float32 accumulation, ONE rounding at the store:
//     out[b, oy, ox, co] = bf16_rne(act(sum_{ky,kx,ci} x[b, s*oy - d + d*ky, s*ox - d + d*kx, ci] * w[co][3*ky + kx][ci]
//                                       + bias[co] (+ residual[b, oy, ox, co])))
// x [B, h, w, c_in] dense channels-last bf16, w [c_out][9][c_in] bf16 (K-major, K = 9 c_in), bias float32 [c_out] or null, residual
// and out dense bf16 [B, ho, wo, c_out]; c_in % 64 == 0, c_out % 64 == 0, stride s 1 or 2, dilation d = padding 1, 2 or 4.
//
// Tile, fragments and epilogue are csrc/gemm_epilogue.hip's: 128 x BN per 256-thread workgroup (BN = 128 where c_out allows, else 64),
// BK = 64, 4 waves as 2 (M) x 2 (N), LDS rows 72 bf16 apart, the next K-step staged in registers while this one multiplies, XCD-aware
// tile order, the residual prefetched, a wave-private float32 patch in the epilogue with 16-byte stores.  What differs is A: a tap
// gather instead of a row of a matrix.  Which 16 bytes of which pixel a thread loads for a K-step -- or that it loads nothing, for a
// tap outside the image -- is decided in csrc/conv3x3_bf16_plan.hpp, which a CPU program enumerates
// (tests/test_conv3x3_bf16_plan.py); each staged row's centre pixel and 9-bit tap mask are computed once per workgroup.  No im2col
// buffer, no atomics (equal inputs give equal bits), no scratch.
#include "common.hpp"
#include "conv3x3_bf16_plan.hpp"

namespace opa {

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;

constexpr int kPitch = kConv3Bf16BK + 8;       // LDS row pitch in bf16 (gemm_epilogue.hip: fragment reads at <= 2-way conflicts)

__device__ __forceinline__ float bf16_lo(unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf16_hi(unsigned w) { return __uint_as_float(w & 0xffff0000u); }
__device__ __forceinline__ unsigned bf16_rne(float x) {
    unsigned u = __float_as_uint(x);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
    u += 0x7fffu + ((u >> 16) & 1u);
    return u >> 16;
}

// M = batch * ho * wo output pixels, N = c_out, K = 9 * c_in
template <int BN, bool RES, bool RELU>
__global__ __launch_bounds__(256, 3) void conv3x3_bf16_kernel(
        const unsigned short* __restrict__ x, const unsigned short* __restrict__ W, const float* __restrict__ bias,
        const unsigned short* __restrict__ res, unsigned short* __restrict__ out, Conv3Bf16Geometry g, int M, int N) {
    constexpr int WN = BN / 2;                 // wave tile width
    constexpr int NT = WN / 32;                // 32-wide MFMA blocks per wave in N (2 or 1)
    constexpr int LDS_A = kConv3Bf16BM * kPitch, LDS_B = BN * kPitch;
    constexpr int STAGE_BYTES = (LDS_A + LDS_B) * 2;
    constexpr int EPI_BYTES = 4 * 32 * WN * 4; // per wave a 32 x WN f32 patch
    __shared__ __attribute__((aligned(16))) unsigned char smem[STAGE_BYTES > EPI_BYTES ? STAGE_BYTES : EPI_BYTES];
    unsigned short* sA = reinterpret_cast<unsigned short*>(smem);
    unsigned short* sB = sA + LDS_A;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int n_tiles = N / BN;
    const int K = 9 * g.c_in;
    // XCD-aware tile order (see gemm_epilogue.hip): the N-tiles sharing one gathered row block run on ONE L2
    const unsigned nwg = gridDim.x, xcd = blockIdx.x & 7u, in_xcd = blockIdx.x >> 3;
    const unsigned q = nwg >> 3, r8 = nwg & 7u;
    const unsigned logical = (xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q) + in_xcd;
    const int m0 = (int)(logical / n_tiles) * kConv3Bf16BM;
    const int n0 = (int)(logical % n_tiles) * BN;

    f32x16_t acc[2][NT];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < NT; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0.0f;

    // the residual tile does not depend on the product: this lane's share travels behind the operand loads and the MFMAs
    constexpr int VEC_PER_ROW = WN / 8;        // 16-B output vectors per patch row
    constexpr int VPL = 32 * VEC_PER_ROW / 64; // epilogue vectors per lane and 32-row block
    u32x4_t rpre[2][VPL];
    auto fetch_residual = [&](int i) {
#pragma unroll
        for (int t = 0; t < VPL; t++) {
            const int v = t * 64 + lane;
            const int row = v / VEC_PER_ROW, c8 = (v % VEC_PER_ROW) * 8;
            const int m = m0 + wm * 64 + i * 32 + row;
            rpre[i][t] = (u32x4_t){0u, 0u, 0u, 0u};
            if (m < M) rpre[i][t] = *reinterpret_cast<const u32x4_t*>(res + (size_t)m * N + n0 + wn * WN + c8);
        }
    };
    if (RES) fetch_residual(0);                // the second half is fetched when the operand registers are free

    // staging map (conv3x3_bf16_plan.hpp): a 64-wide bf16 row is 8 chunks of 16 B; 256 threads cover 32 rows per pass
    const int s_row = tid >> 3, s_col = (tid & 7) * 8;
    Conv3Bf16Row rows[kConv3Bf16Passes];       // this thread's four output pixels: centre and tap mask, once per workgroup
    conv3x3_bf16_plan_rows(g, m0, tid, rows);
    u32x4_t ra[kConv3Bf16Passes], rb[BN / 32];
    auto load_a = [&](int p, long long at) { ra[p] = *reinterpret_cast<const u32x4_t*>(x + at); };
    auto fetch = [&](int k0) {                 // global -> registers for K-step k0; a tap outside the image keeps its zeros
#pragma unroll
        for (int p = 0; p < kConv3Bf16Passes; p++) ra[p] = (u32x4_t){0u, 0u, 0u, 0u};
        conv3x3_bf16_plan_a(g, rows, tid, k0, load_a);
#pragma unroll
        for (int p = 0; p < BN / 32; p++)
            rb[p] = *reinterpret_cast<const u32x4_t*>(W + (size_t)(n0 + p * 32 + s_row) * K + k0 + s_col);
    };
    fetch(0);
    for (int k0 = 0; k0 < K; k0 += kConv3Bf16BK) {
        __syncthreads();                       // previous step's fragment reads are done
#pragma unroll
        for (int p = 0; p < kConv3Bf16Passes; p++)
            *reinterpret_cast<u32x4_t*>(sA + (p * 32 + s_row) * kPitch + s_col) = ra[p];
#pragma unroll
        for (int p = 0; p < BN / 32; p++)
            *reinterpret_cast<u32x4_t*>(sB + (p * 32 + s_row) * kPitch + s_col) = rb[p];
        __syncthreads();
        if (k0 + kConv3Bf16BK < K) fetch(k0 + kConv3Bf16BK);   // the next K-step's operands travel while this one multiplies
#pragma unroll
        for (int kk = 0; kk < kConv3Bf16BK; kk += 16) {
            bf16x8_t fa[2], fb[NT];
            const int kof = kk + (lane >> 5) * 8;
#pragma unroll
            for (int i = 0; i < 2; i++)
                fa[i] = *reinterpret_cast<const bf16x8_t*>(sA + (wm * 64 + i * 32 + (lane & 31)) * kPitch + kof);
#pragma unroll
            for (int j = 0; j < NT; j++)
                fb[j] = *reinterpret_cast<const bf16x8_t*>(sB + (wn * WN + j * 32 + (lane & 31)) * kPitch + kof);
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < NT; j++)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
    }
    __syncthreads();                           // staging LDS is free: reuse it for the epilogue
    if (RES) fetch_residual(1);

    // epilogue, one 32-row block of the wave tile at a time through a wave-private f32 patch
    float* patch = reinterpret_cast<float*>(smem) + wave * (32 * WN);
#pragma unroll
    for (int i = 0; i < 2; i++) {
#pragma unroll
        for (int j = 0; j < NT; j++) {
            const int col = j * 32 + (lane & 31);
            const float b = bias ? bias[n0 + wn * WN + col] : 0.0f;
#pragma unroll
            for (int r = 0; r < 16; r++) {     // C layout: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
                const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                patch[row * WN + col] = acc[i][j][r] + b;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int t = 0; t < VPL; t++) {
            const int v = t * 64 + lane;
            const int row = v / VEC_PER_ROW, c8 = (v % VEC_PER_ROW) * 8;
            const int m = m0 + wm * 64 + i * 32 + row;
            if (m < M) {
                const size_t at = (size_t)m * N + n0 + wn * WN + c8;
                const float4 lo = *reinterpret_cast<const float4*>(patch + row * WN + c8);
                const float4 hi = *reinterpret_cast<const float4*>(patch + row * WN + c8 + 4);
                float f[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
                if (RES) {
                    const u32x4_t rv = rpre[i][t];
#pragma unroll
                    for (int e = 0; e < 4; e++) { f[2 * e] += bf16_lo(rv[e]); f[2 * e + 1] += bf16_hi(rv[e]); }
                }
                if (RELU) {                    // (a select: NaN stays NaN)
#pragma unroll
                    for (int e = 0; e < 8; e++) f[e] = f[e] < 0.0f ? 0.0f : f[e];
                }
                u32x4_t ov;
#pragma unroll
                for (int e = 0; e < 4; e++) ov[e] = bf16_rne(f[2 * e]) | (bf16_rne(f[2 * e + 1]) << 16);
                *reinterpret_cast<u32x4_t*>(out + at) = ov;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

}  // namespace

long long conv3x3_bf16_workgroups(int B, int H, int W, int c_out, int S) {
    const long long M = (long long)B * conv3x3_bf16_out(H, S) * conv3x3_bf16_out(W, S);
    return (M + kConv3Bf16BM - 1) / kConv3Bf16BM * (c_out / (c_out % 128 == 0 ? 128 : 64));
}

hipError_t launch_conv3x3_bf16(const void* x, const void* w, const float* bias, const void* residual, void* out, int B, int H, int W,
                               int c_in, int c_out, int S, int D, int relu, hipStream_t st) {
    if (B <= 0 || H <= 0 || W <= 0 || c_in <= 0 || c_out <= 0 || c_in % 64 != 0 || c_out % 64 != 0 || (S != 1 && S != 2) ||
        (D != 1 && D != 2 && D != 4) || (D > 1 && S != 1))
        return hipErrorInvalidValue;
    const long long M = (long long)B * conv3x3_bf16_out(H, S) * conv3x3_bf16_out(W, S);
    const long long blocks = conv3x3_bf16_workgroups(B, H, W, c_out, S);
    if ((long long)B * H * W * c_in > 0x7fffffffll || M * c_out > 0x7fffffffll || blocks > 0x7fffffffll) return hipErrorInvalidValue;
    const Conv3Bf16Geometry g = {B, H, W, c_in, S, D};
    return with_value<64, 128>(c_out % 128 == 0 ? 128 : 64, [&](auto BN) {
    return with_flag(residual != nullptr, [&](auto RES) {
    return with_flag(relu != 0, [&](auto RELU) {
        conv3x3_bf16_kernel<BN, RES, RELU><<<(unsigned)blocks, kConv3Bf16Threads, 0, st>>>(
            (const unsigned short*)x, (const unsigned short*)w, bias, (const unsigned short*)residual, (unsigned short*)out, g, (int)M, c_out);
        return hipGetLastError();
    }); }); });
}

}  // namespace opa
