// The unit mode of the 1x1 GEMM in bfloat16: the 1x1 convolutions of a ShuffleNetV2K / ShuffleNetV2 unit, conv5 and the heads of a
// network cast to bfloat16 (reference network/basenetworks.py:186-242), ONE v_mfma_f32_32x32x16_bf16 per product where the float32
// unit mode (csrc/gemm_f32x3.hip) spends six:
//     out[M, n]  = bf16_rne(act(A[M, k; row pitch lda] * W^T (float32 accumulate) + bias (+ residual[M, n; row pitch ldt])))
//     out[M, 2n]: out[m, 2c] = partner[m, c; row pitch ldt] (bits copied), out[m, 2c + 1] = the above           (with a partner)
// ANY even k and n; A, the partner and the residual may be channel slices of wider channels-last tensors.  W [Np][Kp] bf16 and
// bias [Np] float32 are padded with zeros on the host (Np, Kp: n, k rounded up to multiples of 64), `out` is dense.
//
// Tile shape, tile order, accumulator layout and patch fence are csrc/bf16_tile.hpp's (BN = 128 where Np allows, else 64).  The K
// loop below is that header's bf16_tile_mainloop written out: on the shared function this kernel's code changes, and one layer timed
// outside its range (profiles/bf16_tile/README.md), so it stays here, compiled to the bytes it had.  What differs from the other two
// kernels is how the operands are reached.  The contract guarantees 4-byte alignment only (k16's stage-2 slice starts 348 bytes into the
// pixel), so the width of A's loads -- 16, 8 or 4 bytes -- is chosen per launch from the base address and the pitch, uniformly for
// the grid; columns from k on are never loaded (their registers keep zeros: a select, not a product with a zero weight) and no byte
// behind column k of the last row is addressed.  Which bytes which thread loads is decided in csrc/unit_bf16_plan.hpp, which a CPU
// program enumerates (tests/test_unit_bf16_plan.py).  The epilogue works in column pairs: 4-byte loads of the partner / residual,
// 4-byte stores of the output (8-byte with a partner: its two elements and the two results interleaved).
//
// The same kernel serves a network cast to FLOAT16 (opa_gemm_unit_actp_f16): the element type is the leading template parameter DT, and
// only TileElem<DT> (csrc/bf16_tile.hpp) depends on it -- v_mfma_f32_32x32x16_f16 on f16x8 fragments, a residual element decoded and the
// result rounded by the language's conversions (round to nearest even; beyond 65504 +-inf, NaN stays NaN, subnormals kept).  Loads,
// staging, the epilogue's pairs and the partner's bits are raw 16-bit words for both types; the bfloat16 instantiations compile to the
// instructions they had (profiles/unit_f16/bf16_codegen.md).
#include "bf16_tile.hpp"
#include "unit_bf16_plan.hpp"

namespace opa {

namespace {

typedef __attribute__((ext_vector_type(2))) unsigned int u32x2_t;
typedef __attribute__((ext_vector_type(2))) float f32x2_t;

enum Third { kNone = 0, kPartner = 1, kResidual = 2 };

// N and K are the padded sizes (W [N][K], bias [N]); n, k the columns that exist; W_A the width of A's loads in bytes; DT the element
// type (the C ABI's dtype code: 2 bfloat16, 1 float16), which decides the fragment type, the MFMA, how a residual element becomes float32
// and how a result is rounded (TileElem<DT>) -- every operand travels as raw 16-bit words
template <int DT, int BN, int W_A, int THIRD>
__global__ __launch_bounds__(256, 3) void gemm_unit_bf16_kernel(
        const unsigned short* __restrict__ A, long long lda, const unsigned short* __restrict__ W, const float* __restrict__ bias,
        const unsigned short* __restrict__ third, long long ldt, unsigned short* __restrict__ out, int M, int N, int K, int n, int k,
        int act, float act_param) {
    using T = Bf16Tile<BN>;
    using E = TileElem<DT>;
    typedef typename E::frag_t frag_t;
    constexpr int WN = T::WN, NT = T::NT;
    __shared__ __attribute__((aligned(16))) unsigned char smem[T::LDS_BYTES];
    unsigned short* sA = reinterpret_cast<unsigned short*>(smem);
    unsigned short* sB = sA + T::LDS_A;

    const int tid = threadIdx.x, lane = bf16_tile_wave().lane, wave = bf16_tile_wave().wave;
    const int wm = bf16_tile_wave().wm, wn = bf16_tile_wave().wn;
    const Bf16TileOrigin org = bf16_tile_origin<BN>(N);
    const int m0 = org.m0, n0 = org.n0;

    f32x16_t acc[2][NT];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < NT; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0.0f;

    const int s_row = bf16_tile_stage(tid).row, s_col = bf16_tile_stage(tid).col;
    u32x4_t ra[kBf16Passes], rb[BN / 32];
    auto load_a = [&](int p, int e, long long at, int bytes) {     // (p, e and bytes are constants once the plan is unrolled)
        const unsigned short* src = A + at;
        if (bytes == 16) {
            ra[p] = *reinterpret_cast<const u32x4_t*>(src);
        } else if (bytes == 8) {
            const u32x2_t v = *reinterpret_cast<const u32x2_t*>(src);
            ra[p][e / 2] = v[0]; ra[p][e / 2 + 1] = v[1];
        } else {
            ra[p][e / 2] = *reinterpret_cast<const unsigned*>(src);
        }
    };
    auto fetch = [&](int k0) {                 // global -> registers for K-step k0
#pragma unroll
        for (int p = 0; p < kBf16Passes; p++) ra[p] = (u32x4_t){0u, 0u, 0u, 0u};
        // (a K-step that ends at or before k has whole pieces only: with k out of the way the plan's tail folds away)
        if (k0 + kBf16BK <= k) unit_bf16_plan_a<W_A>(M, 0x7fffffff, lda, m0, tid, k0, load_a);
        else unit_bf16_plan_a<W_A>(M, k, lda, m0, tid, k0, load_a);
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
                    acc[i][j] = E::mfma(fa[i], fb[j], acc[i][j]);
        }
    }
    __syncthreads();                           // staging LDS is free: reuse it for the epilogue

    // epilogue, one 32-row block of the wave tile at a time through a wave-private f32 patch, in column pairs
    constexpr int PPL = 32 * (WN / 2) / 64;    // pairs per lane and block (16 | 8)
    float* patch = reinterpret_cast<float*>(smem) + wave * (32 * WN);
    const int n0w = n0 + wn * WN;
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const long long m0w = (long long)m0 + wm * 64 + i * 32;
        unsigned tv[PPL];
        if (THIRD != kNone) {                  // the partner's / residual's pairs travel while the patch is written
#pragma unroll
            for (int t = 0; t < PPL; t++) tv[t] = 0u;
            unit_bf16_plan_third<WN>(M, n, ldt, m0w, n0w, lane, [&](int t, long long, int, long long at) {
                tv[t] = *reinterpret_cast<const unsigned*>(third + at);
            });
        }
#pragma unroll
        for (int j = 0; j < NT; j++) {
            const int col = j * 32 + (lane & 31);
            const float b = bias[n0w + col];
#pragma unroll
            for (int r = 0; r < 16; r++) patch[bf16_tile_acc_row(r) * WN + col] = acc[i][j][r] + b;
        }
        bf16_tile_patch_sync();
        unit_bf16_plan_third<WN>(M, n, ldt, m0w, n0w, lane, [&](int t, long long row, int col, long long) {
            f32x2_t f = *reinterpret_cast<const f32x2_t*>(patch + (int)(row - m0w) * WN + (col - n0w));
            if (THIRD == kResidual) { f[0] += E::lo(tv[t]); f[1] += E::hi(tv[t]); }
            f[0] = act_f32(f[0], act, act_param); f[1] = act_f32(f[1], act, act_param);
            const unsigned y0 = E::rne(f[0]), y1 = E::rne(f[1]);
            if (THIRD == kPartner)             // the partner's bits pass through untouched
                *reinterpret_cast<u32x2_t*>(out + (size_t)row * (2 * (size_t)n) + 2 * col) =
                    (u32x2_t){(tv[t] & 0xffffu) | (y0 << 16), (tv[t] >> 16) | (y1 << 16)};
            else
                *reinterpret_cast<unsigned*>(out + (size_t)row * n + col) = y0 | (y1 << 16);
        });
        bf16_tile_patch_sync();
        // (as in x3_unit_epilogue of gemm_f32x3.hip, whose column-pair epilogue this is: the compiler, too, keeps the next block's
        //  patch writes behind this block's patch reads -- the fence orders the memory, this the unrolled code)
        asm volatile("" ::: "memory");
    }
}

}  // namespace

// A [M, k] with `lda` elements between rows, W [Np][Kp] and bias [Np] padded with zeros, partner or residual [M, n] with `ldp` / `ldr`
// elements between rows or null (never both); out [M, n] dense, or [M, 2n] with a partner.  act 0 .. 4 is read at run time.
// dtype: 2 every 16-bit operand bfloat16, 1 float16 (the same kernel on v_mfma_f32_32x32x16_f16).
hipError_t launch_gemm_unit_act_bf16(const void* A, long long lda, const void* W, const float* bias, const void* partner, long long ldp,
                                     const void* residual, long long ldr, void* out, int M, int n, int k, int act, float act_param,
                                     hipStream_t st, int dtype) {
    if (dtype != 1 && dtype != 2) return hipErrorInvalidValue;
    if ((partner && residual) || act < 0 || act > 4 || (residual && act > 2) || M <= 0 || n <= 0 || k <= 0) return hipErrorInvalidValue;
    const int Np = (n + 63) / 64 * 64, Kp = (k + 63) / 64 * 64;
    const int bn = Np % 128 == 0 ? 128 : 64;
    const long long blocks = (long long)((M + (long long)kBf16BM - 1) / kBf16BM) * (Np / bn);
    if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
    const int third = partner ? kPartner : residual ? kResidual : kNone;
    const unsigned short* t = (const unsigned short*)(partner ? partner : residual);
    const long long ldt = partner ? ldp : residual ? ldr : 0;
    return with_value<2, 1>(dtype, [&](auto DT) {
    return with_value<64, 128>(bn, [&](auto BN) {
    return with_value<4, 8, 16>(unit_bf16_width((uintptr_t)A, lda), [&](auto W_A) {
    return with_value<(int)kNone, (int)kPartner, (int)kResidual>(third, [&](auto THIRD) {
        gemm_unit_bf16_kernel<DT, BN, W_A, THIRD><<<(unsigned)blocks, kBf16Threads, 0, st>>>(
            (const unsigned short*)A, lda, (const unsigned short*)W, bias, t, ldt, (unsigned short*)out, M, Np, Kp, n, k, act, act_param);
        return hipGetLastError();
    }); }); }); });
}

}  // namespace opa
