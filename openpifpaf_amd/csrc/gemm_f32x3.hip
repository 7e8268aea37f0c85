// The float32 1x1 convolution on the bf16 MFMA pipe, without giving up a bit of either operand:
//     out[M,N] = act( A[M,K] * W[N,K]^T + bias[N] (+ residual[M,N]) )        (f32 in, f32 out, f32 accumulators)
// gfx950 has no TF32 and its float32 MFMA (v_mfma_f32_32x32x2f32) runs at 1/16 of the bf16 rate (157 against 2 500 TFLOP/s
// dense), so the compute-bound 1x1 convolutions of ResNet layers 3-4 sit at 115-118 TFLOP/s however the kernel around them
// is built (gemm_f32.hip).  A float32 number is, exactly, the sum of three bfloat16 numbers: its 24-bit
// significand cut into 8 + 8 + 8 bits (a1 = a with the low 16 bits cleared, r = a - a1, a2 = r with the low 16 bits cleared,
// a3 = r - a2: every step exact, every piece representable -- bf16 has float32's exponent range -- from |a| = 2^-110 up; what
// becomes of smaller numbers, of +-Inf (NaN: the split's Inf - Inf) and of NaN is stated in split_bf16.hpp and at the end of this
// header).  So
//     a * b = sum over i, j of a_i * b_j                                       (nine products, each EXACT in float32:
// 8 x 8 significand bits), and v_mfma_f32_32x32x16_bf16 forms and accumulates them in float32 like the float32 MFMA
// accumulates its own exact products.  TERMS = 9: all of them -- the GEMM's only rounding is the accumulation's, as in
// any float32 GEMM.  TERMS = 6: without a2*b3, a3*b2, a3*b3 (below 2^-23 of the product each).  The leading products
// a1*b1 and the corrections go to accumulators of their own (the corrections are 2^-8 and less of the sum: added
// among themselves first they are not rounded away against it), joined in the epilogue.
// Nine bf16 MFMAs of 8 passes against eight float32 MFMAs of 16 passes per 32x32x16 block: 0.56 of the MFMA time
// (six: 0.375).  The split costs ~5.5 VALU instructions per operand element, once per element and tile: the weight is
// split on the host, once ([3][N][K] bf16, openpifpaf_amd.fused.split_weight), the activation while its tile is staged.
// Error against a float64 product: tests/test_gpu_gemm_x3.py, tools/gpu/gemm_x3_probe.py (both variants next to
// gemm_f32.hip's float32 MFMA and torch's float32 convolution): six terms 2.4-2.8x BELOW the float32 MFMA's.
// Measured (profiles/r6/gemm_x3_probe.log, gemm_x3_pmc.log): 0.62 ms against 0.93 on the layer-3 reduce shape; the kernel is
// POWER-limited -- the clock falls to 1.8 GHz and the bf16 MFMA sustains 1.0e9 busy cycles per second per SIMD with six and with
// nine terms alike, so MFMA time adds to the launch however well the rest overlaps.
// The same kernel takes a SECOND activation along K (SRC = 1: a block's last 1x1 convolution + its downsampling convolution as
// one product) or NINE / EIGHT shifted views of one activation (SRC = 2: strided 3x3 convolutions and the 7x7 stem as implicit
// GEMMs; padding through out-of-range buffer offsets).
//
// Tile 128 x BN (BN = 128 | 64) per 256-thread workgroup, BK = 32; 4 waves as 2(M) x 2(N), a wave 64 x BN/2 of 32x32
// blocks; operands K-major in LDS, three bf16 planes each, rows of 64 B whose 16-byte chunks are XOR-swizzled by (row / 4) % 4
// (ds_read_b128 fragments of 16 consecutive rows fall on 16 different bank groups AND the 8-byte plane stores of the split do
// not collide: with rows padded to 80 B a third of the LDS cycles were store conflicts; profiles/r6/gemm_x3_swizzle_ab.log:
// 2-7 % on the reduce shapes); XCD-aware tile order and epilogue as in gemm_f32.hip.
// A third tile, 128 x 256 per 512-thread workgroup, for launches of six terms with N % 256 == 0 that are large enough for it:
// gemm_f32x3_wide_kernel, further down, with a header of its own.
// Block tails (RES): the last two K-steps used to request the last tile again (unconditional loads, nothing read them); the residual
// of epilogue block 0 travels in those slots, block 1's from the epilogue's entry, the bias waits in LDS: layer-3 tail 0.81 -> 0.66 ms.
//
// Non-finite and tiny operands (tests/test_gpu_x3_edges.py): a NaN or +-Inf element of A makes its output ROW
// NaN, one of W its output COLUMN (a float32 GEMM gives +-Inf for an Inf operand: the split turns Inf into (Inf, NaN, NaN));
// Inf in the bias or the residual arrives as Inf.  Every other element of the tile is bit for bit what it is without that
// value.  fmaxf returns its other argument for a NaN: ReLU stores NaN, +0 or +Inf there, and the prologue turns a NaN (or -Inf)
// activation into 0 before the split.  The stem's eighth window row and column meet zero weights, so a non-finite pixel
// reaches every output whose 8x8 window holds it (0 x Inf), not the 7x7 ones alone: written down and pinned by a test.  Operands below 2^-110: see split_bf16.hpp; an element loses less than
// 2^-125 sum_k (|a_mk| + |w_nk|).
#include <cstdlib>
#include <type_traits>
#include "common.hpp"
#include "split_bf16.hpp"

namespace opa {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2_t;
typedef __attribute__((ext_vector_type(2))) float f32x2_t;

#ifndef OPA_X3_BK                  // tuning switches (tools/gpu/gemm_x3_probe.py builds the variants): K-step,
#define OPA_X3_BK 32               // workgroups per compute unit the registers are budgeted for,
#endif
#ifndef OPA_X3_WGS
#define OPA_X3_WGS 2
#endif
#ifndef OPA_X3_DIAG                // timing experiments (WRONG results): 1 no split arithmetic, 2 no LDS stores in the K loop,
#define OPA_X3_DIAG 0              // 3 only the leading MFMA of every block, 4 fragments read once per K-step (kk = 0 only)
#endif
#ifndef OPA_X3_ONE_ACC             // 1: the corrections go to the leading products' accumulators (64 registers less)
#define OPA_X3_ONE_ACC 0
#endif
#ifndef OPA_X3_SWIZZLE             // 1: LDS rows without padding, the 16-byte chunks of a row XOR-swizzled by (row / 4) % 4: fragment
#define OPA_X3_SWIZZLE 1           //    reads of 16 consecutive rows AND the 8-byte plane stores of the split fall on distinct banks
#endif                             //    (0: rows 80 bytes apart -- the stores collide two-way, a third of the LDS cycles, profiles/r6/gemm_x3_pmc.log)
constexpr int kX3BM = 128, kX3BK = OPA_X3_BK, kX3Pitch = OPA_X3_SWIZZLE ? kX3BK : kX3BK + 8;      // LDS row pitch in bf16
// bf16 offset of element k (a multiple of 4) of row `row` in a plane
__device__ __forceinline__ int x3_lds(int row, int k) {
    if (OPA_X3_SWIZZLE && kX3BK == 32) return row * kX3Pitch + ((((k >> 3) ^ (row >> 2)) & 3) << 3) + (k & 7);
    return row * kX3Pitch + k;
}

// A SECOND activation behind the first along K (TWO): out = act([A | A2'] * W^T + bias) with A2'[m] = the pixel of A2 that
// output pixel m reads through a 1x1 convolution of stride `stride` -- the last 1x1 convolution of a ResNet block and the
// block's downsampling convolution as ONE product (the weights concatenated along K on the host), so that the identity tensor
// is neither written nor read back.  Columns [0, K1) come from A (row length K1), [K1, K) from A2 (row length K - K1).
// NINE activations along K (SRC = 2): a 3x3 convolution with padding 1 and any stride as an implicit GEMM -- column block
// t = 3 ky + kx of K holds the C channels of input pixel (stride * oy - 1 + ky, stride * ox - 1 + kx); a pixel in the padding is
// requested beyond the end of the buffer, which a buffer load answers with zeros (one bit per row and tap decides).  With a
// dilation d (padding d) the pixel is (stride * oy - d + d ky, stride * ox - d + d kx): the same three expressions times d.
// The defaults are what a mode that does not read a field passes: a launcher sets the fields of its own mode, nothing else.
struct X3Second {
    const float* A2 = nullptr; // (SRC = 1) [B, hi, wi, K - K1] channels-last
    int K1 = 0;                // (SRC = 1) columns of the first activation (a multiple of the K-step)
    int ho_wo = 1, wo = 1, hi_wi = 1, wi = 1, stride = 1;        // (SRC = 1, 2) output pixels per image and row, input ones, the stride
    int hi = 1, C = 0, batch = 1;     // (SRC = 2) input rows, floats per tap (a multiple of the K-step), images
    int pix = 1, taps_x = 1, ntaps = 1, padded = 0;   // (SRC = 2) floats per input pixel; taps per window row; taps; 1: the input is padded in
                               // memory (window origin = (stride oy, stride ox), every tap valid), 0: padding `dil` by the tap mask
    int dil = 1;               // (SRC = 2, not padded) dilation d: tap (ky, kx) reads input pixel (stride oy - d + d ky, stride ox - d + d kx)
    int lda = 0, ldp = 0, n_real = 0, k_real = 0;     // (UNIT) floats between rows of A and of the partner; the columns that exist of N and K
    int act = 0; float act_param = 0.0f;     // (UNIT, kUxActParam) the activation read at run time: 3 LeakyReLU(slope), 4 clipped ReLU(cap)
};

// UNIT: the 1x1 convolutions of a ShuffleNetV2K unit (reference network/basenetworks.py:186-242) -- ANY even K and N, A a channel
// slice of a wider tensor, the output optionally stored into its shuffled position:
//     out[M, n] = act(A[M, k; row pitch lda] * W^T + bias)                                    (RES = false)
//     out[M, 2n]: out[m, 2c] = partner[m, c; row pitch ldp], out[m, 2c + 1] = act(...)[c]     (RES = true: `res` is the partner)
// = channel_shuffle(cat((partner, y), 1), 2), written as contiguous rows.  The kernel's N and K are the PADDED sizes (W3
// [3][N][K] and bias [N] are padded with zeros on the host: N to the tile width, K to two K-steps); sec.n_real / sec.k_real are
// the columns that exist.  Zeros in the weight do not cancel what lies behind column k_real of a row of A (the next pixel, the
// other half of this one: 0 x Inf is NaN), so those columns are replaced by zeros with a select before the split, and what lies
// behind the LAST row is never fetched (the buffer's range ends with that row's column k_real).  A slice starts on an 8-byte
// boundary only (k16 stage 2: 174 floats into a pixel) and so does every row of the output (n_real even): the operand is staged
// with 8-byte loads, the epilogue works in column pairs -- a pair lies inside k_real / n_real or outside, never across.
// UX (MobileNetV3's blocks, reference network/basenetworks.py:432-446; 0 for everything above): (UX & kUxAct) == kUxHardswish -- the
// activation is hardswish (RELU false); UX & kUxResidual -- `partner` is a RESIDUAL [M, n; row pitch ldp]:
// out[M, n] = act(A * W^T + bias + residual), dense rows.
// UX & kUxActParam (MobileNetV2's ReLU6, reference network/basenetworks.py:407-430, and the LeakyReLU of a ShuffleNetV2K unit, :186-268; RELU
// false, never with a residual): the activation is read at run time -- `act` 3: x < 0 ? x * p : x, 4: x < 0 ? 0 : (x > p ? p : x),
// p = `act_param` -- both selects, so that NaN stays NaN (x3_act_param of common.hpp, which csrc/stem.hip shares); one pair of
// instantiations serves both, the epilogue is not where the time goes.
constexpr int kUxAct = 3, kUxHardswish = 2, kUxResidual = 4, kUxActParam = 8;      // (the values are part of the kernels' names)

template <int BN, bool PARTNER, bool RELU, int UX = 0>
__device__ __forceinline__ void x3_unit_epilogue(float* smem_f, const f32x16_t (&acc)[2][BN / 64], const f32x16_t (&low)[2][BN / 64],
                                                 const float* __restrict__ bias, const float* __restrict__ partner,
                                                 float* __restrict__ out, int M, int m0, int n0, int lane, int wave, int ldp, int n_real,
                                                 int act, float act_param) {
    constexpr int WN = BN / 2, NT = WN / 32;
    constexpr int PPR = WN / 2;                // column pairs of a patch row
    constexpr int PPL = 32 * PPR / 64;         // ... per lane (16 | 8)
    constexpr int PPRE = PPL > 8 ? 8 : PPL;    // partner pairs fetched ahead (16 registers); the rest in the loop
    const int wm = wave >> 1, wn = wave & 1;
    float* patch = smem_f + wave * (32 * WN);
#pragma unroll
    for (int i = 0; i < 2; i++) {
        f32x2_t pv[PPRE];
        if (PARTNER) {                         // they travel while the patch is written
#pragma unroll
            for (int t = 0; t < PPRE; t++) {
                const int v = t * 64 + lane;
                const int row = v / PPR, col = n0 + wn * WN + (v % PPR) * 2;
                const int m = m0 + wm * 64 + i * 32 + row;
                pv[t] = (f32x2_t){0.f, 0.f};
                if (m < M && col < n_real) pv[t] = *reinterpret_cast<const f32x2_t*>(partner + (size_t)m * ldp + col);
            }
        }
#pragma unroll
        for (int j = 0; j < NT; j++) {
            const int col = j * 32 + (lane & 31);
            const float b = bias[n0 + wn * WN + col];
#pragma unroll
            for (int r = 0; r < 16; r++) {     // C layout: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
                const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                patch[row * WN + col] = (OPA_X3_ONE_ACC ? acc[i][j][r] : acc[i][j][r] + low[i][j][r]) + b;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int t = 0; t < PPL; t++) {
            const int v = t * 64 + lane;
            const int row = v / PPR, c2 = (v % PPR) * 2, col = n0 + wn * WN + c2;
            const int m = m0 + wm * 64 + i * 32 + row;
            if (m < M && col < n_real) {       // (n_real is even: the pair is inside or outside)
                f32x2_t f = *reinterpret_cast<const f32x2_t*>(patch + row * WN + c2);
                if constexpr (PARTNER && (UX & kUxResidual) != 0) {
                    f32x2_t pp;
                    if (t < PPRE) pp = pv[t < PPRE ? t : 0];
                    else pp = *reinterpret_cast<const f32x2_t*>(partner + (size_t)m * ldp + col);
                    f[0] += pp[0]; f[1] += pp[1];
                }
                if (RELU) { f[0] = fmaxf(f[0], 0.0f); f[1] = fmaxf(f[1], 0.0f); }
                if constexpr ((UX & kUxAct) == kUxHardswish) { f[0] = hardswish_f32(f[0]); f[1] = hardswish_f32(f[1]); }
                if constexpr ((UX & kUxActParam) != 0) { f[0] = x3_act_param(f[0], act, act_param); f[1] = x3_act_param(f[1], act, act_param); }
                if (PARTNER && (UX & kUxResidual) == 0) { // the partner's bits pass through untouched
                    f32x2_t pp;
                    if (t < PPRE) pp = pv[t < PPRE ? t : 0];
                    else pp = *reinterpret_cast<const f32x2_t*>(partner + (size_t)m * ldp + col);
                    *reinterpret_cast<f32x4_t*>(out + (size_t)m * (2 * (size_t)n_real) + 2 * col) = (f32x4_t){pp[0], f[0], pp[1], f[1]};
                } else {
                    *reinterpret_cast<f32x2_t*>(out + (size_t)m * n_real + col) = f;
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        asm volatile("" ::: "memory");
    }
}

template <int BN, bool RES, bool RELU, bool PRO, int TERMS, int SRC, bool UNIT = false, int UX = 0>
__global__ __launch_bounds__(256, OPA_X3_WGS) void gemm_f32x3_bias_act_kernel(
        const float* __restrict__ A, const unsigned short* __restrict__ W3, const float* __restrict__ bias,
        const float* __restrict__ res, float* __restrict__ out, int M, int N, int K, const float* __restrict__ a_bias,
        const X3Second sec) {
    constexpr int WN = BN / 2;                 // wave tile width
    constexpr int NT = WN / 32;                // 32-wide MFMA blocks per wave in N (2 or 1)
    constexpr int LDS_A = kX3BM * kX3Pitch, LDS_B = BN * kX3Pitch;        // bf16 elements of ONE plane
#ifndef OPA_X3_PAD_LDS            // experiment: this many bytes of LDS more (fewer workgroups per compute unit)
#define OPA_X3_PAD_LDS 0
#endif
    constexpr int STAGE_BYTES = 3 * (LDS_A + LDS_B) * 2 + OPA_X3_PAD_LDS;
    constexpr int EPI_BYTES = 4 * 32 * WN * 4; // per wave a 32 x WN f32 patch
    // (a block tail keeps its BN bias values behind the stages: read with ds_read in the epilogue they do not share a counter with
    //  the residual vectors in flight -- as a global load there, the wait for the bias was a wait for every residual vector requested before it)
    constexpr int SMEM_BYTES = STAGE_BYTES > EPI_BYTES ? STAGE_BYTES : EPI_BYTES;
    __shared__ __attribute__((aligned(16))) unsigned char smem[SMEM_BYTES + (RES && !UNIT ? BN * 4 : 0)];
    unsigned short* sA = reinterpret_cast<unsigned short*>(smem);          // [3][128][pitch]
    unsigned short* sB = sA + 3 * LDS_A;                                    // [3][BN][pitch]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int n_tiles = N / BN;
    // XCD-aware tile order (see gemm_epilogue.hip): the N-tiles sharing one A row-block run on ONE L2
    const unsigned nwg = gridDim.x, xcd = blockIdx.x & 7u, in_xcd = blockIdx.x >> 3;
    const unsigned q = nwg >> 3, r8 = nwg & 7u;
    const unsigned logical = (xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q) + in_xcd;
    const int m0 = (int)(logical / n_tiles) * kX3BM;
    const int n0 = (int)(logical % n_tiles) * BN;

    constexpr int NL = OPA_X3_ONE_ACC ? 1 : 2;
    f32x16_t acc[2][NT], low_[NL][NT];         // the leading products a1*b1; everything else
    f32x16_t (&low)[2][NT] = OPA_X3_ONE_ACC ? acc : reinterpret_cast<f32x16_t (&)[2][NT]>(low_);
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < NT; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) { acc[i][j][r] = 0.0f; if (!OPA_X3_ONE_ACC) low[i][j][r] = 0.0f; }

    // staging maps.  A: a 32-float row is 8 x 16 B, 256 threads cover 32 rows per pass.  W3: a 32-bf16 row of one plane is
    // 4 x 16 B; vector v of the 3 * BN * 4 of a K-step = (plane, row, quarter)
    constexpr int VA = kX3BK / 4;              // 16-B vectors of an A row (8 | 4)
    constexpr int RPP = 256 / VA;              // A rows per pass (32 | 64)
    constexpr int NPA = kX3BM / RPP;           // passes (4 | 2)
    constexpr int WQ = kX3BK / 8;              // 16-B vectors of a W row of one plane (4 | 2)
    const int s_row = tid / VA, s_col = (tid % VA) * 4;
    constexpr int WTOT = 3 * BN * WQ;          // W vectors of a K-step
    constexpr int WV = (WTOT + 255) / 256;     // ... per thread
    f32x4_t ra0[NPA], ra1[NPA];                // the activation travels TWO K-steps ahead (HBM), the weight one (L2)
    u32x4_t rb[WV];
    // uniform 64-bit bases (scalar registers) + one 32-bit offset per load: the loads keep their address registers to
    // themselves (with 64-bit per-thread pointers the compiler, short of registers, computed every address INTO the load's
    // destination, which made each K-step wait for all loads in flight before it could issue its own)
    // (buffer loads: a descriptor in scalar registers, ONE 32-bit byte offset per load, the K-step as the scalar offset)
    constexpr bool TWO = SRC == 1, TAPS = SRC == 2;
    const int rows_here = M - m0 < kX3BM ? M - m0 : kX3BM;
    const int KA = TWO ? sec.K1 : TAPS ? sec.C : UNIT ? sec.lda : K;      // row length of the first activation (UNIT: its row pitch)
    // (TAPS: the whole tensor, from d (wi + 1) pixels BEFORE its start -- the window of output pixel (oy, ox) begins at input pixel
    //  (stride oy - d, stride ox - d); what lies before the tensor is only ever asked for by rows whose tap bit is clear)
    const int shift = TAPS && !sec.padded ? sec.dil * (sec.wi + 1) * sec.pix : 0;
    const float* a1_base = TAPS ? A - (size_t)shift : A + (size_t)m0 * KA;
    const int a1_bytes = TAPS ? (int)(((size_t)sec.batch * sec.hi_wi * sec.pix + shift) * 4)
                       : UNIT ? (int)(((size_t)(rows_here - 1) * KA + sec.k_real) * 4) : (int)((size_t)rows_here * KA * 4);
    const __amdgpu_buffer_rsrc_t a_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a1_base), 0, a1_bytes, 0x00020000);
    // the second activation: its rows are the input pixels the tile's output pixels read (monotonic in m: offsets from the first)
    const int K2 = K - KA;
    auto in_row = [&](int m) -> long long {
        const int b = m / sec.ho_wo, r = m - b * sec.ho_wo, oy = r / sec.wo, ox = r - oy * sec.wo;
        return (long long)b * sec.hi_wi + (long long)oy * sec.stride * sec.wi + (long long)ox * sec.stride;
    };
    long long row0_2 = 0;
    const float* a2_base = nullptr;
    int a2_bytes = 0;
    unsigned pa2[NPA];
    if constexpr (TWO) {
        row0_2 = in_row(__builtin_amdgcn_readfirstlane(m0));
        const int m_end = m0 + rows_here - 1;
        a2_base = sec.A2 + (size_t)row0_2 * K2;
        a2_bytes = (int)((size_t)(in_row(__builtin_amdgcn_readfirstlane(m_end)) - row0_2 + 1) * K2 * 4);
    }
    const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<unsigned short*>(W3 + (size_t)n0 * K), 0, (int)(((size_t)3 * N - n0) * K * 2), 0x00020000);
    unsigned pa[NPA], pb[WV];
    unsigned vmask[NPA];                       // (TAPS) bit t: tap t of this row lies inside the image
    int sb_off[WV];
#pragma unroll
    for (int p = 0; p < NPA; p++) {            // rows past M read row M - 1 (valid memory; the epilogue never stores them)
        int m = m0 + p * RPP + s_row;
        if (m > M - 1) m = M - 1;
        pa[p] = ((unsigned)(m - m0) * (unsigned)KA + (unsigned)s_col) * 4u;
        vmask[p] = 0u;
        if constexpr (TAPS) {
            const int b = m / sec.ho_wo, r = m - b * sec.ho_wo, oy = r / sec.wo, ox = r - oy * sec.wo;
            pa[p] = (unsigned)((long long)b * sec.hi_wi + (long long)oy * sec.stride * sec.wi + (long long)ox * sec.stride) * (unsigned)sec.pix * 4u
                    + (unsigned)s_col * 4u;
            if (sec.padded) vmask[p] = 0xffffffffu;
            else
                for (int t = 0; t < sec.ntaps; t++) {
                    const int iy = oy * sec.stride - sec.dil + sec.dil * (t / sec.taps_x), ix = ox * sec.stride - sec.dil + sec.dil * (t % sec.taps_x);
                    if (iy >= 0 && iy < sec.hi && ix >= 0 && ix < sec.wi) vmask[p] |= 1u << t;
                }
        }
        if constexpr (TWO) pa2[p] = ((unsigned)(in_row(m) - row0_2) * (unsigned)K2 + (unsigned)s_col) * 4u;
    }
#pragma unroll
    for (int t = 0; t < WV; t++) {
        const int v = t * 256 + tid < WTOT ? t * 256 + tid : WTOT - 1;     // (a thread without a vector of its own repeats the last one)
        const int plane = v / (BN * WQ), rem = v - plane * (BN * WQ), row = rem / WQ, c = (rem % WQ) * 8;
        pb[t] = (((unsigned)plane * (unsigned)N + (unsigned)row) * (unsigned)K + (unsigned)c) * 2u;
        sb_off[t] = plane * LDS_B + x3_lds(row, c);
    }
    auto fetch_a = [&](f32x4_t (&ra)[NPA], int k0) {      // global -> registers for K-step k0 (with the operand prologue)
        if constexpr (TAPS) {                  // tap t = k0 / C: a uniform shift of every row's window origin
            const int t = k0 / KA, kc = k0 - t * KA;
            // (unsigned: the offset of a tap that no row can reach -- a dilation beyond the image -- may wrap; its bit is clear in every row)
            const int soff = (int)((((unsigned)(sec.dil * (t / sec.taps_x)) * (unsigned)sec.wi + (unsigned)(sec.dil * (t % sec.taps_x))) * (unsigned)sec.pix + (unsigned)kc) * 4u);
#pragma unroll
            for (int p = 0; p < NPA; p++)
                ra[p] = __builtin_bit_cast(f32x4_t, __builtin_amdgcn_raw_buffer_load_b128(a_rsrc, (vmask[p] >> t) & 1u ? pa[p] : 0xFFFFFFF0u, soff, 0));
        } else if constexpr (TWO) {            // (uniform selects, no branch around the loads)
            const bool second = k0 >= KA;
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<float*>(second ? a2_base : a1_base), 0, second ? a2_bytes : a1_bytes, 0x00020000);
            const int ks = (second ? k0 - KA : k0) * 4;
#pragma unroll
            for (int p = 0; p < NPA; p++)
                ra[p] = __builtin_bit_cast(f32x4_t, __builtin_amdgcn_raw_buffer_load_b128(rs, second ? pa2[p] : pa[p], ks, 0));
        } else if constexpr (UNIT) {           // rows on 8-byte boundaries: two 8-byte loads per vector (where the compiler can prove
                                               // them adjacent it merges them into one 16-byte load, which needs dword alignment only:
                                               // tests/test_gpu_unit_gemm.py runs k16's slice, 8 bytes off a 16-byte boundary)
#pragma unroll
            for (int p = 0; p < NPA; p++) {
                const f32x2_t lo = __builtin_bit_cast(f32x2_t, __builtin_amdgcn_raw_buffer_load_b64(a_rsrc, pa[p], k0 * 4, 0));
                const f32x2_t hi = __builtin_bit_cast(f32x2_t, __builtin_amdgcn_raw_buffer_load_b64(a_rsrc, pa[p] + 8u, k0 * 4, 0));
                ra[p] = (f32x4_t){lo[0], lo[1], hi[0], hi[1]};
            }
        } else {
#pragma unroll
            for (int p = 0; p < NPA; p++) ra[p] = __builtin_bit_cast(f32x4_t, __builtin_amdgcn_raw_buffer_load_b128(a_rsrc, pa[p], k0 * 4, 0));
        }
        if (PRO) {                             // the preceding convolution's bias + ReLU, applied to the raw operand
            const f32x4_t ab = *reinterpret_cast<const f32x4_t*>(a_bias + k0 + s_col);
#pragma unroll
            for (int p = 0; p < NPA; p++)
#pragma unroll
                for (int e = 0; e < 4; e++) ra[p][e] = fmaxf(ra[p][e] + ab[e], 0.0f);
        }
    };
    auto fetch_b = [&](int k0) {
#pragma unroll
        for (int t = 0; t < WV; t++) rb[t] = __builtin_bit_cast(u32x4_t, __builtin_amdgcn_raw_buffer_load_b128(w_rsrc, pb[t], k0 * 2, 0));
    };
    auto store = [&](const f32x4_t (&ra)[NPA], int kt) {  // registers -> LDS: the activation (of K-step kt) is split here, once per element and tile
#pragma unroll
        for (int p = 0; p < NPA; p++) {
            u32x2_t p1, p2, p3;
            if (OPA_X3_DIAG == 1) { p1[0] = __float_as_uint(ra[p][0]); p1[1] = __float_as_uint(ra[p][2]); p2 = p1; p3 = p1; }
            else if constexpr (UNIT) {         // columns from k_real on are zeros WHATEVER the memory behind the row holds (a select)
                const bool in0 = kt + s_col < sec.k_real, in1 = kt + s_col + 2 < sec.k_real;
                const f32x4_t v = {in0 ? ra[p][0] : 0.0f, in0 ? ra[p][1] : 0.0f, in1 ? ra[p][2] : 0.0f, in1 ? ra[p][3] : 0.0f};
                split4(v, p1, p2, p3);
            }
            else split4(ra[p], p1, p2, p3);
            unsigned short* d = sA + x3_lds(p * RPP + s_row, s_col);
            *reinterpret_cast<u32x2_t*>(d) = p1;
            *reinterpret_cast<u32x2_t*>(d + LDS_A) = p2;
            *reinterpret_cast<u32x2_t*>(d + 2 * LDS_A) = p3;
        }
#pragma unroll
        for (int t = 0; t < WV; t++)
            if (WTOT % 256 == 0 || t * 256 + tid < WTOT) *reinterpret_cast<u32x4_t*>(sB + sb_off[t]) = rb[t];
    };
    // The residual of a block tail (RES, not UNIT), in the epilogue's own layout: vector t of 32-row block i of the wave tile is
    // row t * 64 / VEC_PER_ROW + lane / VEC_PER_ROW, 4 floats.  A descriptor over the tile's rows that exist; a row past M gets
    // an offset beyond every buffer (a select, no branch): the load answers with zeros and requests nothing.
    constexpr int VEC_PER_ROW = WN / 4;
    constexpr int VPL = 32 * VEC_PER_ROW / 64; // vectors per lane and block (8 | 4)
    // ... of block 0 that travel in K-step k_last - BK; the rest in K-step k_last, where both staging sets and the weight's registers
    // are dead.  One: with two (four) the 128-wide six-term tail spills 3 (7) registers, and a scratch reload counts in vmcnt
    // like the loads it would have to overtake (profiles/tail_prefetch/resource_usage.md)
    constexpr int VRA = 1;
    constexpr bool TAIL_RES = RES && !UNIT;
    f32x4_t rres[2][TAIL_RES ? VPL : 1];
    auto fetch_res = [&](int i, int t_begin, int t_end) {
        if constexpr (TAIL_RES) {
            const __amdgpu_buffer_rsrc_t r_rsrc = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<float*>(res + (size_t)m0 * N + n0), 0, (int)(((size_t)(rows_here - 1) * N + BN) * 4), 0x00020000);
            // (ONE offset register per lane, the block and the vector as the load's scalar offset: eight offsets would stay live through the K loop)
            const int lrow = wm * 64 + lane / VEC_PER_ROW;
            const unsigned off = ((unsigned)lrow * (unsigned)N + (unsigned)(wn * WN + (lane % VEC_PER_ROW) * 4)) * 4u;
#pragma unroll
            for (int t = t_begin; t < t_end; t++) {
                const int urow = i * 32 + t * (64 / VEC_PER_ROW);      // uniform part of the row
                rres[i][t] = __builtin_bit_cast(f32x4_t, __builtin_amdgcn_raw_buffer_load_b128(
                    r_rsrc, lrow < rows_here - urow ? off : 0xFFFFFFF0u, urow * N * 4, 0));
            }
        }
    };
    // fragment BYTE offsets of the wave's first A and B rows for the two halves of a K-step (32 rows further: 32 pitches further, the
    // swizzle has a period of 16 rows).  In a block tail the peeled steps are copies of the step's code: the offsets are made
    // opaque there, or every copy puts them together again from pieces that then stay live, and spill, across the K loop.
    int frag_a[kX3BK / 16], frag_b[kX3BK / 16];
    if constexpr (TAIL_RES) {
#pragma unroll
        for (int h = 0; h < kX3BK / 16; h++) {
            frag_a[h] = 2 * x3_lds(wm * 64 + (lane & 31), h * 16 + (lane >> 5) * 8);
            frag_b[h] = 2 * x3_lds(wn * WN + (lane & 31), h * 16 + (lane >> 5) * 8);
            asm volatile("" : "+v"(frag_a[h]), "+v"(frag_b[h]));
        }
    }
    // one K-step: LDS holds tile k0, `cur` the activation of tile k0 + BK (requested a step ago), `nxt` is free.  The weight's
    // loads are issued BEFORE the activation's: vmcnt counts in order, so the wait for the weight of tile k0 + BK (behind this
    // step's MFMAs) leaves the activation of tile k0 + 2 BK in flight.
    // `tail` 0: any step.  1 | 2 (block tails only): the steps k_last - BK and k_last, peeled at compile time -- what `tail` 0 would
    // request there AGAIN (the activation of tile k_last; then that and the weight of tile k_last) nothing ever reads: the residual
    // of epilogue block 0 travels in those slots, behind the step's real weight fetch, so that the wait for the weight leaves it in flight.
    auto step = [&](auto tail, int k0, f32x4_t (&cur)[NPA], f32x4_t (&nxt)[NPA]) {
        constexpr int TAIL = decltype(tail)::value;
        // (no branch around a load: past the end the last tile is requested again -- behind a conditional load the compiler's
        // wait counts assume the worst path, i.e. they wait for everything in flight, which is what two steps ahead is there to avoid)
        const bool more = TAIL == 1 || (TAIL == 0 && k0 + kX3BK < K);
        const int k_last = K - kX3BK;
        if constexpr (TAIL == 0) {
            fetch_b(k0 + kX3BK < k_last ? k0 + kX3BK : k_last);
            fetch_a(nxt, k0 + 2 * kX3BK < k_last ? k0 + 2 * kX3BK : k_last);
        } else if constexpr (TAIL == 1) {
            fetch_b(k_last);
            fetch_res(0, 0, VRA);
        } else {
            fetch_res(0, VRA, VPL);
        }
        __builtin_amdgcn_sched_barrier(0);     // (the scheduler otherwise sinks the loads behind the MFMAs and lets fragments share their registers)
#pragma unroll
        for (int kk = 0; kk < kX3BK; kk += 16) {
            bf16x8_t fa[3][2], fb[3][NT];
            const int kh = OPA_X3_DIAG == 4 ? 0 : kk / 16;
            const int kof = kh * 16 + (lane >> 5) * 8;
#pragma unroll
            for (int pl = 0; pl < 3; pl++) {
#pragma unroll
                for (int i = 0; i < 2; i++)
                    fa[pl][i] = *reinterpret_cast<const bf16x8_t*>(TAIL_RES ? reinterpret_cast<const unsigned short*>(smem + frag_a[kh]) + (pl * LDS_A + i * 32 * kX3Pitch)
                                                                       : sA + pl * LDS_A + x3_lds(wm * 64 + i * 32 + (lane & 31), kof));
#pragma unroll
                for (int j = 0; j < NT; j++)
                    fb[pl][j] = *reinterpret_cast<const bf16x8_t*>(TAIL_RES ? reinterpret_cast<const unsigned short*>(smem + frag_b[kh]) + (3 * LDS_A + pl * LDS_B + j * 32 * kX3Pitch)
                                                                       : sB + pl * LDS_B + x3_lds(wn * WN + j * 32 + (lane & 31), kof));
            }
            // consecutive MFMAs go to different accumulators (a dependent MFMA waits for its predecessor's passes)
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < NT; j++)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0][i], fb[0][j], acc[i][j], 0, 0, 0);
            // the corrections, smallest first
#pragma unroll
            for (int s = 4; s >= 1; s--) {
                if ((TERMS == 6 && s > 2) || OPA_X3_DIAG == 3) continue;
#pragma unroll
                for (int pa_ = 0; pa_ < 3; pa_++) {
                    const int pb_ = s - pa_;
                    if (pb_ < 0 || pb_ > 2) continue;
#pragma unroll
                    for (int i = 0; i < 2; i++)
#pragma unroll
                        for (int j = 0; j < NT; j++)
                            low[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[pa_][i], fb[pb_][j], low[i][j], 0, 0, 0);
                }
            }
        }
        __syncthreads();                       // every wave is done reading the stage
        if (more && (OPA_X3_DIAG != 2 || cur[0][0] == 12345.678f)) store(cur, k0 + kX3BK);
        __syncthreads();
    };
    fetch_b(0);
    fetch_a(ra0, 0);
    if constexpr (TAIL_RES) {
        if (tid < BN) reinterpret_cast<float*>(smem + SMEM_BYTES)[tid] = bias[n0 + tid];
    }
    store(ra0, 0);
    __syncthreads();
    fetch_a(ra1, kX3BK);                       // (K is a multiple of 2 BK: the launcher checks)
    constexpr std::integral_constant<int, 0> any_step{};
    if constexpr (TAIL_RES) {
        int k0 = 0;
        for (; k0 < K - 2 * kX3BK; k0 += 2 * kX3BK) {
            step(any_step, k0, ra1, ra0);
            step(any_step, k0 + kX3BK, ra0, ra1);
        }
        step(std::integral_constant<int, 1>{}, k0, ra1, ra0);
        step(std::integral_constant<int, 2>{}, k0 + kX3BK, ra0, ra1);
    } else {
        for (int k0 = 0; k0 < K; k0 += 2 * kX3BK) {
            step(any_step, k0, ra1, ra0);
            step(any_step, k0 + kX3BK, ra0, ra1);
        }
    }
    // (the loop's last barrier: staging LDS is free, reuse it for the epilogue)
    if constexpr (UNIT) {
        x3_unit_epilogue<BN, RES, RELU, UX>(reinterpret_cast<float*>(smem), acc, low, bias, res, out, M, m0, n0, lane, wave, sec.ldp, sec.n_real,
                                            sec.act, sec.act_param);
        return;
    }

    // epilogue, one 32-row block of the wave tile at a time through a wave-private f32 patch: the residual load and
    // the output store are row-contiguous 16-B vectors.  The residual of block 0 has been on its way since the last two K-steps;
    // block 1's is requested here, where fragments and staging registers are dead, and travels while block 0 is written out.
    float* patch = reinterpret_cast<float*>(smem) + wave * (32 * WN);
    if constexpr (TAIL_RES) {
        fetch_res(1, 0, VPL);
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int i = 0; i < 2; i++) {
#pragma unroll
        for (int j = 0; j < NT; j++) {
            const int col = j * 32 + (lane & 31);
            const float b = TAIL_RES ? reinterpret_cast<const float*>(smem + SMEM_BYTES)[wn * WN + col] : bias[n0 + wn * WN + col];
#pragma unroll
            for (int r = 0; r < 16; r++) {     // C layout: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
                const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                patch[row * WN + col] = (OPA_X3_ONE_ACC ? acc[i][j][r] : acc[i][j][r] + low[i][j][r]) + b;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int t = 0; t < VPL; t++) {
            const int v = t * 64 + lane;
            const int row = v / VEC_PER_ROW, c4 = (v % VEC_PER_ROW) * 4;
            const int m = m0 + wm * 64 + i * 32 + row;
            if (m < M) {
                f32x4_t f = *reinterpret_cast<const f32x4_t*>(patch + row * WN + c4);
                if constexpr (TAIL_RES) f += rres[i][t];
                if (RELU) {
#pragma unroll
                    for (int e = 0; e < 4; e++) f[e] = fmaxf(f[e], 0.0f);
                }
                *reinterpret_cast<f32x4_t*>(out + (size_t)m * N + n0 + wn * WN + c4) = f;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        asm volatile("" ::: "memory");
    }
}

// ---- The 128 x 256 tile: the two 256-thread workgroups a compute unit hosts above, as ONE of 512 threads that stages, and splits,
// its 128-row activation tile ONCE for 256 output columns instead of once per 128.  Eight waves as 2(M) x 4(N); the wave tile is
// the 64 x 64 of the 128-wide tile with the same accumulator sets, fragment maps and MFMA order (the leading product, then the
// corrections smallest first), the same split, prologue and epilogue arithmetic: every output element sees the same additions in
// the same order, the results are bit for bit those of the 128-wide tile (tests/test_gpu_gemm_x3_wide.py).  Six terms, not UNIT.
// Per wave and K-step the activation loads (4 -> 2 x 16 B), the split (88 -> 44 VALU) and the plane stores (12 -> 6 ds_write_b64)
// halve; MFMAs, fragment reads and weight staging stay what they were.
// LDS (dynamic, 145 KB of the compute unit's 160): TWO stages of three planes x (128 + 256) rows x 64 B, the same XOR swizzle; the
// epilogue's eight 8 KB patches alias stage 0; the tile's 256 bias values sit behind the stages.
// Loop: ONE barrier per K-step.  Step k requests the weight of tile k + 1 and the activation of tile k + 2 (buffer loads, weight
// first, unconditional), multiplies from stage k & 1, and splits and stores tile k + 1 into the other stage -- which every wave
// finished reading before the barrier that ended step k - 1.  With one workgroup per compute unit nothing but the kernel itself
// can put the split under MFMAs: every wave issues one VALU instruction of its split behind each of its MFMAs (see `step`).
// The last two K-steps are peeled in EVERY instantiation: no tile is requested twice, a block tail's residual vectors of epilogue
// block 0 travel in those slots as above.
// What one workgroup per compute unit costs: nothing runs under a workgroup's epilogue, and the last round of a launch occupies
// whole compute units where a 256-thread workgroup leaves half of one to its neighbour.  launch_x3 keeps the 128-wide tile where
// that outweighs the halved staging (a round of workgroups that has only begun; a residual behind a short K loop):
// x3_wide_pays, profiles/x3_wide/README.md.
// The operand prologue is applied where the tile is split, not where it is requested (its a_bias vector travels with the tile):
// the same float32 add and fmaxf on the same values.
#if OPA_X3_BK == 32 && OPA_X3_SWIZZLE && !OPA_X3_ONE_ACC && OPA_X3_DIAG == 0
#define OPA_X3_HAS_WIDE 1
constexpr int kX3WideBN = 256, kX3WideThreads = 512;
constexpr int kX3WideStageBytes = 3 * (kX3BM + kX3WideBN) * kX3Pitch * 2;          // 73 728
constexpr int kX3WideLdsBytes = 2 * kX3WideStageBytes + kX3WideBN * 4;             // 148 480
// Where launch_x3 takes this tile (measured: tools/gpu/gemm_x3_tile_ab.py, profiles/x3_wide/README.md).  ONE workgroup per compute
// unit: W workgroups take ceil(W / 256) whole rounds on the 256 compute units of an MI355X, at about 15/16 of the time the 128-wide
// tile needs for the same rows -- whose 2 W workgroups, two to a compute unit, end in a partial round that costs about a quarter
// of one.  And nothing runs under a workgroup's epilogue: behind a residual it is long -- alone, the tile gains from K = 384 on, but
// inside a resnet50 step the K = 512 tails of layer 4 did not: a residual only from K = 768 on.
constexpr unsigned kX3WideCUs = 256;
constexpr int kX3WideMinKRes = 768;
constexpr bool x3_wide_pays(unsigned long long wide_blocks, bool res, int K) {
    if (res && K < kX3WideMinKRes) return false;
    const unsigned long long rounds = (wide_blocks + kX3WideCUs - 1) / kX3WideCUs;
    return wide_blocks >= 2 * kX3WideCUs && rounds * kX3WideCUs * 15 <= (wide_blocks + kX3WideCUs / 4) * 16;
}

template <bool RES, bool RELU, bool PRO, int SRC>
__global__ __launch_bounds__(kX3WideThreads, 2) void gemm_f32x3_wide_kernel(
        const float* __restrict__ A, const unsigned short* __restrict__ W3, const float* __restrict__ bias,
        const float* __restrict__ res, float* __restrict__ out, int M, int N, int K, const float* __restrict__ a_bias,
        const X3Second sec) {
    constexpr int BN = kX3WideBN, WN = 64, NT = 2;
    constexpr int LDS_A = kX3BM * kX3Pitch, LDS_B = BN * kX3Pitch;        // bf16 elements of ONE plane
    static_assert(kX3WideThreads / 64 * 32 * WN * 4 <= kX3WideStageBytes, "the epilogue patches alias stage 0 alone");
    extern __shared__ __attribute__((aligned(16))) unsigned char x3w_smem[];
    float* s_bias = reinterpret_cast<float*>(x3w_smem + 2 * kX3WideStageBytes);

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int n_tiles = N / BN;
    const unsigned nwg = gridDim.x, xcd = blockIdx.x & 7u, in_xcd = blockIdx.x >> 3;
    const unsigned q = nwg >> 3, r8 = nwg & 7u;
    const unsigned logical = (xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q) + in_xcd;
    const int m0 = (int)(logical / n_tiles) * kX3BM;
    const int n0 = (int)(logical % n_tiles) * BN;

    f32x16_t acc[2][NT], low[2][NT];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < NT; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) { acc[i][j][r] = 0.0f; low[i][j][r] = 0.0f; }

    // staging maps.  A: a 32-float row is 8 x 16 B, 512 threads cover 64 rows per pass, two passes.  W3: a 32-bf16 row of one plane
    // is 4 x 16 B, 512 threads cover 128 rows of a plane: vector t of a thread is plane t / 2, row (t % 2) * 128 + tid / 4 -- ONE
    // offset per thread, plane and half as the load's scalar offset and the store's immediate (the swizzle has a period of 16 rows)
    constexpr int VA = kX3BK / 4, RPP = kX3WideThreads / VA, NPA = kX3BM / RPP, WV = 6;
    static_assert(NPA == 2 && 3 * BN * (kX3BK / 8) == WV * kX3WideThreads, "staging maps");
    const int s_row = tid / VA, s_col = (tid % VA) * 4;
    f32x4_t ra0[NPA], ra1[NPA], ab0, ab1;      // the activation travels TWO K-steps ahead, the weight one
    u32x4_t rb[WV];
    constexpr bool TWO = SRC == 1, TAPS = SRC == 2;
    const int rows_here = M - m0 < kX3BM ? M - m0 : kX3BM;
    const int KA = TWO ? sec.K1 : TAPS ? sec.C : K;
    const int shift = TAPS && !sec.padded ? sec.dil * (sec.wi + 1) * sec.pix : 0;
    const float* a1_base = TAPS ? A - (size_t)shift : A + (size_t)m0 * KA;
    const int a1_bytes = TAPS ? (int)(((size_t)sec.batch * sec.hi_wi * sec.pix + shift) * 4) : (int)((size_t)rows_here * KA * 4);
    const __amdgpu_buffer_rsrc_t a_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a1_base), 0, a1_bytes, 0x00020000);
    const int K2 = K - KA;
    auto in_row = [&](int m) -> long long {
        const int b = m / sec.ho_wo, r = m - b * sec.ho_wo, oy = r / sec.wo, ox = r - oy * sec.wo;
        return (long long)b * sec.hi_wi + (long long)oy * sec.stride * sec.wi + (long long)ox * sec.stride;
    };
    long long row0_2 = 0;
    const float* a2_base = nullptr;
    int a2_bytes = 0;
    unsigned pa2[NPA];
    if constexpr (TWO) {
        row0_2 = in_row(__builtin_amdgcn_readfirstlane(m0));
        const int m_end = m0 + rows_here - 1;
        a2_base = sec.A2 + (size_t)row0_2 * K2;
        a2_bytes = (int)((size_t)(in_row(__builtin_amdgcn_readfirstlane(m_end)) - row0_2 + 1) * K2 * 4);
    }
    const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<unsigned short*>(W3 + (size_t)n0 * K), 0, (int)(((size_t)3 * N - n0) * K * 2), 0x00020000);
    unsigned pa[NPA], vmask[NPA];
#pragma unroll
    for (int p = 0; p < NPA; p++) {            // rows past M read row M - 1 (valid memory; the epilogue never stores them)
        int m = m0 + p * RPP + s_row;
        if (m > M - 1) m = M - 1;
        pa[p] = ((unsigned)(m - m0) * (unsigned)KA + (unsigned)s_col) * 4u;
        vmask[p] = 0u;
        if constexpr (TAPS) {
            const int b = m / sec.ho_wo, r = m - b * sec.ho_wo, oy = r / sec.wo, ox = r - oy * sec.wo;
            pa[p] = (unsigned)((long long)b * sec.hi_wi + (long long)oy * sec.stride * sec.wi + (long long)ox * sec.stride) * (unsigned)sec.pix * 4u
                    + (unsigned)s_col * 4u;
            if (sec.padded) vmask[p] = 0xffffffffu;
            else
                for (int t = 0; t < sec.ntaps; t++) {
                    const int iy = oy * sec.stride - sec.dil + sec.dil * (t / sec.taps_x), ix = ox * sec.stride - sec.dil + sec.dil * (t % sec.taps_x);
                    if (iy >= 0 && iy < sec.hi && ix >= 0 && ix < sec.wi) vmask[p] |= 1u << t;
                }
        }
        if constexpr (TWO) pa2[p] = ((unsigned)(in_row(m) - row0_2) * (unsigned)K2 + (unsigned)s_col) * 4u;
    }
    const unsigned pb = ((unsigned)(tid >> 2) * (unsigned)K + (unsigned)(tid & 3) * 8u) * 2u;
    const int sb_off = x3_lds(tid >> 2, (tid & 3) * 8);
    const int sa_off = x3_lds(s_row, s_col);
    auto fetch_a = [&](f32x4_t (&ra)[NPA], f32x4_t& ab, int k0) {        // global -> registers for K-step k0
        if constexpr (TAPS) {
            const int t = k0 / KA, kc = k0 - t * KA;
            const int soff = (int)((((unsigned)(sec.dil * (t / sec.taps_x)) * (unsigned)sec.wi + (unsigned)(sec.dil * (t % sec.taps_x))) * (unsigned)sec.pix + (unsigned)kc) * 4u);
#pragma unroll
            for (int p = 0; p < NPA; p++)
                ra[p] = __builtin_bit_cast(f32x4_t, __builtin_amdgcn_raw_buffer_load_b128(a_rsrc, (vmask[p] >> t) & 1u ? pa[p] : 0xFFFFFFF0u, soff, 0));
        } else if constexpr (TWO) {
            const bool second = k0 >= KA;
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<float*>(second ? a2_base : a1_base), 0, second ? a2_bytes : a1_bytes, 0x00020000);
            const int ks = (second ? k0 - KA : k0) * 4;
#pragma unroll
            for (int p = 0; p < NPA; p++)
                ra[p] = __builtin_bit_cast(f32x4_t, __builtin_amdgcn_raw_buffer_load_b128(rs, second ? pa2[p] : pa[p], ks, 0));
        } else {
#pragma unroll
            for (int p = 0; p < NPA; p++) ra[p] = __builtin_bit_cast(f32x4_t, __builtin_amdgcn_raw_buffer_load_b128(a_rsrc, pa[p], k0 * 4, 0));
        }
        if (PRO) ab = *reinterpret_cast<const f32x4_t*>(a_bias + k0 + s_col);
    };
    auto fetch_b = [&](int k0) {
#pragma unroll
        for (int t = 0; t < WV; t++)
            rb[t] = __builtin_bit_cast(u32x4_t, __builtin_amdgcn_raw_buffer_load_b128(
                w_rsrc, pb, (int)((((unsigned)(t >> 1) * (unsigned)N + (unsigned)(t & 1) * 128u) * (unsigned)K + (unsigned)k0) * 2u), 0));
    };
    auto store_a = [&](const f32x4_t (&ra)[NPA], const f32x4_t& ab, int stage) {    // prologue, split, three plane stores
        unsigned short* sA = reinterpret_cast<unsigned short*>(x3w_smem + stage * kX3WideStageBytes);
#pragma unroll
        for (int p = 0; p < NPA; p++) {
            f32x4_t v = ra[p];
            if (PRO) {
#pragma unroll
                for (int e = 0; e < 4; e++) v[e] = fmaxf(v[e] + ab[e], 0.0f);
            }
            u32x2_t p1, p2, p3;
            split4(v, p1, p2, p3);
            unsigned short* d = sA + sa_off + p * RPP * kX3Pitch;
            *reinterpret_cast<u32x2_t*>(d) = p1;
            *reinterpret_cast<u32x2_t*>(d + LDS_A) = p2;
            *reinterpret_cast<u32x2_t*>(d + 2 * LDS_A) = p3;
        }
    };
    auto store_b = [&](int stage) {
        unsigned short* sB = reinterpret_cast<unsigned short*>(x3w_smem + stage * kX3WideStageBytes) + 3 * LDS_A;
#pragma unroll
        for (int t = 0; t < WV; t++)
            *reinterpret_cast<u32x4_t*>(sB + (t >> 1) * LDS_B + (t & 1) * 128 * kX3Pitch + sb_off) = rb[t];
    };
    // the residual of a block tail in the epilogue's own layout, as in the 128-wide tile (the wave tile is the same 64 x 64)
    constexpr int VEC_PER_ROW = WN / 4, VPL = 32 * VEC_PER_ROW / 64, VRA = 1;
    f32x4_t rres[2][RES ? VPL : 1];
    auto fetch_res = [&](int i, int t_begin, int t_end) {
        if constexpr (RES) {
            const __amdgpu_buffer_rsrc_t r_rsrc = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<float*>(res + (size_t)m0 * N + n0), 0, (int)(((size_t)(rows_here - 1) * N + BN) * 4), 0x00020000);
            const int lrow = wm * 64 + lane / VEC_PER_ROW;
            const unsigned off = ((unsigned)lrow * (unsigned)N + (unsigned)(wn * WN + (lane % VEC_PER_ROW) * 4)) * 4u;
#pragma unroll
            for (int t = t_begin; t < t_end; t++) {
                const int urow = i * 32 + t * (64 / VEC_PER_ROW);
                rres[i][t] = __builtin_bit_cast(f32x4_t, __builtin_amdgcn_raw_buffer_load_b128(
                    r_rsrc, lrow < rows_here - urow ? off : 0xFFFFFFF0u, urow * N * 4, 0));
            }
        }
    };
    // fragment BYTE offsets of the wave's first A and B rows for the two halves of a K-step, opaque (the steps are copies of one
    // another: put together from pieces they would stay live, and spill, across the K loop)
    int frag_a[2], frag_b[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
        frag_a[h] = 2 * x3_lds(wm * 64 + (lane & 31), h * 16 + (lane >> 5) * 8);
        frag_b[h] = 2 * (3 * LDS_A + x3_lds(wn * WN + (lane & 31), h * 16 + (lane >> 5) * 8));
        asm volatile("" : "+v"(frag_a[h]), "+v"(frag_b[h]));
    }
    auto multiply = [&](int stage) {
        const unsigned char* base = x3w_smem + stage * kX3WideStageBytes;
#pragma unroll
        for (int kh = 0; kh < 2; kh++) {
            bf16x8_t fa[3][2], fb[3][NT];
#pragma unroll
            for (int pl = 0; pl < 3; pl++) {
#pragma unroll
                for (int i = 0; i < 2; i++)
                    fa[pl][i] = *reinterpret_cast<const bf16x8_t*>(reinterpret_cast<const unsigned short*>(base + frag_a[kh]) + (pl * LDS_A + i * 32 * kX3Pitch));
#pragma unroll
                for (int j = 0; j < NT; j++)
                    fb[pl][j] = *reinterpret_cast<const bf16x8_t*>(reinterpret_cast<const unsigned short*>(base + frag_b[kh]) + (pl * LDS_B + j * 32 * kX3Pitch));
            }
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < NT; j++)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0][i], fb[0][j], acc[i][j], 0, 0, 0);
            // the corrections, smallest first
#pragma unroll
            for (int s = 2; s >= 1; s--) {
#pragma unroll
                for (int pa_ = 0; pa_ < 3; pa_++) {
                    const int pb_ = s - pa_;
                    if (pb_ < 0 || pb_ > 2) continue;
#pragma unroll
                    for (int i = 0; i < 2; i++)
#pragma unroll
                        for (int j = 0; j < NT; j++)
                            low[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[pa_][i], fb[pb_][j], low[i][j], 0, 0, 0);
                }
            }
        }
    };
    // one K-step: stage `stage` holds tile k0, `cur` the activation of tile k0 + BK (requested a step ago), `nxt` is free.
    // `tail` 0: any step but the last two.  1: step k_last - BK requests the last weight tile and no activation; 2: step k_last
    // requests and stores nothing.  A block tail's residual of epilogue block 0 travels in the slots that are free there.
    auto step = [&](auto tail, auto stage_c, int k0, f32x4_t (&cur)[NPA], f32x4_t& cur_ab, f32x4_t (&nxt)[NPA], f32x4_t& nxt_ab) {
        constexpr int TAIL = decltype(tail)::value, STAGE = decltype(stage_c)::value;
        if constexpr (TAIL == 0) {
            fetch_b(k0 + kX3BK);
            fetch_a(nxt, nxt_ab, k0 + 2 * kX3BK);
        } else if constexpr (TAIL == 1) {
            fetch_b(k0 + kX3BK);
            fetch_res(0, 0, VRA);
        } else {
            fetch_res(0, VRA, VPL);
        }
        __builtin_amdgcn_sched_barrier(0);
        multiply(STAGE);
        if constexpr (TAIL != 2) {
            // The split rides in the MFMAs' shadow INSIDE each wave: one of its VALU instructions behind each of the first 44 MFMAs
            // (an MFMA occupies its pipe for 8 passes; the wave issues other work meanwhile).  Measured against the two shifts of
            // winograd_f23_w8_kernel -- the second wave of a SIMD splitting first, multiplying second -- this order was faster on
            // ten of thirteen shapes, and so was no shift at all (profiles/x3_wide/README.md): all eight waves meet at one
            // barrier per K-step, which leaves two shifts little room to drift apart.
            store_a(cur, cur_ab, STAGE ^ 1);
#pragma unroll
            for (int g = 0; g < 44; g++) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);         // one MFMA,
                __builtin_amdgcn_sched_group_barrier(0x002, 1, 0);         // one VALU instruction
            }
            store_b(STAGE ^ 1);
        }
        __syncthreads();                       // the other stage is written, this one read by every wave
    };
    const float bias_v = bias[n0 + (tid & (BN - 1))];      // (requested first: its wait leaves the tiles in flight)
    fetch_b(0);
    fetch_a(ra0, ab0, 0);
    fetch_a(ra1, ab1, kX3BK);                  // (K is a multiple of 2 BK: the launcher checks)
    if (tid < BN) s_bias[tid] = bias_v;
    store_a(ra0, ab0, 0);
    store_b(0);
    __syncthreads();
    constexpr std::integral_constant<int, 0> c0{};
    constexpr std::integral_constant<int, 1> c1{};
    constexpr std::integral_constant<int, 2> c2{};
    int k0 = 0;
    for (; k0 < K - 2 * kX3BK; k0 += 2 * kX3BK) {
        step(c0, c0, k0, ra1, ab1, ra0, ab0);
        step(c0, c1, k0 + kX3BK, ra0, ab0, ra1, ab1);
    }
    step(c1, c0, k0, ra1, ab1, ra0, ab0);
    step(c2, c1, k0 + kX3BK, ra0, ab0, ra1, ab1);

    // epilogue: as the 128-wide tile's, one 32-row block of the wave tile at a time through a wave-private f32 patch
    float* patch = reinterpret_cast<float*>(x3w_smem) + wave * (32 * WN);
    if constexpr (RES) {
        fetch_res(1, 0, VPL);
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int i = 0; i < 2; i++) {
#pragma unroll
        for (int j = 0; j < NT; j++) {
            const int col = j * 32 + (lane & 31);
            const float b = s_bias[wn * WN + col];
#pragma unroll
            for (int r = 0; r < 16; r++) {     // C layout: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
                const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                patch[row * WN + col] = acc[i][j][r] + low[i][j][r] + b;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int t = 0; t < VPL; t++) {
            const int v = t * 64 + lane;
            const int row = v / VEC_PER_ROW, c4 = (v % VEC_PER_ROW) * 4;
            const int m = m0 + wm * 64 + i * 32 + row;
            if (m < M) {
                f32x4_t f = *reinterpret_cast<const f32x4_t*>(patch + row * WN + c4);
                if constexpr (RES) f += rres[i][t];
                if (RELU) {
#pragma unroll
                    for (int e = 0; e < 4; e++) f[e] = fmaxf(f[e], 0.0f);
                }
                *reinterpret_cast<f32x4_t*>(out + (size_t)m * N + n0 + wn * WN + c4) = f;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        asm volatile("" ::: "memory");
    }
}
#else
#define OPA_X3_HAS_WIDE 0
#endif

enum X3Mode { kX3Plain = 0, kX3Pair = 1, kX3Taps = 2, kX3Unit = 3 };      // SRC 0, 1, 2; UNIT (whose SRC is 0)

// The instantiations that exist, 89: launch_x3 launches these and refuses everything else.
// Not UNIT, 56: BN x TERMS x RELU, x PRO except with taps (no operand prologue there), x RES with one activation alone (the pair's
// second activation IS the identity branch).  UNIT, 11 for each (BN, TERMS) but (128, 9), which does not fit the register file: one
// activation, no prologue, RES = a third operand; five epilogues, RELU only where UX names no activation, a residual only as RES.
constexpr bool x3_exists(int BN, bool RES, bool RELU, bool PRO, int TERMS, int SRC, bool UNIT, int UX) {
    if (!UNIT) return UX == 0 && !(SRC != 0 && RES) && !(SRC == 2 && PRO);
    if (SRC != 0 || PRO || (BN == 128 && TERMS == 9)) return false;
    const bool known = UX == 0 || UX == kUxHardswish || UX == kUxResidual || UX == (kUxResidual | kUxHardswish) || UX == kUxActParam;
    return known && !(RELU && (UX & ~kUxResidual) != 0) && !((UX & kUxResidual) != 0 && !RES);
}

// Every launch of this file.  N and K are the kernel's (UNIT: the padded sizes), `third` the residual, or UNIT's partner or residual.
static hipError_t launch_x3(X3Mode mode, const float* A, const unsigned short* W3, const float* bias, const float* third, float* out,
                            int M, int N, int K, bool relu, int ux, int terms, const float* a_bias, hipStream_t st, const X3Second& sec) {
    // (the 128-wide tile with nine terms does not fit the register file -- its instantiations spill 8 registers -- so the unit mode has none)
    const int bn = mode != kX3Unit ? (N % 128 == 0 ? 128 : 64)
                                   : (N % 128 == 0 && terms == 6 ? 128 : 64);
    const unsigned blocks = (unsigned)((long long)((M + kX3BM - 1) / kX3BM) * (N / bn));
#if OPA_X3_HAS_WIDE
    // The 128 x 256 tile: not UNIT, six terms, N a multiple of 256, and a launch for which x3_wide_pays.  OPA_X3_TILE = 128 | 256
    // overrides the latter -- never the first three conditions -- and is read on every launch: A/B runs and the tests switch
    // tiles inside one process.
    if (mode != kX3Unit && terms == 6 && N % kX3WideBN == 0) {
        const char* env = std::getenv("OPA_X3_TILE");
        const int forced = env && *env ? std::atoi(env) : 0;
        const unsigned wide_blocks = blocks / 2;
        if (forced == kX3WideBN || (forced != 128 && x3_wide_pays(wide_blocks, third != nullptr, K)))
            return with_value<kX3Plain, kX3Pair, kX3Taps>(mode, [&](auto MODE) {
            return with_flag(third != nullptr, [&](auto RES) {
            return with_flag(relu, [&](auto RELU) {
            return with_flag(a_bias != nullptr, [&](auto PRO) {
                constexpr int SRC = (int)decltype(MODE)::value;
                if constexpr (x3_exists(kX3WideBN, RES, RELU, PRO, 6, SRC, false, 0)) {
                    auto* kernel = &gemm_f32x3_wide_kernel<RES, RELU, PRO, SRC>;
                    // (per device, not per process: set on every launch)
                    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kX3WideLdsBytes);
                    if (e != hipSuccess) return e;
                    kernel<<<wide_blocks, kX3WideThreads, kX3WideLdsBytes, st>>>(A, W3, bias, third, out, M, N, K, a_bias, sec);
                    return hipGetLastError();
                } else {
                    return hipErrorInvalidValue;
                }
            }); }); }); });
    }
#endif
    return with_value<64, 128>(bn, [&](auto BN) {
    return with_value<6, 9>(terms == 6 ? 6 : 9, [&](auto TERMS) {
    return with_value<kX3Plain, kX3Pair, kX3Taps, kX3Unit>(mode, [&](auto MODE) {
    return with_value<0, kUxHardswish, kUxResidual, kUxResidual | kUxHardswish, kUxActParam>(ux, [&](auto UX) {
    return with_flag(third != nullptr, [&](auto RES) {
    return with_flag(relu, [&](auto RELU) {
    return with_flag(a_bias != nullptr, [&](auto PRO) {
        constexpr bool UNIT = MODE == kX3Unit;
        constexpr int SRC = UNIT ? 0 : (int)MODE;
        if constexpr (x3_exists(BN, RES, RELU, PRO, TERMS, SRC, UNIT, UX)) {
            gemm_f32x3_bias_act_kernel<BN, RES, RELU, PRO, TERMS, SRC, UNIT, UX><<<blocks, 256, 0, st>>>(A, W3, bias, third, out, M, N, K, a_bias, sec);
            return hipGetLastError();
        } else {
            return hipErrorInvalidValue;
        }
    }); }); }); }); }); }); });
}

hipError_t launch_gemm_f32x3_bias_act(const float* A, const unsigned short* W3, const float* bias, const float* res, float* out,
                                      int M, int N, int K, int relu, int terms, hipStream_t st, const float* a_bias) {
    return launch_x3(kX3Plain, A, W3, bias, res, out, M, N, K, relu != 0, 0, terms, a_bias, st, X3Second{});
}

// out[B, ho, wo, N] = act([A1 | pixels of A2 at stride s] * W3cat^T + bias): A1 [B*ho*wo, K1], A2 [B, hi, wi, K2], W3cat [3][N][K1 + K2]
hipError_t launch_gemm2_f32x3_bias_act(const float* A1, int K1, const float* A2, int K2, int batch, int hi, int wi, int stride,
                                       const unsigned short* W3, const float* bias, float* out, int N, int relu, int terms,
                                       hipStream_t st, const float* a_bias) {
    const int ho = (hi - 1) / stride + 1, wo = (wi - 1) / stride + 1;
    X3Second sec;
    sec.A2 = A2; sec.K1 = K1;
    sec.ho_wo = ho * wo; sec.wo = wo; sec.hi_wi = hi * wi; sec.wi = wi; sec.stride = stride;
    return launch_x3(kX3Pair, A1, W3, bias, nullptr, out, batch * ho * wo, N, K1 + K2, relu != 0, 0, terms, a_bias, st, sec);
}

// The UNIT mode: A [M, K] with `lda` floats between rows, W3 [3][Np][Kp] and bias [Np] padded with zeros (Np, Kp: N, K rounded up
// to multiples of 64), partner or residual [M, N] with `ldp` / `ldr` floats between rows or null; out [M, N] dense, or [M, 2N] with
// a partner.  act 3 / 4 are read from `sec` at run time; with a residual they have no instantiation.
hipError_t launch_gemm_unit_act_f32x3(const float* A, int lda, const unsigned short* W3, const float* bias, const float* partner, int ldp,
                                      const float* residual, int ldr, float* out, int M, int N, int K, int act, int terms, hipStream_t st,
                                      float act_param) {
    if ((partner && residual) || act < 0 || act > 4) return hipErrorInvalidValue;
    X3Second sec;
    sec.lda = lda; sec.ldp = residual ? ldr : ldp; sec.n_real = N; sec.k_real = K;
    if (act >= 3) { sec.act = act; sec.act_param = act_param; }
    const int ux = (act == 2 ? kUxHardswish : 0) | (act >= 3 ? kUxActParam : 0) | (residual ? kUxResidual : 0);
    const int Np = (N + 63) / 64 * 64, Kp = (K + 63) / 64 * 64;
    return launch_x3(kX3Unit, A, W3, bias, residual ? residual : partner, out, M, Np, Kp, act == 1, ux, terms, nullptr, st, sec);
}

// 3x3 convolution, dilation d, padding d, stride s: out[B, ho, wo, N] = act(im2col(x) * W3^T + bias), x [B, hi, wi, C] channels-last,
// W3 = split_weight of the weight as [N, (ky, kx, c)] ([3][N][9 C]); C % 32 == 0, 9 C % 64 == 0, tensor + d (wi + 1) pixels < 2 GB
hipError_t launch_conv3x3_f32x3(const float* x, int batch, int hi, int wi, int C, int stride, int dilation, const unsigned short* W3,
                                const float* bias, float* out, int N, int relu, int terms, hipStream_t st) {
    const int ho = (hi - 1) / stride + 1, wo = (wi - 1) / stride + 1;
    X3Second sec;
    sec.ho_wo = ho * wo; sec.wo = wo; sec.hi_wi = hi * wi; sec.wi = wi; sec.stride = stride;
    sec.hi = hi; sec.C = C; sec.batch = batch;
    sec.pix = C; sec.taps_x = 3; sec.ntaps = 9; sec.dil = dilation;
    return launch_x3(kX3Taps, x, W3, bias, nullptr, out, batch * ho * wo, N, 9 * C, relu != 0, 0, terms, nullptr, st, sec);
}

// A convolution whose window ROWS are the taps: x [B, hp, wp, pix] is padded in memory (pix floats per pixel), output pixel
// (oy, ox) reads, for tap t, the `tap_floats` contiguous floats that begin at input pixel (stride oy + t, stride ox) -- the 7x7
// stride-2 stem of a ResNet on a 4-channel copy of the image: 8 taps of 8 pixels x 4 channels (the eighth row and column and the
// fourth channel meet zero weights).  W3 [3][N][ntaps * tap_floats].  out [B, ho, wo, N].
hipError_t launch_convrows_f32x3(const float* x, int batch, int hp, int wp, int pix, int ho, int wo, int stride, int ntaps, int tap_floats,
                                 const unsigned short* W3, const float* bias, float* out, int N, int relu, int terms, hipStream_t st) {
    X3Second sec;
    sec.ho_wo = ho * wo; sec.wo = wo; sec.hi_wi = hp * wp; sec.wi = wp; sec.stride = stride;
    sec.hi = hp; sec.C = tap_floats; sec.batch = batch;
    sec.pix = pix; sec.taps_x = 1; sec.ntaps = ntaps; sec.padded = 1;
    return launch_x3(kX3Taps, x, W3, bias, nullptr, out, batch * ho * wo, N, ntaps * tap_floats, relu != 0, 0, terms, nullptr, st, sec);
}

}  // namespace opa
