// 3x3 stride-1 convolution of the float32 network as Winograd F(2x2, 3x3), ONE kernel: input transform -> sixteen
// MFMA GEMMs -> output transform, nothing of the transformed domain ever leaves the compute unit.
//     y[n, h, w, :] = sum_{r,s} x[n, h + r - 1, w + s - 1, :] * g[:, :, r, s]^T        (NHWC float32, zero padding 1)
// The ResNet-50 trunk at 641 px / batch 32 spends 39 of its 75 ms in thirteen such convolutions (250 GFLOP each as a direct
// convolution, CK's implicit GEMM at 112 TFLOP/s = 0.71 of the dense float32 MFMA peak: there is no TF32 on gfx950, the
// float32 MFMA runs at the vector rate).  F(2x2, 3x3) needs 16 multiplications per 2x2 outputs instead of 36: 2.25x fewer
// MFMA flops, in float32 arithmetic throughout (the transforms are additions; G g G^T is computed once on the host in
// float64).  Separate transform kernels would write and re-read the 4x larger transformed tensors (15 GB per layer-1
// convolution) -- so one workgroup does all of it for 64 tiles x BN output channels.  Four kernels share that plan: the
// four-wave one described here (variants 0 / 1, the first version), the eight-wave one in two shifts that the Python side uses
// (variant 2, further down: what the four-wave kernel leaves idle and why) and its persistent form (variant 3: measured slower).
//   * 256 threads, four waves, wave w owns the four transform positions (xi = w, nu = 0..3) as 64 x BN accumulators each:
//     v_mfma_f32_32x32x2f32, 4 x 2 x NB accumulator blocks of 16 registers (NB = 2: 256 accumulator registers, one wave per
//     SIMD -- the float32 MFMA issues once per 64 cycles, one wave's other instructions fit into its shadow);
//   * per K-chunk of KC input channels: thread (tile, channel group) loads its tile's 4x4 pixels (KC/4 channels each) from
//     global memory one chunk AHEAD, transforms them in registers (B^T d B: 32 additions per channel) and stores the sixteen
//     positions into the other LDS buffer as V[position][k][tile] (pitch 66 / 68: conflict-free for the thread map of the
//     stores AND the MFMA operand reads); one barrier per chunk;
//   * the filter operand U[position][k][cout] is used by exactly one wave (the owner of the position), so it does not go
//     through LDS at all: the host lays it out so that a lane's values of a chunk are float4-contiguous, and every register
//     group is reloaded for the next chunk right after its last MFMA of this one;
//   * output transform: A^T m A splits into the nu-sum (inside the owning wave, registers) and the xi-sum across the four
//     waves through LDS (the staging buffers, reused), then bias / ReLU if asked and 256-B contiguous stores.
#include <atomic>
#include <cstdlib>

#include "common.hpp"
#include "split_bf16.hpp"

namespace opa {

typedef __attribute__((ext_vector_type(16))) float wf32x16_t;
typedef __attribute__((ext_vector_type(4))) float wf32x4_t;

template <int KC, int NB>
struct WinoCfg {
    static constexpr int VW = KC / 4;                  // channels per thread and pixel (float2 / float4 loads)
    static constexpr int P = VW == 4 ? 66 : 68;        // floats between two k rows of the LDS operand (64 tiles + pad)
    static constexpr int ROWS = 16 * KC;
    static constexpr int VBUF = ROWS * P;              // floats per stage
    static constexpr int BN = 32 * NB;                 // output channels per workgroup
    static constexpr int KQ = KC / 8;                  // float4 groups of k pairs per chunk
    static constexpr int STAGE_BYTES = 2 * VBUF * 4;
    static constexpr int EPI_BYTES = 4 * 2 * 64 * BN * 4;
    static constexpr int LDS_BYTES = STAGE_BYTES > EPI_BYTES ? STAGE_BYTES : EPI_BYTES;
};

template <int KC, int NB, int WGS>
__global__ __launch_bounds__(256, WGS) void winograd_f23_kernel(
        const float* __restrict__ x, const float* __restrict__ U, float* __restrict__ y, const float* __restrict__ bias,
        int H, int W, int Cin, int Cout, int TH, int TW, int T, int relu, int nb_major) {
    using C = WinoCfg<KC, NB>;
    constexpr int VW = C::VW, P = C::P, BN = C::BN, KQ = C::KQ;
    extern __shared__ __attribute__((aligned(16))) unsigned char wino_smem[];
    float* const lds = reinterpret_cast<float*>(wino_smem);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_nb = Cout / BN;
    // XCD-aware order (gemm_f32.hip): consecutive logical workgroups run on ONE XCD and share its L2
    const unsigned nwg = gridDim.x, xcd = blockIdx.x & 7u, in_xcd = blockIdx.x >> 3;
    const unsigned q8 = nwg >> 3, r8 = nwg & 7u;
    const unsigned logical = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + in_xcd;
    const unsigned n_tb = nwg / (unsigned)n_nb;
    const int tb = nb_major ? (int)(logical % n_tb) : (int)(logical / (unsigned)n_nb);
    const int nb = nb_major ? (int)(logical / n_tb) : (int)(logical % (unsigned)n_nb);
    const int nchunks = Cin / KC;

    // ---- the staging thread's tile: pixel offsets (clamped into the image) and validity, once
    const int tile_l = tid >> 2, cg = tid & 3;
    int t = tb * 64 + tile_l;
    if (t > T - 1) t = T - 1;
    const int tx = t % TW, ty = (t / TW) % TH, n = t / (TW * TH);
    unsigned rowoff[4], coloff[4];
    bool rv[4], cv[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int r = 2 * ty - 1 + i, c = 2 * tx - 1 + i;
        rv[i] = r >= 0 && r < H;
        cv[i] = c >= 0 && c < W;
        const int rc = r < 0 ? 0 : (r > H - 1 ? H - 1 : r), cc = c < 0 ? 0 : (c > W - 1 ? W - 1 : c);
        rowoff[i] = (unsigned)((n * H + rc) * W) * (unsigned)Cin;
        coloff[i] = (unsigned)cc * (unsigned)Cin + (unsigned)(cg * VW);
    }
    float d[16][VW];
    auto fetch_x = [&](int chunk) {
        const unsigned c0 = (unsigned)(chunk * KC);
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const float* p = x + (size_t)(rowoff[i] + coloff[j] + c0);
                if (VW == 4) {
                    const wf32x4_t v = *reinterpret_cast<const wf32x4_t*>(p);
#pragma unroll
                    for (int e = 0; e < VW; e++) d[i * 4 + j][e] = v[e];
                } else {
                    const float2 v = *reinterpret_cast<const float2*>(p);
                    d[i * 4 + j][0] = v.x; d[i * 4 + j][VW - 1] = v.y;
                }
            }
    };
    // B^T d B in registers, then the sixteen positions of this thread's VW channels to stage `buf`
    auto transform_store = [&](int buf) {
        float* const vb = lds + buf * C::VBUF + (cg * VW) * P + tile_l;
#pragma unroll
        for (int e = 0; e < VW; e++) {
            float z[16];
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) z[i * 4 + j] = (rv[i] && cv[j]) ? d[i * 4 + j][e] : 0.0f;
            float s[16];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                s[0 * 4 + j] = z[0 * 4 + j] - z[2 * 4 + j];
                s[1 * 4 + j] = z[1 * 4 + j] + z[2 * 4 + j];
                s[2 * 4 + j] = z[2 * 4 + j] - z[1 * 4 + j];
                s[3 * 4 + j] = z[1 * 4 + j] - z[3 * 4 + j];
            }
#pragma unroll
            for (int i = 0; i < 4; i++) {
                vb[((i * 4 + 0) * KC + e) * P] = s[i * 4 + 0] - s[i * 4 + 2];
                vb[((i * 4 + 1) * KC + e) * P] = s[i * 4 + 1] + s[i * 4 + 2];
                vb[((i * 4 + 2) * KC + e) * P] = s[i * 4 + 2] - s[i * 4 + 1];
                vb[((i * 4 + 3) * KC + e) * P] = s[i * 4 + 1] - s[i * 4 + 3];
            }
        }
    };

    // ---- the filter operand of this wave: U laid out [nb][chunk][position][j][kq][lane] float4 (winograd.py)
    wf32x4_t ub[4][KQ][NB];
    const wf32x4_t* const ubase = reinterpret_cast<const wf32x4_t*>(U) + (size_t)nb * nchunks * (16 * NB * KQ * 64) + lane;
    auto u_ptr = [&](int chunk, int pl, int kq, int j) {
        return ubase + ((size_t)((chunk * 16 + wave * 4 + pl) * NB + j) * KQ + kq) * 64;
    };

    wf32x16_t acc[4][2][NB];
#pragma unroll
    for (int pl = 0; pl < 4; pl++)
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int j = 0; j < NB; j++)
#pragma unroll
                for (int r = 0; r < 16; r++) acc[pl][i][j][r] = 0.0f;

    fetch_x(0);
#pragma unroll
    for (int pl = 0; pl < 4; pl++)
#pragma unroll
        for (int kq = 0; kq < KQ; kq++)
#pragma unroll
            for (int j = 0; j < NB; j++) ub[pl][kq][j] = *u_ptr(0, pl, kq, j);
    transform_store(0);
    __syncthreads();

    const int a_lane = (lane >> 5) * P + (lane & 31);
    // the sixteen GEMM steps of one chunk for this wave's four positions; every filter register group is reloaded for chunk
    // `nxt` right behind its last use (nxt < 0: the last chunk, nothing to reload)
    auto mfma_phase = [&](int chunk, int nxt) {
        const float* const vb = lds + (chunk & 1) * C::VBUF + a_lane;
#pragma unroll
        for (int pl = 0; pl < 4; pl++) {
            const float* const vp = vb + ((wave * 4 + pl) * KC) * P;
#pragma unroll
            for (int kq = 0; kq < KQ; kq++) {
#pragma unroll
                for (int m = 0; m < 4; m++) {
                    const int kp = kq * 4 + m;
                    const float a0 = vp[(2 * kp) * P], a1 = vp[(2 * kp) * P + 32];
#pragma unroll
                    for (int j = 0; j < NB; j++) {
                        acc[pl][0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, ub[pl][kq][j][m], acc[pl][0][j], 0, 0, 0);
                        acc[pl][1][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, ub[pl][kq][j][m], acc[pl][1][j], 0, 0, 0);
                    }
                }
                if (nxt >= 0) {
#pragma unroll
                    for (int j = 0; j < NB; j++) ub[pl][kq][j] = *u_ptr(nxt, pl, kq, j);
                }
            }
        }
    };
    // (the last chunk is peeled off: with `if (more)` around the transform the optimiser sinks the loads of fetch_x into that
    // block, i.e. behind the MFMA phase, and the memory latency of every chunk is exposed)
    for (int chunk = 0; chunk + 1 < nchunks; chunk++) {
        fetch_x(chunk + 1);
        __builtin_amdgcn_sched_barrier(0);
        mfma_phase(chunk, chunk + 1);
        __builtin_amdgcn_sched_barrier(0);
        transform_store((chunk + 1) & 1);
        __syncthreads();
    }
    mfma_phase(nchunks - 1, -1);
    __syncthreads();

    // ---- output transform.  nu-sum in registers: P0 = m0 + m1 + m2, P1 = m1 - m2 - m3 (A^T = [1 1 1 0; 0 1 -1 -1])
    float* const sw = lds + wave * (2 * 64 * BN);
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < NB; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int tile = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                const int col = j * 32 + (lane & 31);
                const float m0 = acc[0][i][j][r], m1 = acc[1][i][j][r], m2 = acc[2][i][j][r], m3 = acc[3][i][j][r];
                sw[tile * BN + col] = (m0 + m1) + m2;
                sw[64 * BN + tile * BN + col] = (m1 - m2) - m3;
            }
    __syncthreads();
    // xi-sum across the waves: Y[0][.] = P(0) + P(1) + P(2), Y[1][.] = P(1) - P(2) - P(3); item = (tile, 4 channels)
    constexpr int V4 = BN / 4;
#pragma unroll
    for (int it = 0; it < 64 * V4 / 256; it++) {
        const int item = it * 256 + tid;
        const int tile = item / V4, c4 = (item % V4) * 4;
        const int tt = tb * 64 + tile;
        if (tt >= T) continue;
        const int ox = tt % TW, oy = (tt / TW) % TH, on = tt / (TW * TH);
        wf32x4_t pq[4][2];
#pragma unroll
        for (int w = 0; w < 4; w++)
#pragma unroll
            for (int jj = 0; jj < 2; jj++)
                pq[w][jj] = *reinterpret_cast<const wf32x4_t*>(lds + (w * 2 + jj) * (64 * BN) + tile * BN + c4);
        wf32x4_t bv = {0.f, 0.f, 0.f, 0.f};
        if (bias) bv = *reinterpret_cast<const wf32x4_t*>(bias + nb * BN + c4);
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int oh = 2 * oy + i;
            if (oh >= H) continue;
#pragma unroll
            for (int jj = 0; jj < 2; jj++) {
                const int ow = 2 * ox + jj;
                if (ow >= W) continue;
                wf32x4_t v = i == 0 ? (pq[0][jj] + pq[1][jj]) + pq[2][jj] : (pq[1][jj] - pq[2][jj]) - pq[3][jj];
                v += bv;
                if (relu) {
#pragma unroll
                    for (int e = 0; e < 4; e++) v[e] = fmaxf(v[e], 0.0f);
                }
                *reinterpret_cast<wf32x4_t*>(y + ((size_t)(on * H + oh) * W + ow) * Cout + nb * BN + c4) = v;
            }
        }
    }
}

// ---- variant 2: the same 64 tiles x 64 channels with EIGHT waves (512 threads), two per SIMD, in two shifts.
// Variant 0's single wave per SIMD does its transform and its LDS round trips in front of the idle MFMA pipe (the compiler
// schedules them behind the multiplications whatever the source says: 20 % + 20 % of a chunk).  Here wave w owns TWO positions
// (xi = w / 2, nu = 2 * (w % 2) + {0, 1}: 128 accumulator registers), waves w and w + 4 share a SIMD, and the two halves of
// the workgroup take the phases of a chunk in opposite order:
//     waves 0-3:  fetch x(c + 1) | multiply chunk c                | transform x(c + 1) -> other stage | barrier
//     waves 4-7:  transform x(c + 1) -> other stage | fetch x(c + 2) | multiply chunk c                 | barrier
// so that one wave of every SIMD has MFMAs to issue while the other one adds, stores and waits for LDS.  Same filter layout
// as variant 0.  Thread (tile = tid / 8, channel pair = tid % 8) stages float2's; LDS pitch 66 is conflict-free for that map.
// Output transform in two halves of 32 tiles (8 waves x 2 x 32 x 64 floats = 128 KB per half).
constexpr int kW8KC = 16, kW8P = 66, kW8VBUF = 16 * kW8KC * kW8P;
constexpr int kW8LdsBytes = 2 * kW8VBUF * 4;            // 135 168 B (>= the 131 072 B of an output half)

template <int DIAG>
__global__ __launch_bounds__(512, 1) void winograd_f23_w8_kernel(
        const float* __restrict__ x, const float* __restrict__ U, float* __restrict__ y, const float* __restrict__ bias,
        int H, int W, int Cin, int Cout, int TH, int TW, int T, int relu, int nb_major) {
    constexpr int KC = kW8KC, P = kW8P, NB = 2, BN = 64, KQ = 2, S = 2 * KQ;
    extern __shared__ __attribute__((aligned(16))) unsigned char wino_smem[];
    float* const lds = reinterpret_cast<float*>(wino_smem);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_nb = Cout / BN;
    const unsigned nwg = gridDim.x, xcd = blockIdx.x & 7u, in_xcd = blockIdx.x >> 3;
    const unsigned q8 = nwg >> 3, r8 = nwg & 7u;
    const unsigned logical = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + in_xcd;
    const unsigned n_tb = nwg / (unsigned)n_nb;
    const int tb = nb_major ? (int)(logical % n_tb) : (int)(logical / (unsigned)n_nb);
    const int nb = nb_major ? (int)(logical / n_tb) : (int)(logical % (unsigned)n_nb);
    const int nchunks = Cin / KC;

    const int tile_l = tid >> 3, cg = tid & 7;
    int t = tb * 64 + tile_l;
    if (t > T - 1) t = T - 1;
    const int tx = t % TW, ty = (t / TW) % TH, n = t / (TW * TH);
    // byte offsets of the tile's sixteen pixels (clamped into the image), once: a fetch is then sixteen loads of the form
    // uniform base (x + chunk * KC, scalar registers) + 32-bit lane offset -- no address arithmetic in the loop
    unsigned off[16];
    unsigned valid = 0u;                               // bit i * 4 + j: pixel (i, j) lies inside the image
    {
        unsigned rowoff[4], coloff[4];
        bool rv[4], cv[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int r = 2 * ty - 1 + i, c = 2 * tx - 1 + i;
            rv[i] = r >= 0 && r < H;
            cv[i] = c >= 0 && c < W;
            const int rc = r < 0 ? 0 : (r > H - 1 ? H - 1 : r), cc = c < 0 ? 0 : (c > W - 1 ? W - 1 : c);
            rowoff[i] = (unsigned)((n * H + rc) * W) * (unsigned)Cin;
            coloff[i] = (unsigned)cc * (unsigned)Cin + (unsigned)(cg * 2);
        }
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                off[i * 4 + j] = (rowoff[i] + coloff[j]) * 4u;
                if (rv[i] && cv[j]) valid |= 1u << (i * 4 + j);
            }
    }
    const bool wave_inside = __ballot(valid != 0xffffu) == 0ull;   // no lane of this wave has a pixel in the padding
    float d[16][2];
    auto fetch_x = [&](int chunk) {
        const char* const base = reinterpret_cast<const char*>(x + chunk * KC);
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const float2 v = *reinterpret_cast<const float2*>(base + off[k]);
            d[k][0] = v.x; d[k][1] = v.y;
        }
    };
    auto transform_store = [&](int buf) {
        float* const vb = lds + buf * kW8VBUF + (cg * 2) * P + tile_l;
        if (!wave_inside) {                            // zero padding: only the waves that hold a border tile pay for it
#pragma unroll
            for (int k = 0; k < 16; k++)
                if (!((valid >> k) & 1u)) { d[k][0] = 0.0f; d[k][1] = 0.0f; }
        }
#pragma unroll
        for (int e = 0; e < 2; e++) {
            float s[16];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                s[0 * 4 + j] = d[0 * 4 + j][e] - d[2 * 4 + j][e];
                s[1 * 4 + j] = d[1 * 4 + j][e] + d[2 * 4 + j][e];
                s[2 * 4 + j] = d[2 * 4 + j][e] - d[1 * 4 + j][e];
                s[3 * 4 + j] = d[1 * 4 + j][e] - d[3 * 4 + j][e];
            }
#pragma unroll
            for (int i = 0; i < 4; i++) {
                vb[((i * 4 + 0) * KC + e) * P] = s[i * 4 + 0] - s[i * 4 + 2];
                vb[((i * 4 + 1) * KC + e) * P] = s[i * 4 + 1] + s[i * 4 + 2];
                vb[((i * 4 + 2) * KC + e) * P] = s[i * 4 + 2] - s[i * 4 + 1];
                vb[((i * 4 + 3) * KC + e) * P] = s[i * 4 + 1] - s[i * 4 + 3];
            }
        }
    };

    // filter operand: step st = (position 2 * wave + st / KQ, kq = st % KQ); all four steps of a chunk in registers, each
    // reloaded for the next chunk behind its last MFMA
    wf32x4_t ub[S][NB];
    const wf32x4_t* const ubase = reinterpret_cast<const wf32x4_t*>(U) + (size_t)nb * nchunks * (16 * NB * KQ * 64) + lane;
    auto u_ptr = [&](int chunk, int st, int j) {
        return ubase + ((size_t)((chunk * 16 + wave * 2 + st / KQ) * NB + j) * KQ + st % KQ) * 64;
    };
    wf32x16_t acc[2][2][NB];
#pragma unroll
    for (int pl = 0; pl < 2; pl++)
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int j = 0; j < NB; j++)
#pragma unroll
                for (int r = 0; r < 16; r++) acc[pl][i][j][r] = 0.0f;

    const int a_lane = (lane >> 5) * P + (lane & 31) + (wave * 2 * KC) * P;
    auto mfma_phase = [&](int chunk, int nxt) {
        const float* const vb = lds + (chunk & 1) * kW8VBUF + a_lane;
#pragma unroll
        for (int st = 0; st < S; st++) {
            const int pl = st / KQ;
            const float* const vp = vb + (pl * KC + (st % KQ) * 8) * P;
#pragma unroll
            for (int m = 0; m < 4; m++) {
                const float a0 = DIAG == 5 ? ub[st][0][m] : vp[(2 * m) * P], a1 = DIAG == 5 ? ub[st][1][m] : vp[(2 * m) * P + 32];
#pragma unroll
                for (int j = 0; j < NB; j++) {
                    acc[pl][0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, ub[st][j][m], acc[pl][0][j], 0, 0, 0);
                    acc[pl][1][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, ub[st][j][m], acc[pl][1][j], 0, 0, 0);
                }
            }
            if (DIAG != 1 && DIAG != 4 && DIAG != 5) {
#pragma unroll
                for (int j = 0; j < NB; j++) ub[st][j] = *u_ptr(nxt, st, j);
            }
        }
    };

    // Prologue in the loops' own order of loads -- pixels first, filter behind them: the compiler's s_waitcnt at a loop head
    // covers the entry edge as well, and with the filter loads issued first the second shift's `wait for the pixels` became
    // vmcnt(0), i.e. every period began by waiting for the filter reloads issued at the end of the period before.
    const int last = nchunks - 1;
    fetch_x(0);
    transform_store(0);
    __builtin_amdgcn_sched_barrier(0);
    if (wave >= 4) fetch_x(nchunks > 1 ? 1 : 0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int st = 0; st < S; st++)
#pragma unroll
        for (int j = 0; j < NB; j++) ub[st][j] = *u_ptr(0, st, j);
    __builtin_amdgcn_sched_barrier(0);
    if (wave < 4) {                                    // first shift: multiply, then transform
        __syncthreads();
        for (int chunk = 0; chunk < nchunks; chunk++) {
            const int nxt = chunk < last ? chunk + 1 : last;
            if (DIAG != 2 && DIAG != 4 && DIAG != 5) fetch_x(nxt);
            __builtin_amdgcn_sched_barrier(0);
            mfma_phase(chunk, nxt);
            __builtin_amdgcn_sched_barrier(0);
            if (DIAG != 3 && DIAG != 4 && DIAG != 5) transform_store((chunk + 1) & 1);          // (the last chunk's goes to the stage nobody reads any more)
            __syncthreads();
        }
    } else {                                           // second shift: transform, then multiply
        __syncthreads();
        for (int chunk = 0; chunk < nchunks; chunk++) {
            const int nxt = chunk < last ? chunk + 1 : last;
            if (DIAG != 3 && DIAG != 4 && DIAG != 5) transform_store((chunk + 1) & 1);
            __builtin_amdgcn_sched_barrier(0);
            if (DIAG != 2 && DIAG != 4 && DIAG != 5) fetch_x(chunk + 2 < nchunks ? chunk + 2 : last);
            __builtin_amdgcn_sched_barrier(0);
            mfma_phase(chunk, nxt);
            __syncthreads();
        }
    }

    if (DIAG == 6) {                                   // timing experiment: no output transform (one store keeps the MFMAs alive)
        float sum = 0.0f;
#pragma unroll
        for (int pl = 0; pl < 2; pl++)
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < NB; j++)
#pragma unroll
                    for (int r = 0; r < 16; r++) sum += acc[pl][i][j][r];
        if (sum == 12345.678f) y[0] = sum;
        return;
    }
    // ---- output transform, 32 tiles (accumulator row block i) at a time.  This wave's part of the nu-sum:
    //      nu in {0, 1}: P0 = m0 + m1, P1 = m1;   nu in {2, 3}: P0 = m2, P1 = -(m2 + m3)
    const int h = wave & 1;
#pragma unroll
    for (int i = 0; i < 2; i++) {
        float* const sw = lds + wave * (2 * 32 * BN);
#pragma unroll
        for (int j = 0; j < NB; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int tile = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                const int col = j * 32 + (lane & 31);
                const float ma = acc[0][i][j][r], mb = acc[1][i][j][r];
                sw[tile * BN + col] = h == 0 ? ma + mb : ma;
                sw[32 * BN + tile * BN + col] = h == 0 ? mb : -(ma + mb);
            }
        __syncthreads();
        // item = (tile of this half, 4 channels): 32 x 16 = 512 = one per thread.  xi-sum over the wave pairs:
        //      Y[0][.] = P(0) + P(1) + P(2), Y[1][.] = P(1) - P(2) - P(3), P(xi) = the two waves 2 xi, 2 xi + 1
        {
            const int tile = tid >> 4, c4 = (tid & 15) * 4;
            const int tt = tb * 64 + i * 32 + tile;
            if (tt < T) {
                const int ox = tt % TW, oy = (tt / TW) % TH, on = tt / (TW * TH);
                wf32x4_t pq[4][2];
#pragma unroll
                for (int xi = 0; xi < 4; xi++)
#pragma unroll
                    for (int jj = 0; jj < 2; jj++)
                        pq[xi][jj] = *reinterpret_cast<const wf32x4_t*>(lds + ((2 * xi) * 2 + jj) * (32 * BN) + tile * BN + c4) +
                                     *reinterpret_cast<const wf32x4_t*>(lds + ((2 * xi + 1) * 2 + jj) * (32 * BN) + tile * BN + c4);
                wf32x4_t bv = {0.f, 0.f, 0.f, 0.f};
                if (bias) bv = *reinterpret_cast<const wf32x4_t*>(bias + nb * BN + c4);
#pragma unroll
                for (int a = 0; a < 2; a++) {
                    const int oh = 2 * oy + a;
                    if (oh >= H) continue;
#pragma unroll
                    for (int jj = 0; jj < 2; jj++) {
                        const int ow = 2 * ox + jj;
                        if (ow >= W) continue;
                        wf32x4_t v = a == 0 ? (pq[0][jj] + pq[1][jj]) + pq[2][jj] : (pq[1][jj] - pq[2][jj]) - pq[3][jj];
                        v += bv;
                        if (relu) {
#pragma unroll
                            for (int e = 0; e < 4; e++) v[e] = fmaxf(v[e], 0.0f);
                        }
                        if (DIAG != 7 || v[0] == 12345.678f)       // (7: timing experiment, the output transform without its stores)
                            {
                            wf32x4_t* const dst = reinterpret_cast<wf32x4_t*>(y + ((size_t)(on * H + oh) * W + ow) * Cout + nb * BN + c4);
                            if (DIAG == 8) __builtin_nontemporal_store(v, dst); else *dst = v;   // (8: timing experiment, nontemporal stores)
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
}

// ---- variant 4: variant 2 on the bf16 MFMA pipe with exactly split operands (the scheme of gemm_f32x3.hip).  The float32
// MFMA runs at 1/16 of the bf16 rate; a float32 number is exactly the sum of three bf16 pieces, and the six leading of the nine
// piece products (the three left out are below 2^-23 of the product each) cost 6 x v_mfma_f32_32x32x16_bf16 at 32 cycles
// against 8 x v_mfma_f32_32x32x2f32 at 64 per 32x32x16 block: 0.375 of the MFMA cycles.  Everything but the products is
// variant 2's (tile, shifts, staging, LDS layout, output transform).  The operand maps fit the bf16 MFMA as they are: lane l
// (h = l / 32) of a 32x32x16 bf16 fragment holds virtual k' = 8 h + j, j = 0..7; variant 2's lane reads real k = 2 j + h
// of the chunk (LDS rows 8 kq + 2 m + h) in its j = 4 kq + m-th float32 MFMA -- so the chunk is ONE bf16 K-step under the
// permutation k' = 8 h + j <-> k = 2 j + h, applied to both operands alike.
//   * V is split when its fragment is read from LDS (each element is read by one lane of one wave: split once);
//   * U is split on the host (winograd.split_filter: [nb][chunk][position][j][piece][lane] x 16 B), 48 registers per wave;
//   * ONE accumulator set: the leading product and then the five corrections (smallest first) go into `acc` -- a second set
//     for the corrections, as gemm_f32x3.hip keeps, does not fit beside the 48 filter registers (128 more), and adding a zeroed
//     block of corrections per K-step spilled (the register report of the build: 492 B per lane).  Six roundings per 16 k
//     against the float32 MFMA's eight; the error against float64 is measured beside variant 2's
//     (tests/test_gpu_winograd_x3.py, tools/gpu/winograd_x3_probe.py).
// DIAG (timing experiments, wrong results; OPA_WINO_DIAG builds): 1 no split (the raw bits as every piece), 2 the leading
// products only, 3 no pixel fetches and no transforms (MFMA + operand reads + split).
template <int DIAG>
__global__ __launch_bounds__(512, 1) void winograd_f23_w8x3_kernel(
        const float* __restrict__ x, const unsigned short* __restrict__ U3, float* __restrict__ y, const float* __restrict__ bias,
        int H, int W, int Cin, int Cout, int TH, int TW, int T, int relu, int nb_major) {
    constexpr int KC = kW8KC, P = kW8P, NB = 2, BN = 64;
    typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
    typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;
    extern __shared__ __attribute__((aligned(16))) unsigned char wino_smem[];
    float* const lds = reinterpret_cast<float*>(wino_smem);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_nb = Cout / BN;
    const unsigned nwg = gridDim.x, xcd = blockIdx.x & 7u, in_xcd = blockIdx.x >> 3;
    const unsigned q8 = nwg >> 3, r8 = nwg & 7u;
    const unsigned logical = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + in_xcd;
    const unsigned n_tb = nwg / (unsigned)n_nb;
    const int tb = nb_major ? (int)(logical % n_tb) : (int)(logical / (unsigned)n_nb);
    const int nb = nb_major ? (int)(logical / n_tb) : (int)(logical % (unsigned)n_nb);
    const int nchunks = Cin / KC;

    const int tile_l = tid >> 3, cg = tid & 7;
    int t = tb * 64 + tile_l;
    if (t > T - 1) t = T - 1;
    const int tx = t % TW, ty = (t / TW) % TH, n = t / (TW * TH);
    // byte offsets of the tile's four rows and four columns (clamped into the image).  The pixels come through buffer loads:
    // descriptor and chunk offset in scalar registers, ONE 32-bit register per load, the row + column sum formed in the loop
    // (kept opaque to the optimiser, which would otherwise hoist sixteen sums -- as 64-bit addresses of global loads they took
    // 32 registers, which the split filter operand needs)
    unsigned rowoff[4], coloff[4];
    unsigned valid = 0u;                               // bit i * 4 + j: pixel (i, j) lies inside the image
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int r = 2 * ty - 1 + i, c = 2 * tx - 1 + i;
        const int rc = r < 0 ? 0 : (r > H - 1 ? H - 1 : r), cc = c < 0 ? 0 : (c > W - 1 ? W - 1 : c);
        rowoff[i] = (unsigned)((n * H + rc) * W) * (unsigned)Cin * 4u;
        coloff[i] = ((unsigned)cc * (unsigned)Cin + (unsigned)(cg * 2)) * 4u;
        if (r >= 0 && r < H) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int cj = 2 * tx - 1 + j;
                if (cj >= 0 && cj < W) valid |= 1u << (i * 4 + j);
            }
        }
    }
    const bool wave_inside = __ballot(valid != 0xffffu) == 0ull;
    // (the activation is below 2^30 elements -- the launcher checks -- and every offset is clamped into it)
    const unsigned x_bytes = (unsigned)(T / (TH * TW)) * (unsigned)(H * W) * (unsigned)Cin * 4u;
    const __amdgpu_buffer_rsrc_t x_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x), 0, (int)x_bytes, 0x00020000);
    float d[16][2];
    auto fetch_x = [&](int chunk) {
        unsigned ro[4];
#pragma unroll
        for (int i = 0; i < 4; i++) { ro[i] = rowoff[i]; asm volatile("" : "+v"(ro[i])); }
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const u32x2_t v = __builtin_bit_cast(u32x2_t, __builtin_amdgcn_raw_buffer_load_b64(x_rsrc, ro[k >> 2] + coloff[k & 3],
                                                                                               chunk * KC * 4, 0));
            d[k][0] = __uint_as_float(v[0]); d[k][1] = __uint_as_float(v[1]);
        }
    };
    auto transform_store = [&](int buf) {
        float* const vb = lds + buf * kW8VBUF + (cg * 2) * P + tile_l;
        if (!wave_inside) {
#pragma unroll
            for (int k = 0; k < 16; k++)
                if (!((valid >> k) & 1u)) { d[k][0] = 0.0f; d[k][1] = 0.0f; }
        }
#pragma unroll
        for (int e = 0; e < 2; e++) {
            float s[16];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                s[0 * 4 + j] = d[0 * 4 + j][e] - d[2 * 4 + j][e];
                s[1 * 4 + j] = d[1 * 4 + j][e] + d[2 * 4 + j][e];
                s[2 * 4 + j] = d[2 * 4 + j][e] - d[1 * 4 + j][e];
                s[3 * 4 + j] = d[1 * 4 + j][e] - d[3 * 4 + j][e];
            }
#pragma unroll
            for (int i = 0; i < 4; i++) {
                vb[((i * 4 + 0) * KC + e) * P] = s[i * 4 + 0] - s[i * 4 + 2];
                vb[((i * 4 + 1) * KC + e) * P] = s[i * 4 + 1] + s[i * 4 + 2];
                vb[((i * 4 + 2) * KC + e) * P] = s[i * 4 + 2] - s[i * 4 + 1];
                vb[((i * 4 + 3) * KC + e) * P] = s[i * 4 + 1] - s[i * 4 + 3];
            }
        }
    };

    // filter operand: position pl = 0, 1 of this wave (2 * wave + pl), channel half j, piece q; reloaded for the next chunk
    // behind the position's last MFMA
    u32x4_t ub[2][NB][3];
    const __amdgpu_buffer_rsrc_t u_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<unsigned short*>(U3 + (size_t)nb * nchunks * (16 * NB * 3 * 64 * 8)), 0, nchunks * (16 * NB * 3 * 64 * 16), 0x00020000);
    const unsigned u_lane = (unsigned)lane * 16u;
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);     // (uniform: the scalar offset of the filter loads)
    auto u_load = [&](int chunk, int pl, int j, int q) {
        return __builtin_bit_cast(u32x4_t, __builtin_amdgcn_raw_buffer_load_b128(
            u_rsrc, u_lane, ((((chunk * 16 + wave_s * 2 + pl) * NB + j) * 3 + q) * 64) * 16, 0));
    };
    wf32x16_t acc[2][2][NB];
#pragma unroll
    for (int pl = 0; pl < 2; pl++)
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int j = 0; j < NB; j++)
#pragma unroll
                for (int r = 0; r < 16; r++) acc[pl][i][j][r] = 0.0f;

    const int a_lane = (lane >> 5) * P + (lane & 31) + (wave * 2 * KC) * P;
    auto mfma_phase = [&](int chunk, int nxt) {
        const float* const vb = lds + (chunk & 1) * kW8VBUF + a_lane;
#pragma unroll
        for (int pl = 0; pl < 2; pl++) {
            const float* const vp = vb + (pl * KC) * P;
#pragma unroll
            for (int i = 0; i < 2; i++) {
                __builtin_amdgcn_sched_barrier(0);
                // fragment element j = 4 kq + m <- LDS row 8 kq + 2 m + h (= real k 2 j + h), tile 32 i + lane % 32
                wf32x4_t lo, hi;
#pragma unroll
                for (int m = 0; m < 4; m++) { lo[m] = vp[(2 * m) * P + 32 * i]; hi[m] = vp[(8 + 2 * m) * P + 32 * i]; }
                u32x2_t l1, l2, l3, h1, h2, h3;
                if (DIAG == 1) {
                    l1[0] = __float_as_uint(lo[0]); l1[1] = __float_as_uint(lo[2]); h1[0] = __float_as_uint(hi[0]); h1[1] = __float_as_uint(hi[2]);
                    l2 = l1; l3 = l1; h2 = h1; h3 = h1;
                } else {
                    split4(lo, l1, l2, l3);
                    split4(hi, h1, h2, h3);
                }
                const bf16x8_t a[3] = {__builtin_bit_cast(bf16x8_t, (u32x4_t){l1[0], l1[1], h1[0], h1[1]}),
                                       __builtin_bit_cast(bf16x8_t, (u32x4_t){l2[0], l2[1], h2[0], h2[1]}),
                                       __builtin_bit_cast(bf16x8_t, (u32x4_t){l3[0], l3[1], h3[0], h3[1]})};
#pragma unroll
                for (int j = 0; j < NB; j++) {
                    const bf16x8_t b[3] = {__builtin_bit_cast(bf16x8_t, ub[pl][j][0]), __builtin_bit_cast(bf16x8_t, ub[pl][j][1]),
                                           __builtin_bit_cast(bf16x8_t, ub[pl][j][2])};
                    // the leading product, then the corrections smallest first, all into `acc` (see the header)
                    acc[pl][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], acc[pl][i][j], 0, 0, 0);
                    if (DIAG == 2) continue;
                    acc[pl][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[2], acc[pl][i][j], 0, 0, 0);
                    acc[pl][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], acc[pl][i][j], 0, 0, 0);
                    acc[pl][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[0], acc[pl][i][j], 0, 0, 0);
                    acc[pl][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], acc[pl][i][j], 0, 0, 0);
                    acc[pl][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], acc[pl][i][j], 0, 0, 0);
                }
            }
            if (DIAG != 3) {
#pragma unroll
                for (int j = 0; j < NB; j++)
#pragma unroll
                    for (int q = 0; q < 3; q++) ub[pl][j][q] = u_load(nxt, pl, j, q);
            }
        }
    };

    // prologue and the two shifts exactly as variant 2
    const int last = nchunks - 1;
    fetch_x(0);
    transform_store(0);
    __builtin_amdgcn_sched_barrier(0);
    if (wave >= 4) fetch_x(nchunks > 1 ? 1 : 0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int pl = 0; pl < 2; pl++)
#pragma unroll
        for (int j = 0; j < NB; j++)
#pragma unroll
            for (int q = 0; q < 3; q++) ub[pl][j][q] = u_load(0, pl, j, q);
    __builtin_amdgcn_sched_barrier(0);
    if (wave < 4) {
        __syncthreads();
        for (int chunk = 0; chunk < nchunks; chunk++) {
            const int nxt = chunk < last ? chunk + 1 : last;
            if (DIAG != 3) fetch_x(nxt);
            __builtin_amdgcn_sched_barrier(0);
            mfma_phase(chunk, nxt);
            __builtin_amdgcn_sched_barrier(0);
            if (DIAG != 3) transform_store((chunk + 1) & 1);
            __syncthreads();
        }
    } else {
        __syncthreads();
        for (int chunk = 0; chunk < nchunks; chunk++) {
            const int nxt = chunk < last ? chunk + 1 : last;
            if (DIAG != 3) transform_store((chunk + 1) & 1);
            __builtin_amdgcn_sched_barrier(0);
            if (DIAG != 3) fetch_x(chunk + 2 < nchunks ? chunk + 2 : last);
            __builtin_amdgcn_sched_barrier(0);
            mfma_phase(chunk, nxt);
            __syncthreads();
        }
    }

    // ---- output transform (variant 2's)
    const int h = wave & 1;
#pragma unroll
    for (int i = 0; i < 2; i++) {
        float* const sw = lds + wave * (2 * 32 * BN);
#pragma unroll
        for (int j = 0; j < NB; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int tile = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                const int col = j * 32 + (lane & 31);
                const float ma = acc[0][i][j][r], mb = acc[1][i][j][r];
                sw[tile * BN + col] = h == 0 ? ma + mb : ma;
                sw[32 * BN + tile * BN + col] = h == 0 ? mb : -(ma + mb);
            }
        __syncthreads();
        {
            const int tile = tid >> 4, c4 = (tid & 15) * 4;
            const int tt = tb * 64 + i * 32 + tile;
            if (tt < T) {
                const int ox = tt % TW, oy = (tt / TW) % TH, on = tt / (TW * TH);
                wf32x4_t pq[4][2];
#pragma unroll
                for (int xi = 0; xi < 4; xi++)
#pragma unroll
                    for (int jj = 0; jj < 2; jj++)
                        pq[xi][jj] = *reinterpret_cast<const wf32x4_t*>(lds + ((2 * xi) * 2 + jj) * (32 * BN) + tile * BN + c4) +
                                     *reinterpret_cast<const wf32x4_t*>(lds + ((2 * xi + 1) * 2 + jj) * (32 * BN) + tile * BN + c4);
                wf32x4_t bv = {0.f, 0.f, 0.f, 0.f};
                if (bias) bv = *reinterpret_cast<const wf32x4_t*>(bias + nb * BN + c4);
#pragma unroll
                for (int a = 0; a < 2; a++) {
                    const int oh = 2 * oy + a;
                    if (oh >= H) continue;
#pragma unroll
                    for (int jj = 0; jj < 2; jj++) {
                        const int ow = 2 * ox + jj;
                        if (ow >= W) continue;
                        wf32x4_t v = a == 0 ? (pq[0][jj] + pq[1][jj]) + pq[2][jj] : (pq[1][jj] - pq[2][jj]) - pq[3][jj];
                        v += bv;
                        if (relu) {
#pragma unroll
                            for (int e = 0; e < 4; e++) v[e] = fmaxf(v[e], 0.0f);
                        }
                        *reinterpret_cast<wf32x4_t*>(y + ((size_t)(on * H + oh) * W + ow) * Cout + nb * BN + c4) = v;
                    }
                }
            }
        }
        __syncthreads();
    }
}

// ---- variant 5: variant 4 with workgroups of 32 tiles x 128 output channels.  Variant 4's loop is bound by the vector issue
// of its activation side (per MFMA 6.6 other vector instructions -- the bf16 split, B^T d B, address sums, the zeroing of the
// padding -- and every workgroup along the output channels does all of it again for the same tiles).  The same 4096
// tile x channel accumulators as 32 x 128 halve that work per MFMA: one activation fragment (8 values, split once) now feeds
// 24 MFMAs instead of 12.  Everything that decides a result is variant 4's -- per accumulator block the six products of a chunk
// in the same order, the chunks in the same order, the transforms' additions in the same order -- so the two are equal bit for
// bit (tests/test_gpu_winograd_x3_wide.py).  What differs:
//   * wave w keeps positions 2 w and 2 w + 1 for ONE block of 32 tiles and four channel blocks of 32: acc[2][4];
//   * thread (tile = tid / 16, channel = tid % 16) fetches its tile's sixteen pixels of one channel (dword buffer loads, 64 B
//     contiguous per tile and pixel as in variant 4); V[position][k][tile] has a pitch of 34: the stores (c * 34 + tile,
//     two tiles per 32 lanes) and the operand reads (32 consecutive tiles) meet no bank twice;
//   * a pixel in the padding is given an offset past the descriptor's range, which loads as zero: no select, no mask in the
//     loop.  kW8WRowOut + kW8WColOut + any valid offset stays below 2^32 and every sum with one of them lies at or above
//     kW8WMaxBytes, which the launcher holds the activation under;
//   * the filter operand is variant 4's (split_filter: channel halves j = 0, 1 from the 64-channel block 2 nb, j = 2, 3 from
//     2 nb + 1).  A chunk's eight (position, j) fragments of 12 registers do not fit; four are kept, fragment (pl, j) is
//     reloaded with (pl ^ 1, j) -- of the next chunk behind position 1 -- right behind its six MFMAs, i.e. three fragments
//     (72 MFMAs) ahead of its use, the same loads in the same order in every iteration (variant 3's comment: static waits);
//   * output transform: variant 4's, per 64-channel half instead of per 32-tile half (the same 128 KB of staging).
constexpr int kW8WP = 34, kW8WVBUF = 16 * kW8KC * kW8WP;
constexpr unsigned kW8WRowOut = 0x80000000u, kW8WColOut = 0x40000000u, kW8WMaxBytes = 0x40000000u;
constexpr int kW8WLdsBytes = 8 * 2 * 32 * 64 * 4;       // 131 072 B: an output half (>= the 69 632 B of the two stages)
static_assert(kW8WLdsBytes <= kW8LdsBytes && 2 * kW8WVBUF * 4 <= kW8WLdsBytes, "the wide kernel's LDS");

__global__ __launch_bounds__(512, 1) void winograd_f23_w8x3w_kernel(
        const float* __restrict__ x, const unsigned short* __restrict__ U3, float* __restrict__ y, const float* __restrict__ bias,
        int H, int W, int Cin, int Cout, int TH, int TW, int T, int relu, int nb_major) {
    constexpr int KC = kW8KC, P = kW8WP, NB = 4, BN = 128, TB = 32, HB = 64;
    typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
    typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;
    extern __shared__ __attribute__((aligned(16))) unsigned char wino_smem[];
    float* const lds = reinterpret_cast<float*>(wino_smem);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_nb = Cout / BN;
    const unsigned nwg = gridDim.x, xcd = blockIdx.x & 7u, in_xcd = blockIdx.x >> 3;
    const unsigned q8 = nwg >> 3, r8 = nwg & 7u;
    const unsigned logical = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + in_xcd;
    const unsigned n_tb = nwg / (unsigned)n_nb;
    const int tb = nb_major ? (int)(logical % n_tb) : (int)(logical / (unsigned)n_nb);
    const int nb = nb_major ? (int)(logical / n_tb) : (int)(logical % (unsigned)n_nb);
    const int nchunks = Cin / KC;

    const int tile_l = tid >> 4, cl = tid & 15;
    int t = tb * TB + tile_l;
    if (t > T - 1) t = T - 1;
    const int tx = t % TW, ty = (t / TW) % TH, n = t / (TW * TH);
    // byte offsets of the tile's four rows and four columns; one outside the image is out of the descriptor's range with
    // every partner.  Buffer loads as in variant 4: the row + column sum is formed in the loop, opaque to the optimiser.
    unsigned rowoff[4], coloff[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int r = 2 * ty - 1 + i, c = 2 * tx - 1 + i;
        rowoff[i] = r >= 0 && r < H ? (unsigned)((n * H + r) * W) * (unsigned)Cin * 4u : kW8WRowOut;
        coloff[i] = c >= 0 && c < W ? ((unsigned)c * (unsigned)Cin + (unsigned)cl) * 4u : kW8WColOut;
    }
    const unsigned x_bytes = (unsigned)(T / (TH * TW)) * (unsigned)(H * W) * (unsigned)Cin * 4u;     // (<= kW8WMaxBytes: the launcher)
    const __amdgpu_buffer_rsrc_t x_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x), 0, (int)x_bytes, 0x00020000);
    float d[16];
    auto fetch_x = [&](int chunk) {
        unsigned ro[4];
#pragma unroll
        for (int i = 0; i < 4; i++) { ro[i] = rowoff[i]; asm volatile("" : "+v"(ro[i])); }
#pragma unroll
        for (int k = 0; k < 16; k++)
            d[k] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(x_rsrc, ro[k >> 2] + coloff[k & 3], chunk * KC * 4, 0));
    };
    auto transform_store = [&](int buf) {
        float* const vb = lds + buf * kW8WVBUF + cl * P + tile_l;
        float s[16];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            s[0 * 4 + j] = d[0 * 4 + j] - d[2 * 4 + j];
            s[1 * 4 + j] = d[1 * 4 + j] + d[2 * 4 + j];
            s[2 * 4 + j] = d[2 * 4 + j] - d[1 * 4 + j];
            s[3 * 4 + j] = d[1 * 4 + j] - d[3 * 4 + j];
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            vb[((i * 4 + 0) * KC) * P] = s[i * 4 + 0] - s[i * 4 + 2];
            vb[((i * 4 + 1) * KC) * P] = s[i * 4 + 1] + s[i * 4 + 2];
            vb[((i * 4 + 2) * KC) * P] = s[i * 4 + 2] - s[i * 4 + 1];
            vb[((i * 4 + 3) * KC) * P] = s[i * 4 + 1] - s[i * 4 + 3];
        }
    };

    // filter operand: the four channel blocks j of ONE position at a time (see the header), piece q
    u32x4_t ub[NB][3];
    const __amdgpu_buffer_rsrc_t u_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<unsigned short*>(U3 + (size_t)(2 * nb) * nchunks * (16 * 2 * 3 * 64 * 8)), 0, 2 * nchunks * (16 * 2 * 3 * 64 * 16), 0x00020000);
    const unsigned u_lane = (unsigned)lane * 16u;
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);
    auto u_load = [&](int chunk, int pl, int j, int q) {
        return __builtin_bit_cast(u32x4_t, __builtin_amdgcn_raw_buffer_load_b128(
            u_rsrc, u_lane, ((((((j >> 1) * nchunks + chunk) * 16 + wave_s * 2 + pl) * 2 + (j & 1)) * 3 + q) * 64) * 16, 0));
    };
    wf32x16_t acc[2][NB];
#pragma unroll
    for (int pl = 0; pl < 2; pl++)
#pragma unroll
        for (int j = 0; j < NB; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[pl][j][r] = 0.0f;

    const int a_lane = (lane >> 5) * P + (lane & 31) + (wave * 2 * KC) * P;
    auto mfma_phase = [&](int chunk, int nxt) {
        const float* const vb = lds + (chunk & 1) * kW8WVBUF + a_lane;
#pragma unroll
        for (int pl = 0; pl < 2; pl++) {
            const float* const vp = vb + (pl * KC) * P;
            __builtin_amdgcn_sched_barrier(0);
            // fragment element j = 4 kq + m <- LDS row 8 kq + 2 m + h (= real k 2 j + h), tile lane % 32: variant 4's
            wf32x4_t lo, hi;
#pragma unroll
            for (int m = 0; m < 4; m++) { lo[m] = vp[(2 * m) * P]; hi[m] = vp[(8 + 2 * m) * P]; }
            u32x2_t l1, l2, l3, h1, h2, h3;
            split4(lo, l1, l2, l3);
            split4(hi, h1, h2, h3);
            const bf16x8_t a[3] = {__builtin_bit_cast(bf16x8_t, (u32x4_t){l1[0], l1[1], h1[0], h1[1]}),
                                   __builtin_bit_cast(bf16x8_t, (u32x4_t){l2[0], l2[1], h2[0], h2[1]}),
                                   __builtin_bit_cast(bf16x8_t, (u32x4_t){l3[0], l3[1], h3[0], h3[1]})};
#pragma unroll
            for (int j = 0; j < NB; j++) {
                const bf16x8_t b[3] = {__builtin_bit_cast(bf16x8_t, ub[j][0]), __builtin_bit_cast(bf16x8_t, ub[j][1]),
                                       __builtin_bit_cast(bf16x8_t, ub[j][2])};
                // variant 4's order: the leading product, then the corrections smallest first
                acc[pl][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], acc[pl][j], 0, 0, 0);
                acc[pl][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[2], acc[pl][j], 0, 0, 0);
                acc[pl][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], acc[pl][j], 0, 0, 0);
                acc[pl][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[0], acc[pl][j], 0, 0, 0);
                acc[pl][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], acc[pl][j], 0, 0, 0);
                acc[pl][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], acc[pl][j], 0, 0, 0);
#pragma unroll
                for (int q = 0; q < 3; q++) ub[j][q] = u_load(pl == 0 ? chunk : nxt, pl ^ 1, j, q);
                // (left to itself the scheduler gathers a position's twelve reloads behind its LAST MFMAs, three MFMAs ahead of
                // the wait for the first of them)
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };

    // prologue and the two shifts exactly as variant 2
    const int last = nchunks - 1;
    fetch_x(0);
    transform_store(0);
    __builtin_amdgcn_sched_barrier(0);
    if (wave >= 4) fetch_x(nchunks > 1 ? 1 : 0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < NB; j++)
#pragma unroll
        for (int q = 0; q < 3; q++) ub[j][q] = u_load(0, 0, j, q);
    __builtin_amdgcn_sched_barrier(0);
    if (wave < 4) {
        __syncthreads();
        for (int chunk = 0; chunk < nchunks; chunk++) {
            const int nxt = chunk < last ? chunk + 1 : last;
            fetch_x(nxt);
            __builtin_amdgcn_sched_barrier(0);
            mfma_phase(chunk, nxt);
            __builtin_amdgcn_sched_barrier(0);
            transform_store((chunk + 1) & 1);
            __syncthreads();
        }
    } else {
        __syncthreads();
        for (int chunk = 0; chunk < nchunks; chunk++) {
            const int nxt = chunk < last ? chunk + 1 : last;
            transform_store((chunk + 1) & 1);
            __builtin_amdgcn_sched_barrier(0);
            fetch_x(chunk + 2 < nchunks ? chunk + 2 : last);
            __builtin_amdgcn_sched_barrier(0);
            mfma_phase(chunk, nxt);
            __syncthreads();
        }
    }

    // ---- output transform (variant 2's), the 32 tiles x one 64-channel half (accumulator blocks 2 jh, 2 jh + 1) at a time
    const int h = wave & 1;
#pragma unroll
    for (int jh = 0; jh < 2; jh++) {
        float* const sw = lds + wave * (2 * 32 * HB);
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int tile = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                const int col = j * 32 + (lane & 31);
                const float ma = acc[0][2 * jh + j][r], mb = acc[1][2 * jh + j][r];
                sw[tile * HB + col] = h == 0 ? ma + mb : ma;
                sw[32 * HB + tile * HB + col] = h == 0 ? mb : -(ma + mb);
            }
        __syncthreads();
        {
            const int tile = tid >> 4, c4 = (tid & 15) * 4;
            const int tt = tb * TB + tile;
            if (tt < T) {
                const int ox = tt % TW, oy = (tt / TW) % TH, on = tt / (TW * TH);
                const int ch = nb * BN + jh * HB + c4;
                wf32x4_t pq[4][2];
#pragma unroll
                for (int xi = 0; xi < 4; xi++)
#pragma unroll
                    for (int jj = 0; jj < 2; jj++)
                        pq[xi][jj] = *reinterpret_cast<const wf32x4_t*>(lds + ((2 * xi) * 2 + jj) * (32 * HB) + tile * HB + c4) +
                                     *reinterpret_cast<const wf32x4_t*>(lds + ((2 * xi + 1) * 2 + jj) * (32 * HB) + tile * HB + c4);
                wf32x4_t bv = {0.f, 0.f, 0.f, 0.f};
                if (bias) bv = *reinterpret_cast<const wf32x4_t*>(bias + ch);
#pragma unroll
                for (int a = 0; a < 2; a++) {
                    const int oh = 2 * oy + a;
                    if (oh >= H) continue;
#pragma unroll
                    for (int jj = 0; jj < 2; jj++) {
                        const int ow = 2 * ox + jj;
                        if (ow >= W) continue;
                        wf32x4_t v = a == 0 ? (pq[0][jj] + pq[1][jj]) + pq[2][jj] : (pq[1][jj] - pq[2][jj]) - pq[3][jj];
                        v += bv;
                        if (relu) {
#pragma unroll
                            for (int e = 0; e < 4; e++) v[e] = fmaxf(v[e], 0.0f);
                        }
                        *reinterpret_cast<wf32x4_t*>(y + ((size_t)(on * H + oh) * W + ow) * Cout + ch) = v;
                    }
                }
            }
        }
        __syncthreads();
    }
}

// ---- variant 3: variant 2 as PERSISTENT workgroups.  With one workgroup per compute unit nothing overlaps a workgroup's
// prologue (the first pixels come from HBM: 2-3 us) -- a third of a workgroup's time at 64 input channels.  Here a workgroup
// walks tile blocks tb, tb + G, ... of ONE channel block, and during a block's LAST chunk both shifts fetch the first chunk
// of the NEXT block; its B^T d B is computed in registers before the output transform starts (so that the transform's
// stores are not in front of it in the vmcnt queue) and stored to stage 0 behind it.  Every iteration of the chunk loops
// issues the same loads in the same order (a chunk with nothing to fetch re-fetches its own pixels): the compiler's
// s_waitcnt counts are static, a load under a condition makes every wait behind the join conservative.
__global__ __launch_bounds__(512, 1) void winograd_f23_w8p_kernel(
        const float* __restrict__ x, const float* __restrict__ U, float* __restrict__ y, const float* __restrict__ bias,
        int H, int W, int Cin, int Cout, int TH, int TW, int T, int relu, int n_tb, int G) {
    constexpr int KC = kW8KC, P = kW8P, NB = 2, BN = 64, KQ = 2, S = 2 * KQ;
    extern __shared__ __attribute__((aligned(16))) unsigned char wino_smem[];
    float* const lds = reinterpret_cast<float*>(wino_smem);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_nb = Cout / BN;
    const unsigned nwg = gridDim.x, xcd = blockIdx.x & 7u, in_xcd = blockIdx.x >> 3;
    const unsigned q8 = nwg >> 3, r8 = nwg & 7u;
    const unsigned logical = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + in_xcd;
    const int nb = (int)(logical % (unsigned)n_nb);
    int tb = (int)(logical / (unsigned)n_nb);          // < G <= n_tb
    const int nchunks = Cin / KC, last = nchunks - 1;
    const bool shift_b = wave >= 4;

    const int tile_l = tid >> 3, cg = tid & 7;
    unsigned off[16];
    unsigned valid = 0u;
    auto set_block = [&](int blk) {                    // this thread's tile of block `blk`: pixel offsets and validity
        int t = blk * 64 + tile_l;
        if (t > T - 1) t = T - 1;
        const int tx = t % TW, ty = (t / TW) % TH, n = t / (TW * TH);
        unsigned rowoff[4], coloff[4];
        bool rv[4], cv[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int r = 2 * ty - 1 + i, c = 2 * tx - 1 + i;
            rv[i] = r >= 0 && r < H;
            cv[i] = c >= 0 && c < W;
            const int rc = r < 0 ? 0 : (r > H - 1 ? H - 1 : r), cc = c < 0 ? 0 : (c > W - 1 ? W - 1 : c);
            rowoff[i] = (unsigned)((n * H + rc) * W) * (unsigned)Cin;
            coloff[i] = (unsigned)cc * (unsigned)Cin + (unsigned)(cg * 2);
        }
        valid = 0u;
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                off[i * 4 + j] = (rowoff[i] + coloff[j]) * 4u;
                if (rv[i] && cv[j]) valid |= 1u << (i * 4 + j);
            }
    };
    float d[16][2];
    auto fetch_x = [&](int chunk) {
        const char* const base = reinterpret_cast<const char*>(x + chunk * KC);
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const float2 v = *reinterpret_cast<const float2*>(base + off[k]);
            d[k][0] = v.x; d[k][1] = v.y;
        }
    };
    auto transform_regs = [&]() {                      // d <- B^T d B, in place
        // (zero padding as 32 unconditional selects: a branch around them -- only the waves with a border tile need them --
        // splits the loop body, and the compiler's wait for the pixels at the loop head degrades to vmcnt(0), i.e. to a wait
        // for the filter reloads issued at the end of the period before)
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const bool ok = (valid >> k) & 1u;
            d[k][0] = ok ? d[k][0] : 0.0f; d[k][1] = ok ? d[k][1] : 0.0f;
        }
#pragma unroll
        for (int e = 0; e < 2; e++) {
            float s[16];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                s[0 * 4 + j] = d[0 * 4 + j][e] - d[2 * 4 + j][e];
                s[1 * 4 + j] = d[1 * 4 + j][e] + d[2 * 4 + j][e];
                s[2 * 4 + j] = d[2 * 4 + j][e] - d[1 * 4 + j][e];
                s[3 * 4 + j] = d[1 * 4 + j][e] - d[3 * 4 + j][e];
            }
#pragma unroll
            for (int i = 0; i < 4; i++) {
                d[i * 4 + 0][e] = s[i * 4 + 0] - s[i * 4 + 2];
                d[i * 4 + 1][e] = s[i * 4 + 1] + s[i * 4 + 2];
                d[i * 4 + 2][e] = s[i * 4 + 2] - s[i * 4 + 1];
                d[i * 4 + 3][e] = s[i * 4 + 1] - s[i * 4 + 3];
            }
        }
    };
    auto store_v = [&](int buf) {                      // the sixteen positions of this thread's two channels to stage `buf`
        float* const vb = lds + buf * kW8VBUF + (cg * 2) * P + tile_l;
#pragma unroll
        for (int pos = 0; pos < 16; pos++)
#pragma unroll
            for (int e = 0; e < 2; e++) vb[(pos * KC + e) * P] = d[pos][e];
    };

    wf32x4_t ub[S][NB];
    const wf32x4_t* const ubase = reinterpret_cast<const wf32x4_t*>(U) + (size_t)nb * nchunks * (16 * NB * KQ * 64) + lane;
    auto u_ptr = [&](int chunk, int st, int j) {
        return ubase + ((size_t)((chunk * 16 + wave * 2 + st / KQ) * NB + j) * KQ + st % KQ) * 64;
    };
    wf32x16_t acc[2][2][NB];
    auto zero_acc = [&]() {
#pragma unroll
        for (int pl = 0; pl < 2; pl++)
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < NB; j++)
#pragma unroll
                    for (int r = 0; r < 16; r++) acc[pl][i][j][r] = 0.0f;
    };
    zero_acc();

    const int a_lane = (lane >> 5) * P + (lane & 31) + (wave * 2 * KC) * P;
    auto mfma_phase = [&](int chunk, int nxt) {
        const float* const vb = lds + (chunk & 1) * kW8VBUF + a_lane;
#pragma unroll
        for (int st = 0; st < S; st++) {
            const int pl = st / KQ;
            const float* const vp = vb + (pl * KC + (st % KQ) * 8) * P;
#pragma unroll
            for (int m = 0; m < 4; m++) {
                const float a0 = vp[(2 * m) * P], a1 = vp[(2 * m) * P + 32];
#pragma unroll
                for (int j = 0; j < NB; j++) {
                    acc[pl][0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, ub[st][j][m], acc[pl][0][j], 0, 0, 0);
                    acc[pl][1][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, ub[st][j][m], acc[pl][1][j], 0, 0, 0);
                }
            }
#pragma unroll
            for (int j = 0; j < NB; j++) ub[st][j] = *u_ptr(nxt, st, j);
        }
    };
    // output transform of block `blk` (as in variant 2: two halves of 32 tiles through all of LDS)
    const int h = wave & 1;
    auto epilogue = [&](int blk) {
#pragma unroll
        for (int i = 0; i < 2; i++) {
            float* const sw = lds + wave * (2 * 32 * BN);
#pragma unroll
            for (int j = 0; j < NB; j++)
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int tile = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    const int col = j * 32 + (lane & 31);
                    const float ma = acc[0][i][j][r], mb = acc[1][i][j][r];
                    sw[tile * BN + col] = h == 0 ? ma + mb : ma;
                    sw[32 * BN + tile * BN + col] = h == 0 ? mb : -(ma + mb);
                }
            __syncthreads();
            {
                const int tile = tid >> 4, c4 = (tid & 15) * 4;
                const int tt = blk * 64 + i * 32 + tile;
                if (tt < T) {
                    const int ox = tt % TW, oy = (tt / TW) % TH, on = tt / (TW * TH);
                    wf32x4_t pq[4][2];
#pragma unroll
                    for (int xi = 0; xi < 4; xi++)
#pragma unroll
                        for (int jj = 0; jj < 2; jj++)
                            pq[xi][jj] = *reinterpret_cast<const wf32x4_t*>(lds + ((2 * xi) * 2 + jj) * (32 * BN) + tile * BN + c4) +
                                         *reinterpret_cast<const wf32x4_t*>(lds + ((2 * xi + 1) * 2 + jj) * (32 * BN) + tile * BN + c4);
                    wf32x4_t bv = {0.f, 0.f, 0.f, 0.f};
                    if (bias) bv = *reinterpret_cast<const wf32x4_t*>(bias + nb * BN + c4);
#pragma unroll
                    for (int a = 0; a < 2; a++) {
                        const int oh = 2 * oy + a;
                        if (oh >= H) continue;
#pragma unroll
                        for (int jj = 0; jj < 2; jj++) {
                            const int ow = 2 * ox + jj;
                            if (ow >= W) continue;
                            wf32x4_t v = a == 0 ? (pq[0][jj] + pq[1][jj]) + pq[2][jj] : (pq[1][jj] - pq[2][jj]) - pq[3][jj];
                            v += bv;
                            if (relu) {
#pragma unroll
                                for (int e = 0; e < 4; e++) v[e] = fmaxf(v[e], 0.0f);
                            }
                            *reinterpret_cast<wf32x4_t*>(y + ((size_t)(on * H + oh) * W + ow) * Cout + nb * BN + c4) = v;
                        }
                    }
                }
            }
            __syncthreads();
        }
    };

    set_block(tb);
    fetch_x(0);
    int prev = -1;
    while (true) {
        __builtin_amdgcn_sched_barrier(0);
        transform_regs();                              // (waits for the pixels only: they were fetched before the filter reloads)
        __builtin_amdgcn_sched_barrier(0);
        if (prev >= 0) { epilogue(prev); zero_acc(); }
        if (tb >= n_tb) break;
        store_v(0);
        __builtin_amdgcn_sched_barrier(0);
        // The output transform's stores must be out of the vmcnt queue before the chunk loops are entered: with loads AND
        // stores pending the compiler's waits cannot count (the two kinds return out of order) and every wait of the second
        // shift's loop becomes vmcnt(0).  They drained while the accumulators were zeroed and stage 0 was written.
        __builtin_amdgcn_s_waitcnt(0x0F70);            // vmcnt(0)
        __builtin_amdgcn_sched_barrier(0);
        // loads in the chunk loops' order: second shift pixels first, filter behind them
        if (shift_b) fetch_x(nchunks > 1 ? 1 : 0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int st = 0; st < S; st++)
#pragma unroll
            for (int j = 0; j < NB; j++) ub[st][j] = *u_ptr(0, st, j);
        __builtin_amdgcn_sched_barrier(0);
        const int nxt_tb = tb + G < n_tb ? tb + G : tb; // (no next block: its own pixels again, never used)
        __syncthreads();
        if (!shift_b) {                                // first shift: fetch, multiply, transform
            for (int chunk = 0; chunk < nchunks; chunk++) {
                const bool is_last = chunk == last;
                if (is_last) set_block(nxt_tb);
                fetch_x(is_last ? 0 : chunk + 1);
                __builtin_amdgcn_sched_barrier(0);
                mfma_phase(chunk, is_last ? 0 : chunk + 1);
                __builtin_amdgcn_sched_barrier(0);
                if (!is_last) { transform_regs(); store_v((chunk + 1) & 1); }
                __syncthreads();
            }
        } else {                                       // second shift: transform, fetch, multiply
            for (int chunk = 0; chunk < nchunks; chunk++) {
                const bool is_last = chunk == last;
                if (!is_last) { transform_regs(); store_v((chunk + 1) & 1); }
                __builtin_amdgcn_sched_barrier(0);
                if (is_last) set_block(nxt_tb);
                fetch_x(is_last ? 0 : (chunk + 2 < nchunks ? chunk + 2 : last));
                __builtin_amdgcn_sched_barrier(0);
                mfma_phase(chunk, is_last ? 0 : chunk + 1);
                __syncthreads();
            }
        }
        prev = tb;
        tb += G;
    }
}

// hipFuncSetAttribute holds per device: the 132 KB of dynamic LDS are allowed once per (kernel, device); `done` is the kernel's
// bit set of devices
static hipError_t allow_lds(const void* fn, int bytes, std::atomic<unsigned long long>& done) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const unsigned long long bit = dev >= 0 && dev < 64 ? 1ull << dev : 0ull;
    if (bit && (done.load(std::memory_order_relaxed) & bit)) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) done.fetch_or(bit, std::memory_order_relaxed);
    return e;
}

static hipError_t launch_wino_w8p(const float* x, const float* U, float* y, const float* bias, int N, int H, int W, int Cin,
                                  int Cout, int relu, hipStream_t st) {
    const int TH = (H + 1) / 2, TW = (W + 1) / 2, T = N * TH * TW;
    const int n_tb = (T + 63) / 64, n_nb = Cout / 64;
    static std::atomic<int> cus_of[64];                // compute units of each device, asked once
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    int cus = dev >= 0 && dev < 64 ? cus_of[dev].load(std::memory_order_relaxed) : 0;
    if (!cus) {
        int v = 0;
        cus = hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0 ? v : 256;
        if (dev >= 0 && dev < 64) cus_of[dev].store(cus, std::memory_order_relaxed);
    }
    int G = cus / n_nb;                                // workgroups per channel block: one workgroup per compute unit in all
    if (G < 1) G = 1;
    if (G > n_tb) G = n_tb;
    static std::atomic<unsigned long long> lds_set{0};
    e = allow_lds(reinterpret_cast<const void*>(&winograd_f23_w8p_kernel), kW8LdsBytes, lds_set);
    if (e != hipSuccess) return e;
    winograd_f23_w8p_kernel<<<(unsigned)(G * n_nb), 512, kW8LdsBytes, st>>>(x, U, y, bias, H, W, Cin, Cout, TH, TW, T, relu, n_tb, G);
    return hipGetLastError();
}

template <int DIAG>
static hipError_t launch_wino_w8(const float* x, const float* U, float* y, const float* bias, int N, int H, int W, int Cin,
                                 int Cout, int relu, int nb_major, hipStream_t st) {
    const int TH = (H + 1) / 2, TW = (W + 1) / 2, T = N * TH * TW;
    const long long blocks = (long long)((T + 63) / 64) * (Cout / 64);
    static std::atomic<unsigned long long> lds_set{0};
    hipError_t e = allow_lds(reinterpret_cast<const void*>(&winograd_f23_w8_kernel<DIAG>), kW8LdsBytes, lds_set);
    if (e != hipSuccess) return e;
    winograd_f23_w8_kernel<DIAG><<<(unsigned)blocks, 512, kW8LdsBytes, st>>>(x, U, y, bias, H, W, Cin, Cout, TH, TW, T, relu, nb_major);
    return hipGetLastError();
}

template <int DIAG>
static hipError_t launch_wino_w8x3(const float* x, const unsigned short* U3, float* y, const float* bias, int N, int H, int W,
                                   int Cin, int Cout, int relu, int nb_major, hipStream_t st) {
    const int TH = (H + 1) / 2, TW = (W + 1) / 2, T = N * TH * TW;
    const long long blocks = (long long)((T + 63) / 64) * (Cout / 64);
    static std::atomic<unsigned long long> lds_set{0};
    hipError_t e = allow_lds(reinterpret_cast<const void*>(&winograd_f23_w8x3_kernel<DIAG>), kW8LdsBytes, lds_set);
    if (e != hipSuccess) return e;
    winograd_f23_w8x3_kernel<DIAG><<<(unsigned)blocks, 512, kW8LdsBytes, st>>>(x, U3, y, bias, H, W, Cin, Cout, TH, TW, T, relu,
                                                                                nb_major);
    return hipGetLastError();
}

static hipError_t launch_wino_w8x3w(const float* x, const unsigned short* U3, float* y, const float* bias, int N, int H, int W,
                                    int Cin, int Cout, int relu, int nb_major, hipStream_t st) {
    const int TH = (H + 1) / 2, TW = (W + 1) / 2, T = N * TH * TW;
    const long long blocks = (long long)((T + 31) / 32) * (Cout / 128);
    static std::atomic<unsigned long long> lds_set{0};
    hipError_t e = allow_lds(reinterpret_cast<const void*>(&winograd_f23_w8x3w_kernel), kW8WLdsBytes, lds_set);
    if (e != hipSuccess) return e;
    winograd_f23_w8x3w_kernel<<<(unsigned)blocks, 512, kW8WLdsBytes, st>>>(x, U3, y, bias, H, W, Cin, Cout, TH, TW, T, relu, nb_major);
    return hipGetLastError();
}

// What the 128-channel kernel can run at all: its channel blocks, and an activation under the offsets that stand for the padding.
static bool wino_x3_wide_runs(int N, int H, int W, int Cin, int Cout) {
    return Cout % 128 == 0 && (double)N * H * W * Cin * 4.0 <= (double)kW8WMaxBytes;
}

// Whether variant 4 takes the 128-channel workgroups (T tiles): a rule on shapes, so that every run and every rank of a job
// take the same kernel -- although the two agree bit for bit.
//   * the launch must fill the chip as winograd.MIN_WORKGROUPS asks of the 64-channel one;
//   * the 128-channel block's split filter (16 * 128 * Cin * 6 bytes) is what the workgroups of an XCD read over and over.  The
//     plan was to ask that it fit the 4 MiB L2 beside the pixels (3.1 MB at 256 input channels); at 512 (6.3 MB) the wide
//     kernel measured 5 % faster all the same (profiles/wino_x3_wide/README.md), so the bound is the largest size MEASURED.
static bool wino_x3_wide_pays(int Cin, int Cout, int T) {
    const long long wide_blocks = (long long)((T + 31) / 32) * (Cout / 128);
    return Cout % 128 == 0 && Cin <= 512 && wide_blocks >= 256;
}

template <int KC, int NB, int WGS>
static hipError_t launch_wino(const float* x, const float* U, float* y, const float* bias, int N, int H, int W, int Cin,
                              int Cout, int relu, int nb_major, hipStream_t st) {
    using C = WinoCfg<KC, NB>;
    const int TH = (H + 1) / 2, TW = (W + 1) / 2, T = N * TH * TW;
    const long long blocks = (long long)((T + 63) / 64) * (Cout / C::BN);
    static std::atomic<unsigned long long> lds_set{0};
    hipError_t e = allow_lds(reinterpret_cast<const void*>(&winograd_f23_kernel<KC, NB, WGS>), C::LDS_BYTES, lds_set);
    if (e != hipSuccess) return e;
    winograd_f23_kernel<KC, NB, WGS><<<(unsigned)blocks, 256, C::LDS_BYTES, st>>>(x, U, y, bias, H, W, Cin, Cout, TH, TW, T,
                                                                                  relu, nb_major);
    return hipGetLastError();
}

// variant 0: 64 tiles x 64 channels, K-chunks of 16, one workgroup per compute unit (256 accumulator registers per lane);
// variant 1: 64 tiles x 32 channels, K-chunks of 8, two workgroups per compute unit;
// variant 2: variant 0's tile and filter layout, eight waves in two shifts;
// variant 3: variant 2 as persistent workgroups.  The filter layout depends on the variant (0, 2, 3 share one).
// Any other variant (variant 4 included: its filter is not float32) is refused.
hipError_t launch_winograd_f23(const float* x, const float* U, float* y, const float* bias, int N, int H, int W, int Cin,
                               int Cout, int relu, int variant, int nb_major, hipStream_t st) {
    if (variant == 0) return launch_wino<16, 2, 1>(x, U, y, bias, N, H, W, Cin, Cout, relu, nb_major, st);
    if (variant == 1) return launch_wino<8, 1, 2>(x, U, y, bias, N, H, W, Cin, Cout, relu, nb_major, st);
    if (variant == 2) return launch_wino_w8<0>(x, U, y, bias, N, H, W, Cin, Cout, relu, nb_major, st);
    if (variant == 3) return launch_wino_w8p(x, U, y, bias, N, H, W, Cin, Cout, relu, st);
#ifdef OPA_WINO_DIAG          // timing experiments (wrong results): without the filter reloads / pixel fetches / transforms
    if (variant == 11) return launch_wino_w8<1>(x, U, y, bias, N, H, W, Cin, Cout, relu, nb_major, st);
    if (variant == 12) return launch_wino_w8<2>(x, U, y, bias, N, H, W, Cin, Cout, relu, nb_major, st);
    if (variant == 13) return launch_wino_w8<3>(x, U, y, bias, N, H, W, Cin, Cout, relu, nb_major, st);
    if (variant == 14) return launch_wino_w8<4>(x, U, y, bias, N, H, W, Cin, Cout, relu, nb_major, st);
    if (variant == 15) return launch_wino_w8<5>(x, U, y, bias, N, H, W, Cin, Cout, relu, nb_major, st);
    if (variant == 16) return launch_wino_w8<6>(x, U, y, bias, N, H, W, Cin, Cout, relu, nb_major, st);
    if (variant == 17) return launch_wino_w8<7>(x, U, y, bias, N, H, W, Cin, Cout, relu, nb_major, st);
    if (variant == 18) return launch_wino_w8<8>(x, U, y, bias, N, H, W, Cin, Cout, relu, nb_major, st);
#endif
    return hipErrorInvalidValue;
}

// variant 4: variant 2 on the bf16 MFMA pipe, U3 = the three bf16 planes of the filter (openpifpaf_amd.winograd.split_filter).
// It runs on 64-channel or on 128-channel workgroups (the same bits): by wino_x3_wide_pays, or as OPA_WINO_X3_BN = 64 | 128 says
// -- read on every launch, A/B runs and the tests switch inside one process; it never overrides what wino_x3_wide_runs asks.
// variant 5: the 128-channel workgroups or nothing.
// Any other variant is refused (21-23: variant 4's timing experiments, OPA_WINO_DIAG builds only).
hipError_t launch_winograd_f23x3(const float* x, const unsigned short* U3, float* y, const float* bias, int N, int H, int W,
                                 int Cin, int Cout, int relu, int variant, int nb_major, hipStream_t st) {
    if (variant == 5)
        return wino_x3_wide_runs(N, H, W, Cin, Cout) ? launch_wino_w8x3w(x, U3, y, bias, N, H, W, Cin, Cout, relu, nb_major, st)
                                                     : hipErrorInvalidValue;
    if (variant == 4) {
        if (wino_x3_wide_runs(N, H, W, Cin, Cout)) {
            const char* env = std::getenv("OPA_WINO_X3_BN");
            const int forced = env && *env ? std::atoi(env) : 0;
            if (forced == 128 || (forced != 64 && wino_x3_wide_pays(Cin, Cout, N * ((H + 1) / 2) * ((W + 1) / 2))))
                return launch_wino_w8x3w(x, U3, y, bias, N, H, W, Cin, Cout, relu, nb_major, st);
        }
        return launch_wino_w8x3<0>(x, U3, y, bias, N, H, W, Cin, Cout, relu, nb_major, st);
    }
#ifdef OPA_WINO_DIAG
    if (variant == 21) return launch_wino_w8x3<1>(x, U3, y, bias, N, H, W, Cin, Cout, relu, nb_major, st);
    if (variant == 22) return launch_wino_w8x3<2>(x, U3, y, bias, N, H, W, Cin, Cout, relu, nb_major, st);
    if (variant == 23) return launch_wino_w8x3<3>(x, U3, y, bias, N, H, W, Cin, Cout, relu, nb_major, st);
#endif
    return hipErrorInvalidValue;
}

}  // namespace opa
