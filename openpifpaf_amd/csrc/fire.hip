// Both expand convolutions of a SqueezeNet Fire module (reference network/basenetworks.py:461-487: torchvision's Fire), their
// biases, their ReLUs and the concatenation, in one launch:
//     out[b, y, x, n]      = relu(b1[n] + sum_c       h[b, y, x, c]           * W1[n, c])          n < E1
//     out[b, y, x, E1 + n] = relu(b3[n] + sum_ky,kx,c h[b, y+ky-1, x+kx-1, c] * W3[n, c, ky, kx])  n < E3   (outside the image: 0)
// h [B, H, W, S] channels-last float32 (the squeezed activation, S = 16 / 32 / 48 / 64), out [B, H, W, E1 + E3] channels-last
// float32.  The arithmetic is the split-operand scheme of gemm_f32x3.hip: every float32 operand as the exact sum of three bfloat16
// pieces (split_bf16.hpp), the partial products on v_mfma_f32_32x32x16_bf16 with float32 accumulators, the leading products a1*b1
// and the corrections in accumulators of their own, TERMS = 9 (all products) or 6 (without a2*b3, a3*b2, a3*b3).
//
// Why a kernel of its own: gemm_f32x3.hip's implicit GEMM (SRC = 2) fetches and splits every activation element once per tap and
// N tile and needs C % 64 == 0.  Here S <= 64, so a workgroup keeps the whole halo of its pixel tile in LDS:
//   * a 256-thread workgroup owns 8 x 16 output pixels (M = 128).  It loads the 10 x 18 x S halo once (zeros where it leaves the
//     image), splits each element ONCE and stores the three bf16 planes ([3][180 pixels][S]; 69 120 B at S = 64; the 16-byte
//     chunks of a pixel XOR-swizzled for S = 32 and 64 so that the fragment reads of 16 neighbouring pixels fall on 16 different
//     bank groups).  A tap of the 3x3 window is a shift of the pixel index in that tile: no im2col.
//   * S % 16 == 0 is the MFMA's K: a tap is S / 16 K-steps, there are no padded K columns.
//   * then it walks N tiles of 64 channels (4 waves as 2(M) x 2(N), a wave 64 pixels x 32 channels).  E1 % 64 == 0, so a tile lies
//     in one half: a tile of the 1x1 half walks the centre tap only (K = S), a tile of the 3x3 half the nine taps (K = 9 S).
//     Where the launch has few pixel tiles (a batch of one at 41 x 41) grid.y spreads the N tiles over workgroups instead.
//   * the weights are split and put into FRAGMENT order on the host, once (openpifpaf_amd.fused.fire_weight_of): one block
//     [3 planes][fragment][64 lanes][8 bf16], the fragment of (32-channel block, tap, K-step) being what the MFMA's B operand
//     holds, so a wave's load is 1 KB of consecutive bytes straight into registers -- no LDS stage, no barrier in the K loop.  The
//     block is at most 0.9 MB and stays in L2.  The fragments of the NEXT tap travel while this tap's MFMAs run.  (The issue
//     asked for "[3][...]": the planes are outermost; what follows is fragment order rather than [N][K], which would make
//     every lane's 16 bytes a row of its own.)
//   * epilogue: accumulators + bias through a wave-private 16 x 32 float patch in LDS (the MFMA's C layout has a lane per
//     channel; the store wants a lane per 16-byte vector), ReLU, 16-byte stores, eight lanes per pixel = 128 consecutive bytes.
//     The patch is 9 KB for the four waves: 78 336 B at S = 64, two workgroups per compute unit.
// NOT MEASURED, for the timing run (tools/gpu/squeezenet_times.py) to look at: the threshold of 512 pixel tiles between walking every
// N tile and spreading them over grid.y, and the cap of 64 on grid.y, are guesses (two workgroups on each of 256 compute units);
// both waves of a workgroup that share an N block (wm = 0, 1) fetch the same 3 KB of weight fragments per tap and K-step from L2
// -- at S = 16 on the 161 x 161 layers about twice the bytes the workgroup stores -- where one LDS stage could serve both.
// More than 64 KB of LDS needs hipFuncAttributeMaxDynamicSharedMemorySize, set on EVERY launch (no process-wide flag that a
// second device or a reloaded module would find stale).  Offsets into h and out are unsigned 32-bit BYTE counts: the entry point
// refuses tensors of 2 GB and more.
//
// Non-finite values follow the split kernels' rule (split_bf16.hpp: +-Inf splits into (+-Inf, NaN, NaN), NaN into NaNs): a NaN or
// +-Inf at pixel p of h makes NaN in every E1 channel at p and in every E3 channel at the pixels whose 3x3 window holds p; every
// other output is bit for bit what it is without that value (an MFMA row takes nothing from another row).  ReLU is written as
// v < 0 ? 0 : v, which keeps a NaN (fmaxf would return the zero).
#include "common.hpp"
#include "split_bf16.hpp"

namespace opa {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;

constexpr int kFireTH = 8, kFireTW = 16;                               // output pixels of a workgroup: 8 rows of 16
constexpr int kFireHW = kFireTW + 2, kFireHalo = (kFireTH + 2) * kFireHW;          // halo: 10 rows of 18 = 180 pixels
constexpr int kFirePatchPitch = 36;                                    // floats between rows of the epilogue patch (16-B aligned rows)
constexpr int kFirePatchBytes = 4 * 16 * kFirePatchPitch * 4;          // four waves, 16 rows each

// bf16 offset inside one plane of channel k (a multiple of 4) of halo pixel p: rows of S bf16, the 16-byte chunks of a row
// XOR-swizzled where the row is a power of two of them (S = 64: 8 chunks, S = 32: 4)
template <int S16>
__device__ __forceinline__ int fire_lds(int p, int k) {
    int c = k >> 3;
    if (S16 == 4) c ^= (p >> 1) & 7;
    else if (S16 == 2) c ^= (p >> 2) & 3;
    return p * (S16 * 16) + (c << 3) + (k & 7);
}

static size_t fire_lds_bytes(int S) { return (size_t)3 * kFireHalo * S * 2 + kFirePatchBytes; }

template <int S16, int TERMS>
__global__ __launch_bounds__(256, 2) void fire_expand_kernel(const float* __restrict__ h, const unsigned short* __restrict__ W3,
                                                             const float* __restrict__ bias, float* __restrict__ out,
                                                             int H, int W, int E1, int E3, int tiles_x, int tiles_y) {
    constexpr int S = S16 * 16;
    constexpr int PLANE = kFireHalo * S;                               // bf16 elements of one activation plane
    extern __shared__ __attribute__((aligned(16))) unsigned char fire_smem[];
    unsigned short* sA = reinterpret_cast<unsigned short*>(fire_smem);                  // [3][180][S]
    float* patches = reinterpret_cast<float*>(fire_smem + (size_t)3 * PLANE * 2);       // [4][16][36]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const unsigned tile = blockIdx.x;
    const int tx = (int)(tile % (unsigned)tiles_x), tq = (int)(tile / (unsigned)tiles_x);
    const int ty = tq % tiles_y, b = tq / tiles_y;
    const int y0 = ty * kFireTH, x0 = tx * kFireTW;

    // ---- the halo: global -> split -> LDS, every element once ----
    constexpr int VP = S / 4;                                          // 16-byte vectors of a pixel
    constexpr int NV = kFireHalo * VP;
    constexpr int UN = 4;                                              // loads in flight per thread before the first split
    for (int v0 = tid; v0 < NV; v0 += 256 * UN) {
        f32x4_t a[UN];
#pragma unroll
        for (int u = 0; u < UN; u++) {
            const int v = v0 + u * 256;
            const int p = v / VP, k = (v - p * VP) * 4;
            const int hy = p / kFireHW, hx = p - hy * kFireHW;
            const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;
            a[u] = (f32x4_t){0.0f, 0.0f, 0.0f, 0.0f};
            if (v < NV && iy >= 0 && iy < H && ix >= 0 && ix < W) {
                const unsigned off = ((((unsigned)b * (unsigned)H + (unsigned)iy) * (unsigned)W + (unsigned)ix) * (unsigned)S + (unsigned)k) * 4u;
                a[u] = *reinterpret_cast<const f32x4_t*>(reinterpret_cast<const char*>(h) + off);
            }
        }
#pragma unroll
        for (int u = 0; u < UN; u++) {
            const int v = v0 + u * 256;
            if (v >= NV) break;
            const int p = v / VP, k = (v - p * VP) * 4;
            u32x2_t p1, p2, p3;
            split4(a[u], p1, p2, p3);
            unsigned short* d = sA + fire_lds<S16>(p, k);
            *reinterpret_cast<u32x2_t*>(d) = p1;
            *reinterpret_cast<u32x2_t*>(d + PLANE) = p2;
            *reinterpret_cast<u32x2_t*>(d + 2 * PLANE) = p3;
        }
    }
    __syncthreads();

    // the wave's two 32-pixel blocks: row (lane & 31) of block i is tile pixel m = wm * 64 + i * 32 + (lane & 31); its window's
    // first tap is halo pixel (m / 16) * 18 + m % 16
    int pbase[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int m = wm * 64 + i * 32 + (lane & 31);
        pbase[i] = (m >> 4) * kFireHW + (m & 15);
    }
    const int kof = (lane >> 5) * 8;                                   // the lane's eight K columns of a K-step
    const int N = E1 + E3, n_tiles = N / 64;
    const size_t w_plane = ((size_t)E1 + (size_t)9 * E3) * S;          // bf16 elements of one weight plane
    float* patch = patches + wave * (16 * kFirePatchPitch);

    for (int nt = blockIdx.y; nt < n_tiles; nt += gridDim.y) {
        const int n0 = nt * 64;
        const int nb = nt * 2 + wn;                                    // the wave's 32-channel block of the concatenation
        const bool one = n0 < E1;                                      // (uniform) a tile of the 1x1 half
        const int t0 = one ? 4 : 0, t1 = one ? 5 : 9;
        // first fragment of the block: the 1x1 half holds S16 fragments per block, the 3x3 half 9 * S16 (tap-major)
        const size_t f0 = one ? (size_t)nb * S16 : (size_t)(E1 / 32) * S16 + (size_t)(nb - E1 / 32) * 9 * S16;
        const unsigned short* wb = W3 + f0 * 512 + lane * 8;

        f32x16_t acc[2], low[2];
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int r = 0; r < 16; r++) { acc[i][r] = 0.0f; low[i][r] = 0.0f; }

        u32x4_t fb0[S16][3], fb1[S16][3];
        auto fetch = [&](u32x4_t (&fb)[S16][3], int t) {              // the fragments of tap t (index from t0)
            const unsigned short* src = wb + (size_t)(t - t0) * S16 * 512;
#pragma unroll
            for (int ks = 0; ks < S16; ks++)
#pragma unroll
                for (int pl = 0; pl < 3; pl++)
                    fb[ks][pl] = *reinterpret_cast<const u32x4_t*>(src + (size_t)pl * w_plane + ks * 512);
        };
        auto tap = [&](int t, const u32x4_t (&cur)[S16][3], u32x4_t (&nxt)[S16][3]) {
            fetch(nxt, t + 1 < t1 ? t + 1 : t);                        // (no branch around the loads: the last tap is asked for again)
            const int shift = (t / 3) * kFireHW + t % 3;
#pragma unroll
            for (int ks = 0; ks < S16; ks++) {
                bf16x8_t fa[3][2], fw[3];
#pragma unroll
                for (int pl = 0; pl < 3; pl++) {
                    fw[pl] = __builtin_bit_cast(bf16x8_t, cur[ks][pl]);
#pragma unroll
                    for (int i = 0; i < 2; i++)
                        fa[pl][i] = *reinterpret_cast<const bf16x8_t*>(sA + pl * PLANE + fire_lds<S16>(pbase[i] + shift, ks * 16 + kof));
                }
#pragma unroll
                for (int i = 0; i < 2; i++) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0][i], fw[0], acc[i], 0, 0, 0);
                // the corrections, smallest first
#pragma unroll
                for (int s = 4; s >= 1; s--) {
                    if (TERMS == 6 && s > 2) continue;
#pragma unroll
                    for (int pa = 0; pa < 3; pa++) {
                        const int pb = s - pa;
                        if (pb < 0 || pb > 2) continue;
#pragma unroll
                        for (int i = 0; i < 2; i++) low[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[pa][i], fw[pb], low[i], 0, 0, 0);
                    }
                }
            }
        };
        fetch(fb0, t0);
        for (int t = t0;;) {
            tap(t, fb0, fb1);
            if (++t == t1) break;
            tap(t, fb1, fb0);
            if (++t == t1) break;
        }

        // ---- epilogue: 16 pixels (one tile row) x 32 channels at a time through the wave's patch ----
        const float bn = bias[n0 + wn * 32 + (lane & 31)];
#pragma unroll
        for (int i = 0; i < 2; i++) {
#pragma unroll
            for (int half = 0; half < 2; half++) {
#pragma unroll
                for (int g = 0; g < 2; g++)
#pragma unroll
                    for (int q = 0; q < 4; q++) {                      // C layout: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
                        const int r = (half * 2 + g) * 4 + q;
                        patch[(q + 8 * g + 4 * (lane >> 5)) * kFirePatchPitch + (lane & 31)] = (acc[i][r] + low[i][r]) + bn;
                    }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                const int y = y0 + wm * 4 + i * 2 + half;              // the tile row of these 16 pixels
#pragma unroll
                for (int pass = 0; pass < 2; pass++) {
                    const int v = pass * 64 + lane, row = v >> 3, c4 = (v & 7) * 4;
                    const int x = x0 + row;
                    if (y < H && x < W) {
                        f32x4_t f = *reinterpret_cast<const f32x4_t*>(patch + row * kFirePatchPitch + c4);
#pragma unroll
                        for (int e = 0; e < 4; e++) f[e] = f[e] < 0.0f ? 0.0f : f[e];          // (keeps a NaN)
                        const unsigned off = ((((unsigned)b * (unsigned)H + (unsigned)y) * (unsigned)W + (unsigned)x) * (unsigned)N
                                              + (unsigned)(n0 + wn * 32 + c4)) * 4u;
                        *reinterpret_cast<f32x4_t*>(reinterpret_cast<char*>(out) + off) = f;
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
}

long long fire_expand_workgroups(int B, int H, int W) {
    return (long long)B * ((H + kFireTH - 1) / kFireTH) * ((W + kFireTW - 1) / kFireTW);
}

template <int S16, int TERMS>
static hipError_t launch_fire_st(const float* h, const unsigned short* w3, const float* bias, float* out, int B, int H, int W,
                                 int E1, int E3, hipStream_t st) {
    const int tiles_x = (W + kFireTW - 1) / kFireTW, tiles_y = (H + kFireTH - 1) / kFireTH;
    const long long tiles = fire_expand_workgroups(B, H, W);
    const int n_tiles = (E1 + E3) / 64;
    // enough pixel tiles to fill the device: a workgroup walks every N tile of its pixels (the halo is loaded and split once);
    // fewer: the N tiles are spread over grid.y (at most 64 of them)
    const int split = tiles >= 512 ? 1 : (n_tiles < 64 ? n_tiles : 64);
    const size_t lds = fire_lds_bytes(S16 * 16);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&fire_expand_kernel<S16, TERMS>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    fire_expand_kernel<S16, TERMS><<<dim3((unsigned)tiles, (unsigned)split), 256, lds, st>>>(h, w3, bias, out, H, W, E1, E3, tiles_x, tiles_y);
    return hipGetLastError();
}

template <int TERMS>
static hipError_t launch_fire_terms(const float* h, const unsigned short* w3, const float* bias, float* out, int B, int H, int W, int S,
                                    int E1, int E3, hipStream_t st) {
    switch (S) {
        case 16: return launch_fire_st<1, TERMS>(h, w3, bias, out, B, H, W, E1, E3, st);
        case 32: return launch_fire_st<2, TERMS>(h, w3, bias, out, B, H, W, E1, E3, st);
        case 48: return launch_fire_st<3, TERMS>(h, w3, bias, out, B, H, W, E1, E3, st);
        case 64: return launch_fire_st<4, TERMS>(h, w3, bias, out, B, H, W, E1, E3, st);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_fire_expand(const float* h, const unsigned short* w3, const float* bias, float* out, int B, int H, int W, int S,
                              int E1, int E3, int terms, hipStream_t st) {
    if (E1 <= 0 || E3 <= 0 || E1 % 64 != 0 || E3 % 64 != 0) return hipErrorInvalidValue;
    if (terms == 6) return launch_fire_terms<6>(h, w3, bias, out, B, H, W, S, E1, E3, st);
    return launch_fire_terms<9>(h, w3, bias, out, B, H, W, S, E1, E3, st);
}

}  // namespace opa
