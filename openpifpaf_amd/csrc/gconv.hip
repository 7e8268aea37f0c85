// Grouped 3x3 convolution (padding 1, stride 1 or 2, as many output as input channels) on gfx950: the middle convolution of a
// ResNeXt bottleneck (reference network/basenetworks.py:71-150 with torchvision's grouped Bottleneck: 32 groups of 4 ... 64
// channels), float32, channels innermost, the folded batch-norm bias and optionally ReLU applied before the single store.
//
//   out[b, y, x, co] = act(bias[co] + sum_{t, ci} x[b, y*s - 1 + ky, x*s - 1 + kx, (co / CG) * CG + ci] * wt[t][ci][co]),  t = ky*3 + kx
//
// wt is tap-major with the output channel innermost, [9][CG][C]: the lanes of a wave read consecutive output channels.
//
// A workgroup of 256 threads computes a tile of TH x TW output pixels of one image for a chunk of 64 channels (a whole number of
// groups for every CG).  Thread = 4 consecutive output channels (never across a group: CG % 4 == 0) x P consecutive output pixels
// of one row: 16 channel quads x 16 pixel slots, the slots laid out SX along x and TH = 16 / SX along y, TW = SX * P.  The tile's
// input window -- ((TH - 1) * S + 3) x ((TW - 1) * S + 3) pixels x 64 channels -- is brought into the LDS once with 16-byte loads
// (a pixel's 64 channels are 256 consecutive bytes), zeros where the window leaves the image or the chunk leaves the tensor, so
// the inner loop tests no bounds.  There a thread reads 4 input channels of its group as one 16-byte LDS read (the lanes of a
// group read the same address: a broadcast; lanes of different groups and of different slots fall on different banks) and 4
// weight vectors from global memory (L2-resident: the whole operand is 18 KB ... 4.7 MB), 16 * P multiply-adds for every such set.
// SX is chosen on the host from the shape alone (pick_tile): the split that stages the fewest input pixels.
//
// Summation: explicit fmaf (the library is built with -ffp-contract=off), input channels in ascending order inside a partial sum
// per tap (CG >= 16: chains of CG terms) or per kernel row (CG 4, 8: chains of 3 * CG terms), the partial sums added in tap order,
// the bias last.  The order depends on nothing but CG: equal inputs give equal bits, whatever the tile.
// Every offset into x and out is 64-bit.
#include "common.hpp"
#include <atomic>

namespace opa {

constexpr int kGconvChunk = 64;                 // channels of a workgroup
constexpr int kGconvQuads = kGconvChunk / 4;    // channel quads = threads along the channels
constexpr int kGconvSlots = 256 / kGconvQuads;  // pixel slots of a workgroup
constexpr int kGconvMaxLds = 80 * 1024;         // two workgroups per compute unit

template <int CG, int S, int P>
__global__ __launch_bounds__(256) void gconv3x3_kernel(const float* __restrict__ x, long long xs, const float* __restrict__ wt,
                                                       const float* __restrict__ bias, float* __restrict__ out, long long os,
                                                       int H, int W, int C, int Ho, int Wo, int sxl, int tiles_x, int chunks,
                                                       int relu) {
    extern __shared__ float4 gconv_tile[];      // [IR][IC][16 channel quads]
    const int SX = 1 << sxl, TH = kGconvSlots >> sxl, TW = SX * P;
    const int IR = (TH - 1) * S + 3, IC = (TW - 1) * S + 3;
    const int tid = threadIdx.x;
    const int chunk = blockIdx.x % chunks, t = blockIdx.x / chunks;
    const int tx = t % tiles_x, ty = t / tiles_x, b = blockIdx.y;
    const int c0 = chunk * kGconvChunk;
    const int nq = min(kGconvQuads, (C - c0) / 4);              // channel quads of this chunk that exist
    const int y0 = ty * TH, x0 = tx * TW;

    {   // the input window: 16 lanes per pixel, 16 pixels per pass
        const int q = tid & (kGconvQuads - 1);
        const int iy0 = y0 * S - 1, ix0 = x0 * S - 1;
        const float* xb = x + (size_t)b * H * W * xs + c0 + q * 4;
        int r = 0, col = tid >> 4;
        while (col >= IC) { col -= IC; r++; }
        for (int p = tid >> 4; p < IR * IC; p += kGconvSlots) {
            const int yy = iy0 + r, xx = ix0 + col;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (q < nq && yy >= 0 && yy < H && xx >= 0 && xx < W)
                v = *reinterpret_cast<const float4*>(xb + ((size_t)yy * W + xx) * xs);
            gconv_tile[p * kGconvQuads + q] = v;
            col += kGconvSlots;
            while (col >= IC) { col -= IC; r++; }
        }
    }
    __syncthreads();

    const int cq = tid & (kGconvQuads - 1), slot = tid >> 4;
    const int sxi = slot & (SX - 1), ry = slot >> sxl;
    const int yo = y0 + ry, xo0 = x0 + sxi * P;
    if (cq >= nq || yo >= Ho || xo0 >= Wo) return;              // (behind the only barrier)
    const int co = c0 + cq * 4;
    const int gq = (cq * 4 / CG) * (CG / 4);                    // the group's first channel quad inside the chunk
    constexpr bool kPerTap = CG >= 16;
    constexpr int kUnroll = CG / 4 <= 4 ? CG / 4 : 2;           // of the loop over the group's channel quads

    float acc[P][4];
#pragma unroll
    for (int p = 0; p < P; p++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[p][j] = 0.0f;

#pragma unroll 1
    for (int ky = 0; ky < 3; ky++) {
        float part[P][4];
#pragma unroll
        for (int p = 0; p < P; p++)
#pragma unroll
            for (int j = 0; j < 4; j++) part[p][j] = 0.0f;
#pragma unroll 1
        for (int kx = 0; kx < 3; kx++) {
            const float4* trow = gconv_tile + ((size_t)((ry * S + ky) * IC + sxi * P * S + kx) * kGconvQuads + gq);
            const float* wrow = wt + (size_t)((ky * 3 + kx) * CG) * C + co;
#pragma unroll kUnroll
            for (int c4 = 0; c4 < CG / 4; c4++) {
                const float4 w0 = *reinterpret_cast<const float4*>(wrow + (size_t)(c4 * 4 + 0) * C);
                const float4 w1 = *reinterpret_cast<const float4*>(wrow + (size_t)(c4 * 4 + 1) * C);
                const float4 w2 = *reinterpret_cast<const float4*>(wrow + (size_t)(c4 * 4 + 2) * C);
                const float4 w3 = *reinterpret_cast<const float4*>(wrow + (size_t)(c4 * 4 + 3) * C);
#pragma unroll
                for (int p = 0; p < P; p++) {
                    const float4 xv = trow[p * S * kGconvQuads + c4];
                    part[p][0] = fmaf(xv.x, w0.x, part[p][0]); part[p][1] = fmaf(xv.x, w0.y, part[p][1]);
                    part[p][2] = fmaf(xv.x, w0.z, part[p][2]); part[p][3] = fmaf(xv.x, w0.w, part[p][3]);
                    part[p][0] = fmaf(xv.y, w1.x, part[p][0]); part[p][1] = fmaf(xv.y, w1.y, part[p][1]);
                    part[p][2] = fmaf(xv.y, w1.z, part[p][2]); part[p][3] = fmaf(xv.y, w1.w, part[p][3]);
                    part[p][0] = fmaf(xv.z, w2.x, part[p][0]); part[p][1] = fmaf(xv.z, w2.y, part[p][1]);
                    part[p][2] = fmaf(xv.z, w2.z, part[p][2]); part[p][3] = fmaf(xv.z, w2.w, part[p][3]);
                    part[p][0] = fmaf(xv.w, w3.x, part[p][0]); part[p][1] = fmaf(xv.w, w3.y, part[p][1]);
                    part[p][2] = fmaf(xv.w, w3.z, part[p][2]); part[p][3] = fmaf(xv.w, w3.w, part[p][3]);
                }
            }
            if (kPerTap) {
#pragma unroll
                for (int p = 0; p < P; p++)
#pragma unroll
                    for (int j = 0; j < 4; j++) { acc[p][j] += part[p][j]; part[p][j] = 0.0f; }
            }
        }
        if (!kPerTap) {
#pragma unroll
            for (int p = 0; p < P; p++)
#pragma unroll
                for (int j = 0; j < 4; j++) acc[p][j] += part[p][j];
        }
    }

    float4 bv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (bias) bv = *reinterpret_cast<const float4*>(bias + co);
    float* orow = out + (((size_t)b * Ho + yo) * Wo + xo0) * os + co;
#pragma unroll
    for (int p = 0; p < P; p++) {
        if (xo0 + p >= Wo) break;
        float4 o = make_float4(acc[p][0] + bv.x, acc[p][1] + bv.y, acc[p][2] + bv.z, acc[p][3] + bv.w);
        if (relu) o = make_float4(fmaxf(o.x, 0.0f), fmaxf(o.y, 0.0f), fmaxf(o.z, 0.0f), fmaxf(o.w, 0.0f));
        *reinterpret_cast<float4*>(orow + (size_t)p * os) = o;
    }
}

// output pixels of a thread: 8 at stride 1; 4 at stride 2, where the same outputs need four times the window
static constexpr int gconv_pixels(int S) { return S == 1 ? 8 : 4; }

// log2(SX): of the splits of the 16 pixel slots whose window fits kGconvMaxLds, the one that stages the fewest input pixels over
// the whole image (ties: the wider tile).  A function of (Ho, Wo, S) alone.
static int pick_tile(int Ho, int Wo, int S) {
    const int P = gconv_pixels(S);
    int best = 0;
    long long best_cost = -1;
    for (int l = 0; l <= 4; l++) {
        const int SX = 1 << l, TH = kGconvSlots >> l, TW = SX * P;
        const long long IR = (TH - 1) * S + 3, IC = (TW - 1) * S + 3;
        if (IR * IC * kGconvQuads * 16 > kGconvMaxLds) continue;
        const long long cost = (long long)((Ho + TH - 1) / TH) * ((Wo + TW - 1) / TW) * IR * IC;
        if (best_cost < 0 || cost <= best_cost) { best = l; best_cost = cost; }
    }
    return best;
}

long long gconv3x3_workgroups(int H, int W, int C, int S) {
    const int Ho = (H - 1) / S + 1, Wo = (W - 1) / S + 1, l = pick_tile(Ho, Wo, S);
    const int TH = kGconvSlots >> l, TW = (1 << l) * gconv_pixels(S);
    return (long long)((Ho + TH - 1) / TH) * ((Wo + TW - 1) / TW) * ((C + kGconvChunk - 1) / kGconvChunk);
}

// hipFuncSetAttribute holds per device: more than 64 KB of dynamic LDS are allowed once per (kernel, device)
static hipError_t allow_lds(const void* fn, std::atomic<unsigned long long>& done) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const unsigned long long bit = dev >= 0 && dev < 64 ? 1ull << dev : 0ull;
    if (bit && (done.load(std::memory_order_relaxed) & bit)) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kGconvMaxLds);
    if (e == hipSuccess) done.fetch_or(bit, std::memory_order_relaxed);
    return e;
}

template <int CG, int S>
static hipError_t launch_gconv_t(const float* x, long long xs, const float* wt, const float* bias, float* out, long long os,
                                 int B, int H, int W, int C, int relu, hipStream_t st) {
    constexpr int P = gconv_pixels(S);
    static std::atomic<unsigned long long> done{0};
    hipError_t e = allow_lds((const void*)gconv3x3_kernel<CG, S, P>, done);
    if (e != hipSuccess) return e;
    const int Ho = (H - 1) / S + 1, Wo = (W - 1) / S + 1, l = pick_tile(Ho, Wo, S);
    const int TH = kGconvSlots >> l, TW = (1 << l) * P;
    const int IR = (TH - 1) * S + 3, IC = (TW - 1) * S + 3;
    const int tiles_x = (Wo + TW - 1) / TW, tiles_y = (Ho + TH - 1) / TH, chunks = (C + kGconvChunk - 1) / kGconvChunk;
    const size_t lds = (size_t)IR * IC * kGconvQuads * sizeof(float4);
    dim3 grid((unsigned)((long long)tiles_x * tiles_y * chunks), (unsigned)B);
    gconv3x3_kernel<CG, S, P><<<grid, 256, lds, st>>>(x, xs, wt, bias, out, os, H, W, C, Ho, Wo, l, tiles_x, chunks, relu);
    prof_mark(st, "gconv3x3_kernel");
    return hipGetLastError();
}

hipError_t launch_gconv3x3(const float* x, long long xs, const float* wt, const float* bias, float* out, long long os,
                           int B, int H, int W, int C, int CG, int S, int relu, hipStream_t st) {
#define OPA_GCONV(G) \
    if (CG == G) return S == 1 ? launch_gconv_t<G, 1>(x, xs, wt, bias, out, os, B, H, W, C, relu, st) \
                               : launch_gconv_t<G, 2>(x, xs, wt, bias, out, os, B, H, W, C, relu, st)
    if (S != 1 && S != 2) return hipErrorInvalidValue;
    OPA_GCONV(4); OPA_GCONV(8); OPA_GCONV(16); OPA_GCONV(32); OPA_GCONV(64);
#undef OPA_GCONV
    return hipErrorInvalidValue;
}

}  // namespace opa
