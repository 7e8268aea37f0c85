// The RGB stem of every non-ResNet backbone (reference network/basenetworks.py: ShuffleNetV2K's input_block :271-355, torchvision's
// ShuffleNetV2 conv1 :36-69, MobileNetV2 / V3 features[0] :407-446, SqueezeNet features[0] :461-487): a direct 3x3 convolution from 3
// input channels, padding 1, dilation 1, stride S (1: MobileNetV3, 2: the others), float32 in and out, with the folded bias and the
// activation applied before the single store:
//     out[b, oy, ox, co] = act(sum_t x[b, ci, oy*S - 1 + ky, ox*S - 1 + kx] * w[t][co] + bias[co]),   t = (ky * 3 + kx) * 3 + ci
// Input.   [B, 3, H, W] given by four element strides (batch, channel, row, pixel): NCHW-contiguous, channels-last (3 floats per
//          pixel) and a cropped view of either are read where they lie, nothing is copied.  Any 4-byte alignment.
// Output.  Dense channels-last [B, Ho, Wo, C], Ho = (H - 1) / S + 1, Wo = (W - 1) / S + 1.
// Weights. w [27][C], TAP-MAJOR: row t = (ky * 3 + kx) * 3 + ci holds weight[co][ci][ky][kx] for co = 0 .. C - 1
//          (openpifpaf_amd.fused.stem_weight_of: weight.permute(2, 3, 1, 0).reshape(27, C)).
// C.       16 (MobileNetV3), 24 (shufflenetv2k16, ShuffleNetV2), 32 (k20 / k30 / k44, MobileNetV2), 42 (shufflenetv2kx5), 64
//          (SqueezeNet); one instantiation per (C, S).
// Arithmetic.  One FLOAT64 accumulator per output element, started at 0 and advanced by an EXPLICIT fma(x, w, acc) per tap in the
//          order t = 0 .. 26 -- rows, then columns, then input channels -- whatever the launch geometry (a product of two float32
//          numbers is exact in float64); the bias is added last, in float64 (no addition without a bias); ONE rounding to float32;
//          then the activation in float32.  The library is built with -ffp-contract=off: the fma calls are the only fused
//          operations.  Equal inputs give equal bits.  Why float64: the route's criterion is twice the error of torch's own float32
//          convolution, and at small shapes that convolution is MIOpen's direct kernel, which accumulates in float64 and is as good
//          as correctly rounded -- 27 float32 fmaf in any order measure 1.5 ... 4.4 times its error (rms 1.9 ... 2.5), this chain
//          1.0.  The 27 x V float64 fma are half-rate instructions; the inputs are converted once, when they are staged, and the
//          weights once per workgroup.
// Padding. A tap outside the image is a literal 0.0 in the staged patch: nothing is loaded for it (no clamped address, so an Inf
//          or NaN at a border pixel reaches exactly the windows that hold that pixel), and fma(0, w, acc) leaves acc's value.
// Activation codes (the trunk's: 0 none, 1 ReLU, 2 hardswish, 3 LeakyReLU(act_param), 4 ReLU clipped at act_param): act_f32 of
//          common.hpp, selects that keep a NaN.
//
// Work.    A workgroup of 256 threads computes a tile of 8 x 32 output pixels of one image (kStemTileH x kStemTileW; grid.x the tiles
//          of an image, grid.y the batch).  It first stages the input patch the tile needs -- ((8 - 1) S + 3) x ((32 - 1) S + 3)
//          pixels x 3 channels, 26 KB of float64 at S = 2 -- in LDS as three planes, every thread loading single floats in the order in which the
//          input is contiguous (channel innermost where the channel stride is below the pixel stride, else pixel innermost): every
//          input element comes from HBM once but for the one-pixel halo between tiles.  Then thread i takes the vector
//          i % VPP of the pixel's C / V channels (V = 2 floats, 8 bytes: an odd pixel of C = 42 begins on an 8-byte boundary only, and
//          27 x 4 float64 weights -- 216 registers -- leave one wave per SIMD or spill; with 27 x 2 the kernels take 182 registers, two
//          waves per SIMD, no scratch) and the pixels i / VPP, i / VPP + PPI, ... of the tile in row-major order, PPI = 256 / VPP
//          (rounded down; the 256 % VPP last threads of C = 24 and 42 only stage): its 27 x V weights and V biases stay in registers,
//          the 27 inputs of a pixel come from LDS (the threads of a pixel read the same 8 bytes: a broadcast), and neighbouring
//          threads store neighbouring vectors -- every output row segment of the tile is written once, contiguously.
// Indexing. 32-bit element indices into x and out; the host checks that the input's extent and the output's element count stay
//          below 2^31 and the batch within grid.y (capi_trunk.hip: opa_stem3x3_actp).
#include "common.hpp"

namespace opa {

constexpr int kStemTileH = 8, kStemTileW = 32, kStemThreads = 256;

template <int V> struct StemVec;
template <> struct alignas(8) StemVec<2> { float v[2]; };

template <int C, int S>
__global__ __launch_bounds__(kStemThreads) void stem3x3_kernel(const float* __restrict__ x, int xb, int xc, int xr, int xp,
                                                               const float* __restrict__ w, const float* __restrict__ bias,
                                                               float* __restrict__ out, int H, int W, int Ho, int Wo, int tiles_x,
                                                               int act, float act_param) {
    constexpr int V = 2, VPP = C / V, PPI = kStemThreads / VPP;
    constexpr int PH = (kStemTileH - 1) * S + 3, PW = (kStemTileW - 1) * S + 3, NE = 3 * PH * PW;
    static_assert(C % V == 0 && VPP <= kStemThreads, "a pixel's vectors fit a workgroup");
    __shared__ double patch[3][PH][PW];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int oy0 = ((int)blockIdx.x / tiles_x) * kStemTileH, ox0 = ((int)blockIdx.x % tiles_x) * kStemTileW;
    const int iy0 = oy0 * S - 1, ix0 = ox0 * S - 1;

    // the patch: zeros where it leaves the image
    const float* xi = x + (size_t)b * (size_t)xb;
    const bool channel_inner = xc < xp;
    constexpr int NL = (NE + kStemThreads - 1) / kStemThreads;      // loads per thread: all in flight before the first is used
    float staged[NL];
#pragma unroll
    for (int k = 0; k < NL; k++) {
        const int e = tid + k * kStemThreads;
        int ci, r, c;
        if (channel_inner) { ci = e % 3; c = (e / 3) % PW; r = e / (3 * PW); }
        else { c = e % PW; r = (e / PW) % PH; ci = e / (PW * PH); }
        const int iy = iy0 + r, ix = ix0 + c;
        staged[k] = 0.0f;
        if (e < NE && iy >= 0 && iy < H && ix >= 0 && ix < W) staged[k] = xi[ci * xc + iy * xr + ix * xp];
    }
    // the weights and the bias of this thread's channels (L2 hits for all but the first workgroups), in flight behind the patch
    const bool computes = tid < VPP * PPI;
    const int cv = tid % VPP;
    StemVec<V> wf[27], bf;
#pragma unroll
    for (int t = 0; t < 27; t++) wf[t] = *reinterpret_cast<const StemVec<V>*>(w + t * C + cv * V);
#pragma unroll
    for (int q = 0; q < V; q++) bf.v[q] = 0.0f;
    if (bias) bf = *reinterpret_cast<const StemVec<V>*>(bias + cv * V);
#pragma unroll
    for (int k = 0; k < NL; k++) {
        const int e = tid + k * kStemThreads;
        int ci, r, c;
        if (channel_inner) { ci = e % 3; c = (e / 3) % PW; r = e / (3 * PW); }
        else { c = e % PW; r = (e / PW) % PH; ci = e / (PW * PH); }
        if (e < NE) patch[ci][r][c] = (double)staged[k];
    }
    __syncthreads();
    if (!computes) return;
    double wv[27][V], bv[V];
#pragma unroll
    for (int t = 0; t < 27; t++)
#pragma unroll
        for (int q = 0; q < V; q++) wv[t][q] = (double)wf[t].v[q];
#pragma unroll
    for (int q = 0; q < V; q++) bv[q] = (double)bf.v[q];


    for (int p = tid / VPP; p < kStemTileH * kStemTileW; p += PPI) {
        const int ty = p / kStemTileW, tx = p % kStemTileW, oy = oy0 + ty, ox = ox0 + tx;
        if (oy >= Ho) break;                    // (row-major: every later pixel lies lower still)
        if (ox >= Wo) continue;
        double acc[V];
#pragma unroll
        for (int q = 0; q < V; q++) acc[q] = 0.0;
#pragma unroll
        for (int ky = 0; ky < 3; ky++)
#pragma unroll
            for (int kx = 0; kx < 3; kx++)
#pragma unroll
                for (int ci = 0; ci < 3; ci++) {
                    const double xin = patch[ci][ty * S + ky][tx * S + kx];
#pragma unroll
                    for (int q = 0; q < V; q++) acc[q] = fma(xin, wv[(ky * 3 + kx) * 3 + ci][q], acc[q]);
                }
        StemVec<V> o;
#pragma unroll
        for (int q = 0; q < V; q++) o.v[q] = act_f32((float)(bias ? acc[q] + bv[q] : acc[q]), act, act_param);
        *reinterpret_cast<StemVec<V>*>(out + (((unsigned)b * (unsigned)Ho + (unsigned)oy) * (unsigned)Wo + (unsigned)ox) * (unsigned)C + cv * V) = o;
    }
}

bool stem3x3_channels_ok(int C) { return C == 16 || C == 24 || C == 32 || C == 42 || C == 64; }

// grid.x of the launch: the tiles of one image
long long stem3x3_tiles(int H, int W, int S) {
    const long long ho = (H - 1) / S + 1, wo = (W - 1) / S + 1;
    return ((ho + kStemTileH - 1) / kStemTileH) * ((wo + kStemTileW - 1) / kStemTileW);
}

template <int C>
static hipError_t launch_stem_c(const float* x, int xb, int xc, int xr, int xp, const float* w, const float* bias, float* out, int B, int H,
                                int W, int S, int act, float act_param, hipStream_t st) {
    const int Ho = (H - 1) / S + 1, Wo = (W - 1) / S + 1, tiles_x = (Wo + kStemTileW - 1) / kStemTileW;
    const dim3 grid((unsigned)stem3x3_tiles(H, W, S), (unsigned)B);
    if (S == 1) stem3x3_kernel<C, 1><<<grid, kStemThreads, 0, st>>>(x, xb, xc, xr, xp, w, bias, out, H, W, Ho, Wo, tiles_x, act, act_param);
    else if (S == 2) stem3x3_kernel<C, 2><<<grid, kStemThreads, 0, st>>>(x, xb, xc, xr, xp, w, bias, out, H, W, Ho, Wo, tiles_x, act, act_param);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_stem3x3(const float* x, long long xb, long long xc, long long xr, long long xp, const float* w, const float* bias,
                          float* out, int B, int H, int W, int C, int S, int act, float act_param, hipStream_t st) {
#define OPA_STEM(C_) case C_: return launch_stem_c<C_>(x, (int)xb, (int)xc, (int)xr, (int)xp, w, bias, out, B, H, W, S, act, act_param, st)
    if (B == 1) xb = 0;                         // (the stride of a dimension of one element addresses nothing and may be any number)
    if (H == 1) xr = 0;
    if (W == 1) xp = 1;
    switch (C) {
        OPA_STEM(16); OPA_STEM(24); OPA_STEM(32); OPA_STEM(42); OPA_STEM(64);
        default: return hipErrorInvalidValue;
    }
#undef OPA_STEM
}

}  // namespace opa
