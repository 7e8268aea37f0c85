// Group norm + activation of a ShuffleNetV2K built with --shufflenetv2k-group-norm on gfx950 (reference network/basenetworks.py:376-400:
// GroupNorm((32 if c % 32 == 0 else 29) if c > 100 else 4, c) in place of every BatchNorm2d).  Its statistics belong to the image, so
// it folds into no convolution:
//     y[b, p, c] = act((x[b, p, c] - mean[b, g]) * rstd[b, g] * gamma[c] + beta[c]),   g = c / (C / G),
// mean and the (biased) variance taken over the (C / G) x HW elements of group g of image b.
//
// x is float32, channels innermost, [B, HW, C] with xs floats between pixels -- a dense channels-last tensor or a channel slice of a
// wider one, as the unit-mode GEMM's operands are: C, C / G and both pixel strides are even and the pointers on 8-byte boundaries
// (shufflenetv2k16's 174-channel slice begins 696 bytes into its pixel), so every access to x and y is ONE 8-byte vector of two
// channels.  Three launches:
//   moments       the pixels of an image are cut into chunks of kGnChunkPixels; a workgroup sums x and x^2 of one chunk for up to 128
//                 channel pairs (consecutive pairs across the lanes, `slots` pixels at a time) and writes ONE (sum, sum of squares) pair
//                 per (image, chunk, channel).  The stem's output at 641 px is 321 x 321 x 24 in B x 4 groups: 202 x B workgroups
//                 instead of 4 x B.
//   coefficients  one workgroup per (image, group): per channel the chunks' pairs are added in their order, then the channels of the
//                 group in their order; mean = sum / n, var = max(sumsq / n - mean^2, 0), rstd = 1 / sqrt(var + (double)eps), all in
//                 float64; per (image, channel) ONE rounding each: a = float(gamma * rstd), s = float(beta - mean * (double)a).
//   apply         y = act(fmaf(x, a, s)) in float32, the activation (act_f32 of common.hpp: codes 0 .. 4) last; y may be x itself
//                 (same pixel stride): a thread reads the two floats it writes and no other.
// HBM-bound streaming kernels -- x is read twice and written once --, so the sums are kept in float64 (the adds hide behind the
// loads; a product of two float32 numbers is exact in float64): every addition's order is fixed by the shape alone -- eight loads as
// a tree, the batches of a thread in sequence, the threads of a workgroup as a tree through the LDS, the chunks in sequence, the
// channels in sequence -- there are no atomics, and two calls give the same bits.  The library is built with -ffp-contract=off: the
// fmaf of the apply kernel is the only fused operation.
// Indexing.  64-bit offsets into x and y.  The host checks the grids (capi_trunk.hip: opa_groupnorm_actp): B <= 65535 (grid.z / .y),
//            HW <= 65535 * kGnChunkPixels (grid.y of the moments), C / G <= kGnMaxGroupWidth (the coefficients' LDS) and
//            HW * C / 2 < 2^31 (32-bit vector indices within an image in the apply kernel; its last workgroup counts less than 2^11
//            past the last vector, in unsigned arithmetic).
#include "common.hpp"

namespace opa {

constexpr int kGnLoads = 8;               // 8-byte loads a thread of the moments kernel has in flight
constexpr int kGnPairs = 128;             // channel pairs of one workgroup of the moments kernel, at most
constexpr int kGnApplyVecs = 4;           // 8-byte vectors per thread of the apply kernel

// the pairs are dealt out evenly: 174 of them (C = 348) are 2 x 87, not 128 + 46
__host__ __device__ inline int gn_pairs_per_workgroup(int cvs) {
    const int wgs = (cvs + kGnPairs - 1) / kGnPairs;
    return (cvs + wgs - 1) / wgs;
}

// partial [B][chunks][C] (sum, sum of squares)
__global__ __launch_bounds__(256) void gn_moments_kernel(const float* __restrict__ x, long long xs, long long HW, int C,
                                                         double2* __restrict__ partial) {
    __shared__ double red[256][4];
    const int tid = threadIdx.x;
    const int cvs = C / 2, cvb = gn_pairs_per_workgroup(cvs);          // channel pairs; ... of one workgroup
    const int slots = 256 / cvb;                                       // pixels the workgroup reads at a time
    const int slot = tid / cvb, cv = blockIdx.x * cvb + (tid - slot * cvb);
    const bool active = slot < slots && cv < cvs;
    const long long chunk = blockIdx.y, chunks = gridDim.y, b = blockIdx.z;
    const long long p0 = chunk * kGnChunkPixels, p1 = p0 + kGnChunkPixels < HW ? p0 + kGnChunkPixels : HW;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};                              // sum, sum of squares of the pair's first channel; of its second
    if (active) {
        const float* base = x + (size_t)b * (size_t)HW * (size_t)xs + (size_t)cv * 2;
        for (long long p = p0 + slot; p < p1; p += (long long)slots * kGnLoads) {
            float2 v[kGnLoads];
#pragma unroll
            for (int j = 0; j < kGnLoads; j++) {
                const long long pj = p + (long long)j * slots;
                v[j] = make_float2(0.f, 0.f);
                if (pj < p1) v[j] = *reinterpret_cast<const float2*>(base + (size_t)pj * (size_t)xs);
            }
#define OPA_GN_SUM(m) ((((double)v[0].m + (double)v[1].m) + ((double)v[2].m + (double)v[3].m)) + \
                       (((double)v[4].m + (double)v[5].m) + ((double)v[6].m + (double)v[7].m)))
#define OPA_GN_SQ(j, m) ((double)v[j].m * (double)v[j].m)
#define OPA_GN_SUMSQ(m) (((OPA_GN_SQ(0, m) + OPA_GN_SQ(1, m)) + (OPA_GN_SQ(2, m) + OPA_GN_SQ(3, m))) + \
                         ((OPA_GN_SQ(4, m) + OPA_GN_SQ(5, m)) + (OPA_GN_SQ(6, m) + OPA_GN_SQ(7, m))))
            acc[0] += OPA_GN_SUM(x); acc[1] += OPA_GN_SUMSQ(x); acc[2] += OPA_GN_SUM(y); acc[3] += OPA_GN_SUMSQ(y);
#undef OPA_GN_SUM
#undef OPA_GN_SQ
#undef OPA_GN_SUMSQ
        }
    }
#pragma unroll
    for (int q = 0; q < 4; q++) red[tid][q] = acc[q];
    __syncthreads();
    for (int n = slots; n > 1;) {                            // slot s takes slot s + h: a tree whose shape `slots` fixes
        const int h = (n + 1) / 2;
        if (active && slot + h < n) {
#pragma unroll
            for (int q = 0; q < 4; q++) red[tid][q] += red[tid + h * cvb][q];
        }
        __syncthreads();
        n = h;
    }
    if (active && slot == 0) {
        double2* o = partial + ((size_t)b * (size_t)chunks + (size_t)chunk) * (size_t)C + (size_t)cv * 2;
        o[0] = make_double2(red[tid][0], red[tid][1]);
        o[1] = make_double2(red[tid][2], red[tid][3]);
    }
}

// one workgroup per (group, image); dynamic LDS: double2 sums[C / G]; coef [B][C] (a, s)
__global__ __launch_bounds__(64) void gn_coefficients_kernel(const double2* __restrict__ partial, int chunks, long long HW, int C, int G,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                             float2* __restrict__ coef) {
    extern __shared__ double2 gn_sums[];
    __shared__ double stats[2];
    const int tid = threadIdx.x, cg = C / G, c0 = blockIdx.x * cg;
    const size_t b = blockIdx.y;
    for (int i = tid; i < cg; i += blockDim.x) {
        double s = 0.0, q = 0.0;
        for (int ch = 0; ch < chunks; ch++) {
            const double2 v = partial[(b * (size_t)chunks + (size_t)ch) * (size_t)C + (size_t)(c0 + i)];
            s += v.x; q += v.y;
        }
        gn_sums[i] = make_double2(s, q);
    }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0, q = 0.0;
        for (int i = 0; i < cg; i++) { s += gn_sums[i].x; q += gn_sums[i].y; }
        const double n = (double)cg * (double)HW;
        const double mean = s / n;
        double var = q / n - mean * mean;
        var = var < 0.0 ? 0.0 : var;                         // (a select: NaN stays)
        stats[0] = mean;
        stats[1] = 1.0 / sqrt(var + (double)eps);
    }
    __syncthreads();
    const double mean = stats[0], rstd = stats[1];
    for (int i = tid; i < cg; i += blockDim.x) {
        const int c = c0 + i;
        const float a = (float)((gamma ? (double)gamma[c] : 1.0) * rstd);
        const float s = (float)((beta ? (double)beta[c] : 0.0) - mean * (double)a);
        coef[b * (size_t)C + (size_t)c] = make_float2(a, s);
    }
}

// (x and out may be the same tensor: neither is __restrict__); 32-bit vector indices within an image
__global__ __launch_bounds__(256) void gn_apply_kernel(const float* x, long long xs, float* out, long long os, long long HW, int C,
                                                       const float4* __restrict__ coef, int act, float act_param) {
    const unsigned cvs = (unsigned)C / 2u, total = (unsigned)HW * cvs;
    const unsigned step_p = 256u / cvs, step_c = 256u % cvs;          // 256 vectors on: so many pixels and pairs further
    const size_t b = blockIdx.y;
    const float* xb = x + b * (size_t)HW * (size_t)xs;
    float* ob = out + b * (size_t)HW * (size_t)os;
    const float4* kb = coef + b * (size_t)cvs;
    const unsigned i0 = blockIdx.x * (256u * kGnApplyVecs) + threadIdx.x;
    unsigned p[kGnApplyVecs], cv[kGnApplyVecs];
    float2 v[kGnApplyVecs];
    p[0] = i0 / cvs;
    cv[0] = i0 - p[0] * cvs;
#pragma unroll
    for (int j = 1; j < kGnApplyVecs; j++) {
        cv[j] = cv[j - 1] + step_c;
        p[j] = p[j - 1] + step_p + (cv[j] >= cvs ? 1u : 0u);
        cv[j] -= cv[j] >= cvs ? cvs : 0u;
    }
#pragma unroll
    for (int j = 0; j < kGnApplyVecs; j++) {
        v[j] = make_float2(0.f, 0.f);
        if (i0 + (unsigned)j * 256u < total) v[j] = *reinterpret_cast<const float2*>(xb + (size_t)p[j] * (size_t)xs + (size_t)cv[j] * 2);
    }
#pragma unroll
    for (int j = 0; j < kGnApplyVecs; j++) {
        if (i0 + (unsigned)j * 256u >= total) continue;
        const float4 k = kb[cv[j]];                                    // (a, s) of the pair's two channels
        float2 y;
        y.x = act_f32(fmaf(v[j].x, k.x, k.y), act, act_param);
        y.y = act_f32(fmaf(v[j].y, k.z, k.w), act, act_param);
        *reinterpret_cast<float2*>(ob + (size_t)p[j] * (size_t)os + (size_t)cv[j] * 2) = y;
    }
}

size_t groupnorm_partial_bytes(int B, long long HW, int C) { return (size_t)B * (size_t)gn_chunks(HW) * (size_t)C * sizeof(double2); }

hipError_t launch_groupnorm(const float* x, long long xs, const float* gamma, const float* beta, float* out, long long os, int B,
                            long long HW, int C, int G, float eps, int act, float act_param, void* workspace, hipStream_t st) {
    double2* partial = (double2*)workspace;
    float2* coef = (float2*)((char*)workspace + groupnorm_partial_bytes(B, HW, C));
    const int cvs = C / 2, cvb = gn_pairs_per_workgroup(cvs), chunks = (int)gn_chunks(HW);
    gn_moments_kernel<<<dim3((unsigned)((cvs + cvb - 1) / cvb), (unsigned)chunks, (unsigned)B), 256, 0, st>>>(x, xs, HW, C, partial);
    prof_mark(st, "gn_moments_kernel");
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    gn_coefficients_kernel<<<dim3((unsigned)G, (unsigned)B), 64, (size_t)(C / G) * sizeof(double2), st>>>(partial, chunks, HW, C, G, gamma,
                                                                                                         beta, eps, coef);
    prof_mark(st, "gn_coefficients_kernel");
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const long long vecs = HW * cvs, per_wg = 256 * kGnApplyVecs;
    gn_apply_kernel<<<dim3((unsigned)((vecs + per_wg - 1) / per_wg), (unsigned)B), 256, 0, st>>>(x, xs, out, os, HW, C, (const float4*)coef,
                                                                                                  act, act_param);
    prof_mark(st, "gn_apply_kernel");
    return hipGetLastError();
}

}  // namespace opa
