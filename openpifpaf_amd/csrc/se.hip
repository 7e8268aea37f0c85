// Squeeze-and-excitation of a MobileNetV3 block on gfx950 (producer side; reference network/basenetworks.py:432-446 takes
// torchvision's block: x * hardsigmoid(fc2(relu(fc1(mean over the pixels of x))))).
//
// x is the activated depthwise output, channels-last float32 [B, HW, C] with xs floats between pixels.  Three launches:
//   pool   the pixels of an image are cut into chunks of kSePoolPixels; a workgroup sums one chunk for up to 64 channel
//          vectors (16-byte loads, consecutive channels across the lanes) and writes ONE partial sum per channel.  At 641 px and
//          batch 32 the first SE block pools 161 x 161 x 72 per image (18 channel vectors: one group): 51 x 32 workgroups instead of 32.
//   gate   one workgroup per image: adds the chunks' partial sums in their order, then the two small matrix-vector products
//          (a wave per output row, lanes along the row) and the hardsigmoid.
//   scale  x[b, p, c] *= g[b, c], one 16-byte vector per thread.
// HBM-bound streaming kernels, so the sums are kept in float64 (the adds hide behind the loads): every addition's order is fixed
// by the shape alone -- eight loads as a tree, the batches of a thread in sequence, the threads of a workgroup as a tree through
// the LDS, the chunks in sequence -- there are no atomics, and two calls give the same bits.  The mean is rounded to float32 once.
#include "common.hpp"

namespace opa {

constexpr int kSeLoads = 8;               // 16-byte loads a thread has in flight

__global__ __launch_bounds__(256) void se_pool_kernel(const float* __restrict__ x, long long xs, long long HW, int C,
                                                      double* __restrict__ partial) {
    __shared__ double red[256][4];
    const int tid = threadIdx.x;
    const int cvs = C / 4, cvb = cvs < 64 ? cvs : 64;        // channel vectors; ... of one workgroup
    const int slots = 256 / cvb;                             // pixels the workgroup reads at a time
    const int slot = tid / cvb, cv = blockIdx.x * cvb + (tid - slot * cvb);
    const bool active = slot < slots && cv < cvs;
    const long long chunk = blockIdx.y, chunks = gridDim.y, b = blockIdx.z;
    const long long p0 = chunk * kSePoolPixels, p1 = p0 + kSePoolPixels < HW ? p0 + kSePoolPixels : HW;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (active) {
        const float* base = x + (size_t)b * HW * xs + (size_t)cv * 4;
        for (long long p = p0 + slot; p < p1; p += (long long)slots * kSeLoads) {
            float4 v[kSeLoads];
#pragma unroll
            for (int j = 0; j < kSeLoads; j++) {
                const long long pj = p + (long long)j * slots;
                v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (pj < p1) v[j] = *reinterpret_cast<const float4*>(base + (size_t)pj * xs);
            }
#define OPA_SE_TREE(m) ((((double)v[0].m + (double)v[1].m) + ((double)v[2].m + (double)v[3].m)) + \
                        (((double)v[4].m + (double)v[5].m) + ((double)v[6].m + (double)v[7].m)))
            acc[0] += OPA_SE_TREE(x); acc[1] += OPA_SE_TREE(y); acc[2] += OPA_SE_TREE(z); acc[3] += OPA_SE_TREE(w);
#undef OPA_SE_TREE
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
        double* o = partial + ((size_t)b * chunks + chunk) * C + (size_t)cv * 4;
        *reinterpret_cast<double2*>(o) = make_double2(red[tid][0], red[tid][1]);
        *reinterpret_cast<double2*>(o + 2) = make_double2(red[tid][2], red[tid][3]);
    }
}

__device__ __forceinline__ double se_wave_sum(double a) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) a += __shfl_xor(a, d, 64);
    return a;
}

// dynamic LDS: float mean[C], float hidden[S]
__global__ __launch_bounds__(1024) void se_gate_kernel(const double* __restrict__ partial, int chunks, long long HW, int C, int S,
                                                       const float* __restrict__ w1, const float* __restrict__ b1,
                                                       const float* __restrict__ w2, const float* __restrict__ b2,
                                                       float* __restrict__ gate, float* __restrict__ mean_out) {
    extern __shared__ float se_lds[];
    float* mean = se_lds;
    float* hidden = se_lds + C;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves = blockDim.x >> 6;
    const size_t b = blockIdx.x;
    for (int c = tid; c < C; c += blockDim.x) {
        double s = 0.0;
        for (int ch = 0; ch < chunks; ch++) s += partial[(b * chunks + ch) * C + c];
        mean[c] = (float)(s / (double)HW);
        if (mean_out) mean_out[b * C + c] = mean[c];
    }
    __syncthreads();
    for (int j = wave; j < S; j += waves) {                  // hidden = relu(W1 mean + b1), W1 [S, C]
        double a = 0.0;
        for (int c = lane; c < C; c += 64) a = fma((double)w1[(size_t)j * C + c], (double)mean[c], a);
        a = se_wave_sum(a);
        if (lane == 0) hidden[j] = fmaxf((float)(a + (double)b1[j]), 0.0f);
    }
    __syncthreads();
    for (int c = wave; c < C; c += waves) {                  // g = hardsigmoid(W2 hidden + b2), W2 [C, S]
        double a = 0.0;
        for (int j = lane; j < S; j += 64) a = fma((double)w2[(size_t)c * S + j], (double)hidden[j], a);
        a = se_wave_sum(a);
        if (lane == 0) gate[b * C + c] = hardsigmoid_f32((float)(a + (double)b2[c]));
    }
}

__global__ __launch_bounds__(256) void se_scale_kernel(float* __restrict__ x, long long xs, long long HW, int C,
                                                       const float* __restrict__ gate) {
    const int cvs = C / 4;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= HW * cvs) return;
    const long long p = i / cvs;
    const int c = (int)(i - p * cvs) * 4;
    const size_t b = blockIdx.y;
    const float4 g = *reinterpret_cast<const float4*>(gate + b * C + c);
    float4* px = reinterpret_cast<float4*>(x + (b * HW + p) * xs + c);
    float4 v = *px;
    v.x *= g.x; v.y *= g.y; v.z *= g.z; v.w *= g.w;
    *px = v;
}

hipError_t launch_se_pool(const float* x, long long xs, int B, long long HW, int C, double* partial, hipStream_t st) {
    const int cvs = C / 4, cvb = cvs < 64 ? cvs : 64;
    dim3 grid((unsigned)((cvs + cvb - 1) / cvb), (unsigned)se_pool_chunks(HW), (unsigned)B);
    se_pool_kernel<<<grid, 256, 0, st>>>(x, xs, HW, C, partial);
    prof_mark(st, "se_pool_kernel");
    return hipGetLastError();
}

hipError_t launch_se_gate(const double* partial, int B, long long HW, int C, int S, const float* w1, const float* b1,
                          const float* w2, const float* b2, float* gate, float* mean_out, hipStream_t st) {
    se_gate_kernel<<<(unsigned)B, 1024, (size_t)(C + S) * sizeof(float), st>>>(partial, (int)se_pool_chunks(HW), HW, C, S, w1, b1,
                                                                               w2, b2, gate, mean_out);
    prof_mark(st, "se_gate_kernel");
    return hipGetLastError();
}

hipError_t launch_se_scale(float* x, long long xs, int B, long long HW, int C, const float* gate, hipStream_t st) {
    dim3 grid((unsigned)((HW * (C / 4) + 255) / 256), (unsigned)B);
    se_scale_kernel<<<grid, 256, 0, st>>>(x, xs, HW, C, gate);
    prof_mark(st, "se_scale_kernel");
    return hipGetLastError();
}

}  // namespace opa
