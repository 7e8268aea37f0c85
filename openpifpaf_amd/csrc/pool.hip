// The input max-pool of a ResNet (reference network/basenetworks.py:85-93: torchvision's MaxPool2d(3, 2, 1) behind the stem) with the
// stem's epilogue in front of it, in one pass over a channels-last activation:
//     out[b, oy, ox, c] = max over the 3x3 window at (2 oy - 1, 2 ox - 1) of act(x[b, iy, ix, c] + bias[c])
// x + bias and ReLU are non-decreasing in x and so is the rounding to the storage type: the maximum of the window is taken FIRST,
// of the stored values (exact in float32), and bias, ReLU and the one rounding are applied once -- the same NUMBERS as
// max_pool2d(relu(x + bias), 3, 2, 1) computes with nine of each (torch.equal; where the result is a zero its sign may differ, since
// x + bias and ReLU may turn -0.0 into +0.0 before torch compares).  Without bias and ReLU the bits are torch's: the window is
// scanned in torch's order from -inf with a strict comparison, so the first of two equal values -- +0.0 and -0.0 -- stays.
// The largest activation of the network (64 channels at half resolution) is read once and a quarter of it written, where the
// epilogue pass + torch's pool read it twice and write 1.25 of it.
// Padding never wins: only pixels inside the image are compared, and every window holds at least one.  In floor mode that is its
// centre (2 oy, 2 ox); in ceil mode (SqueezeNet's pools, reference network/basenetworks.py:461-487: MaxPool2d(3, 2, 1,
// ceil_mode=True); the launcher passes ho, wo) an even H has one more output row whose window holds row H - 1 alone -- its first
// row, the centre lies outside -- and likewise column W - 1 for an even W.  A NaN in the
// window gives NaN, as in torch (fmaxf would drop it: the comparison is written out), and ReLU keeps it (v < 0 ? 0 : v).
// One thread per output pixel and 16-byte vector of channels (4 float32 | 8 bfloat16); 32-bit vector indices (the host checks).
#include "common.hpp"
#include "vec16.hpp"

namespace opa {

template <int DT, bool BIAS, bool RELU>
__global__ __launch_bounds__(256) void maxpool3x3s2_kernel(const Vec16* __restrict__ x, const Vec16* __restrict__ bias,
                                                           Vec16* __restrict__ out, unsigned n_vec, int H, int W, int ho, int wo, int vpp) {
    constexpr int N = Elem<DT>::kPerVec;
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_vec) return;
    const unsigned cv = i % (unsigned)vpp, p = i / (unsigned)vpp;          // vector of the pixel, output pixel
    const unsigned ox = p % (unsigned)wo, q = p / (unsigned)wo, oy = q % (unsigned)ho, b = q / (unsigned)ho;
    const int iy0 = 2 * (int)oy - 1, ix0 = 2 * (int)ox - 1;
    Vec16 v[9];
    bool in[9];
#pragma unroll
    for (int t = 0; t < 9; t++) {              // every load of the window in flight before the first comparison
        const int iy = iy0 + t / 3, ix = ix0 + t % 3;
        in[t] = iy >= 0 && iy < H && ix >= 0 && ix < W;
        if (in[t]) v[t] = x[((b * (unsigned)H + (unsigned)iy) * (unsigned)W + (unsigned)ix) * (unsigned)vpp + cv];
    }
    float m[N];
#pragma unroll
    for (int k = 0; k < N; k++) m[k] = -INFINITY;      // (at least one pixel of every window is inside: see the header)
#pragma unroll
    for (int t = 0; t < 9; t++) {              // torch's scan: rows, then columns, the first of equal values stays
        if (!in[t]) continue;
        float f[N];
        Elem<DT>::unpack(v[t], f);
#pragma unroll
        for (int k = 0; k < N; k++) m[k] = (f[k] > m[k] || f[k] != f[k]) ? f[k] : m[k];      // (a NaN stays: nothing is > NaN)
    }
    if (BIAS) {
        float bf[N];
        Elem<DT>::unpack(bias[cv], bf);
#pragma unroll
        for (int k = 0; k < N; k++) m[k] = m[k] + bf[k];
    }
    if (RELU) {
#pragma unroll
        for (int k = 0; k < N; k++) m[k] = m[k] < 0.0f ? 0.0f : m[k];
    }
    Vec16 o;
    Elem<DT>::pack(m, o);
    out[i] = o;
}

static int pool_per_vec(int dtype) { return dtype == 0 ? 4 : 8; }

// output rows of kernel 3, stride 2, padding 1 for h >= 1 input rows.  Floor mode: (h - 1) / 2 + 1.  Ceil mode is torch's rule:
// ceil((h - 1) / 2) + 1, one less where the last window would begin behind the input and its left padding ((o - 1) * 2 >= h + 1:
// never the case for this kernel, stride and padding; kept as torch states it) -- the floor-mode size for odd h, one more for even h
int maxpool3x3_out(int h, int ceil_mode) {
    if (!ceil_mode) return (h - 1) / 2 + 1;
    int o = h / 2 + 1;
    if ((o - 1) * 2 >= h + 1) o--;
    return o;
}

// workgroups of the launch (one thread per output pixel and vector)
long long maxpool3x3_blocks(int B, int H, int W, int C, int ceil_mode) {
    const long long ho = maxpool3x3_out(H, ceil_mode), wo = maxpool3x3_out(W, ceil_mode);
    return ((long long)B * ho * wo * (C / 4) + 255) / 256;      // (float32's vector count: the larger of the two)
}

template <int DT>
static hipError_t launch_pool_dt(const void* x, const void* bias, void* out, int B, int H, int W, int C, int relu, int ceil_mode, hipStream_t st) {
    const int ho = maxpool3x3_out(H, ceil_mode), wo = maxpool3x3_out(W, ceil_mode), vpp = C / Elem<DT>::kPerVec;
    const unsigned n_vec = (unsigned)((long long)B * ho * wo * vpp);
    const unsigned blocks = (n_vec + 255u) / 256u;
    const Vec16* xv = (const Vec16*)x; const Vec16* bv = (const Vec16*)bias; Vec16* ov = (Vec16*)out;
#define OPA_POOL(BIAS_, RELU_) maxpool3x3s2_kernel<DT, BIAS_, RELU_><<<blocks, 256, 0, st>>>(xv, bv, ov, n_vec, H, W, ho, wo, vpp)
    if (bias) { if (relu) OPA_POOL(true, true); else OPA_POOL(true, false); }
    else { if (relu) OPA_POOL(false, true); else OPA_POOL(false, false); }
#undef OPA_POOL
    return hipGetLastError();
}

hipError_t launch_maxpool3x3(const void* x, const void* bias, void* out, int dtype, int B, int H, int W, int C, int relu, hipStream_t st,
                             int ceil_mode) {
    if (C % pool_per_vec(dtype) != 0) return hipErrorInvalidValue;
    switch (dtype) {
        case 0: return launch_pool_dt<0>(x, bias, out, B, H, W, C, relu, ceil_mode, st);
        case 2: return launch_pool_dt<2>(x, bias, out, B, H, W, C, relu, ceil_mode, st);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace opa
