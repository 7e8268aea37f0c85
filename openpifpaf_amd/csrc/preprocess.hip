// Image preprocessing in front of the network on gfx950: packed uint8 RGB frames of any sizes -> rescale with the
// reference's arithmetic -> centre pad with its fill colour -> ToTensor + Normalize -> float32 batch (NCHW or
// channels-last), one launch per pass for the WHOLE batch (reference transforms/scale.py:42-63,150-174, pad.py:15-112,
// transforms/__init__.py:26-33).  Each image is one row of a descriptor table (opa_pre_image, include/openpifpaf_amd.h).
//
//  preprocess_h_kernel   Pillow's horizontal pass: frame [h0, w0, 3] -> uint8 intermediate [h0, pitch] (images whose width
//                        changes only).  One workgroup = one source row x 256 output columns.
//  preprocess_v_kernel   Pillow's vertical pass over the intermediate (or the frame itself where the width is unchanged),
//                        centre pad, look-up normalisation, store.  One workgroup = one canvas row x 256 columns.
//  preprocess_zoom_kernel  the same tail for scipy's order-1 zoom (--precise-rescaling): four source pixels per output,
//                        weighted and summed in double in scipy's order.
//
// All three are HBM-bound (a handful of integer multiply-adds per byte), so what matters is how the bytes move: source
// rows are byte rows of arbitrary alignment, and every one of them is brought in as aligned 16-B vectors through LDS
// (stage_span: the row start is aligned down, the taps then read bytes from LDS); the intermediate's pitch is a multiple
// of 16 so that pass H stores 16-B vectors too.  No kernel divides: the normalised value of every byte comes from a
// 3 x 256 float32 table the host forms with the host pipeline's own expression, so equality with it is by construction.
// Tap counts are run-time values of the tables (a 4000-px frame reduced to 641 has 15).
#include "common.hpp"

namespace opa {

constexpr int kPreCols = 256;                        // output columns per workgroup = its threads
constexpr int kPreTapRows = 8;                       // tap rows pass V stages per round
constexpr int kPreRowBytes = kPreCols * 3 + 32;      // LDS bytes of 256 staged pixels: up to 15 B in front, vectors of 16
constexpr int kPrePrecisionBits = 22;                // Pillow's fixed-point precision for 8-bit images (32 - 8 - 2)

// Copies the aligned 16-B vectors that cover src[0, nbytes) to `lds` (16-B aligned): src[i] is then lds[shift + i], and
// shift (< 16) is returned.  The buffer src lies in is 16-B aligned and a multiple of 16 long, so every vector is inside it.
__device__ __forceinline__ int stage_span(unsigned char* lds, const unsigned char* src, int nbytes) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(src);
    const int shift = (int)(a & 15);
    const uint4* g = reinterpret_cast<const uint4*>(a - shift);
    const int nvec = (shift + nbytes + 15) >> 4;
    for (int i = threadIdx.x; i < nvec; i += kPreCols) reinterpret_cast<uint4*>(lds)[i] = g[i];
    return shift;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ void store_pixel(float* __restrict__ out, int b, int Y, int X, int ch, int cw, int channels_last,
                                            float r, float g, float bl) {
    if (channels_last) {
        float* p = out + (((size_t)b * ch + Y) * cw + X) * 3;          // 12 contiguous bytes per pixel
        p[0] = r; p[1] = g; p[2] = bl;
    } else {
        const size_t plane = (size_t)ch * cw;
        float* p = out + (size_t)b * 3 * plane + (size_t)Y * cw + X;   // three coalesced planes
        p[0] = r; p[plane] = g; p[2 * plane] = bl;
    }
}

extern __shared__ __attribute__((aligned(16))) unsigned char pre_lds[];

// LDS: [0, 784) the 256 output pixels of the workgroup, then the staged source span (in_cap pixels + 32 bytes).
__global__ __launch_bounds__(kPreCols) void preprocess_h_kernel(const opa_pre_image* __restrict__ images,
                                                                const unsigned char* __restrict__ frames,
                                                                const int32_t* __restrict__ tables,
                                                                unsigned char* __restrict__ ws, int in_cap) {
    const opa_pre_image d = images[blockIdx.y];
    if (d.tw == d.w0) return;                                           // pass V reads the frame itself
    const int chunks = (d.tw + kPreCols - 1) / kPreCols;
    const int y = blockIdx.x / chunks, x0 = (blockIdx.x - y * chunks) * kPreCols;
    if (y >= d.h0) return;
    const int x1 = min(x0 + kPreCols, d.tw);                            // this workgroup: columns [x0, x1) of row y
    const int32_t* tab = tables + d.x_table;                            // [1 + ksize][tw]
    const int ks = d.x_ksize;
    const int lo = clampi(tab[x0], 0, d.w0 - 1);                        // `first` never decreases along the axis
    const int hi = min(max(tab[x1 - 1], lo) + ks, d.w0);
    const int npix = min(hi - lo, in_cap);                              // (the host sized in_cap for the widest span)
    unsigned char* lds_out = pre_lds;
    unsigned char* lds_in = pre_lds + kPreRowBytes - 16;
    const int shift = stage_span(lds_in, frames + d.src_offset + ((size_t)y * d.w0 + lo) * 3, npix * 3);
    __syncthreads();
    const int x = x0 + (int)threadIdx.x;
    if (x < x1) {
        const int first = tab[x] - lo;
        int r = 1 << (kPrePrecisionBits - 1), g = r, b = r;
        for (int k = 0; k < ks; k++) {                                  // taps beyond a sample's count carry weight 0
            const int w = tab[(size_t)(1 + k) * d.tw + x];
            const unsigned char* p = lds_in + shift + clampi(first + k, 0, npix - 1) * 3;
            r += (int)p[0] * w; g += (int)p[1] * w; b += (int)p[2] * w;
        }
        unsigned char* q = lds_out + threadIdx.x * 3;
        q[0] = (unsigned char)clampi(r >> kPrePrecisionBits, 0, 255);
        q[1] = (unsigned char)clampi(g >> kPrePrecisionBits, 0, 255);
        q[2] = (unsigned char)clampi(b >> kPrePrecisionBits, 0, 255);
    }
    __syncthreads();
    // the row's pitch is a multiple of 16 and x0 * 3 one of 768: whole vectors (the last one may reach into the row's padding)
    const int pitch = (d.tw * 3 + 15) & ~15;
    uint4* dst = reinterpret_cast<uint4*>(ws + d.mid_offset + (size_t)y * pitch + (size_t)x0 * 3);
    const int nvec = ((x1 - x0) * 3 + 15) >> 4;
    if ((int)threadIdx.x < nvec) dst[threadIdx.x] = reinterpret_cast<const uint4*>(lds_out)[threadIdx.x];
}

__global__ __launch_bounds__(kPreCols) void preprocess_v_kernel(const opa_pre_image* __restrict__ images,
                                                                const unsigned char* __restrict__ frames,
                                                                const int32_t* __restrict__ tables,
                                                                const unsigned char* __restrict__ ws,
                                                                const float* __restrict__ lut, float* __restrict__ out,
                                                                int ch, int cw, int channels_last, unsigned fill) {
    __shared__ __attribute__((aligned(16))) unsigned char rows[kPreTapRows * kPreRowBytes];
    __shared__ float s_lut[3 * 256];
    const int b = blockIdx.z, Y = blockIdx.y, X0 = blockIdx.x * kPreCols;
    const opa_pre_image d = images[b];
    for (int i = threadIdx.x; i < 3 * 256; i += kPreCols) s_lut[i] = lut[i];
    const int X = X0 + (int)threadIdx.x;
    const int y = Y - d.top;
    const int xlo = max(X0, d.left), xhi = min(min(X0 + kPreCols, cw), d.left + d.tw);   // canvas columns that show the image
    const bool row_inside = y >= 0 && y < d.th && xlo < xhi;                             // the same for the whole workgroup
    const bool inside = row_inside && X >= xlo && X < xhi;
    int r = (int)(fill & 255u), g = (int)((fill >> 8) & 255u), bl = (int)((fill >> 16) & 255u);
    if (row_inside) {
        const bool direct = d.tw == d.w0;                               // no horizontal pass: the frame is the source
        const unsigned char* src = direct ? frames + d.src_offset : ws + d.mid_offset;
        const size_t pitch = direct ? (size_t)d.w0 * 3 : (size_t)((d.tw * 3 + 15) & ~15);
        const size_t begin = (size_t)(xlo - d.left) * 3;
        const int nbytes = (xhi - xlo) * 3;
        const int px = (X - xlo) * 3;
        if (d.th == d.h0) {                                             // the row is copied
            const int shift = stage_span(rows, src + (size_t)y * pitch + begin, nbytes);
            __syncthreads();
            if (inside) { const unsigned char* p = rows + shift + px; r = p[0]; g = p[1]; bl = p[2]; }
        } else {
            const int32_t* tab = tables + d.y_table;                    // [1 + ksize][th]
            const int ks = d.y_ksize, first = clampi(tab[y], 0, d.h0 - 1);
            int ar = 1 << (kPrePrecisionBits - 1), ag = ar, ab = ar;
            for (int k0 = 0; k0 < ks; k0 += kPreTapRows) {
                const int n = min(kPreTapRows, ks - k0);
                if (k0) __syncthreads();
                int shift[kPreTapRows];
#pragma unroll
                for (int k = 0; k < kPreTapRows; k++)
                    if (k < n)
                        shift[k] = stage_span(rows + k * kPreRowBytes,
                                              src + (size_t)min(first + k0 + k, d.h0 - 1) * pitch + begin, nbytes);
                __syncthreads();
                if (inside) {
#pragma unroll
                    for (int k = 0; k < kPreTapRows; k++)
                        if (k < n) {
                            const int w = tab[(size_t)(1 + k0 + k) * d.th + y];
                            const unsigned char* p = rows + k * kPreRowBytes + shift[k] + px;
                            ar += (int)p[0] * w; ag += (int)p[1] * w; ab += (int)p[2] * w;
                        }
                }
            }
            if (inside) {
                r = clampi(ar >> kPrePrecisionBits, 0, 255);
                g = clampi(ag >> kPrePrecisionBits, 0, 255);
                bl = clampi(ab >> kPrePrecisionBits, 0, 255);
            }
        }
    } else {
        __syncthreads();                                                // s_lut
    }
    if (X < cw) store_pixel(out, b, Y, X, ch, cw, channels_last, s_lut[r], s_lut[256 + g], s_lut[512 + bl]);
}

// One axis table of the zoom: i0[n], i1[n], outside[n] (int32), then from the next even word w0[n], w1[n] (double).
struct ZoomAxis {
    const int32_t* i0; const int32_t* i1; const int32_t* outside; const double* w0; const double* w1;
    __device__ ZoomAxis(const int32_t* t, int n)
        : i0(t), i1(t + n), outside(t + 2 * n), w0(reinterpret_cast<const double*>(t + ((3 * n + 1) & ~1))), w1(w0 + n) {}
};

// LDS: the look-up table (3072 B), then the staged spans of the two source rows (in_cap pixels + 32 bytes each).
__global__ __launch_bounds__(kPreCols) void preprocess_zoom_kernel(const opa_pre_image* __restrict__ images,
                                                                   const unsigned char* __restrict__ frames,
                                                                   const int32_t* __restrict__ tables,
                                                                   const float* __restrict__ lut, float* __restrict__ out,
                                                                   int ch, int cw, int channels_last, unsigned fill,
                                                                   int in_cap) {
    float* s_lut = reinterpret_cast<float*>(pre_lds);
    const int row_bytes = (in_cap * 3 + 32 + 15) & ~15;
    unsigned char* lds_a = pre_lds + 3 * 256 * sizeof(float);
    unsigned char* lds_b = lds_a + row_bytes;
    const int b = blockIdx.z, Y = blockIdx.y, X0 = blockIdx.x * kPreCols;
    const opa_pre_image d = images[b];
    for (int i = threadIdx.x; i < 3 * 256; i += kPreCols) s_lut[i] = lut[i];
    const int X = X0 + (int)threadIdx.x;
    const int y = Y - d.top;
    const int xlo = max(X0, d.left), xhi = min(min(X0 + kPreCols, cw), d.left + d.tw);
    const bool row_inside = y >= 0 && y < d.th && xlo < xhi;
    const bool inside = row_inside && X >= xlo && X < xhi;
    int r = (int)(fill & 255u), g = (int)((fill >> 8) & 255u), bl = (int)((fill >> 16) & 255u);
    if (row_inside) {
        const ZoomAxis ay(tables + d.y_table, d.th), ax(tables + d.x_table, d.tw);
        const int y0 = clampi(ay.i0[y], 0, d.h0 - 1), y1 = clampi(ay.i1[y], 0, d.h0 - 1);
        const double wy0 = ay.w0[y], wy1 = ay.w1[y];
        const int lo = clampi(ax.i0[xlo - d.left], 0, d.w0 - 1);        // i0 never decreases along the axis, i1 = i0 + 1 clamped
        const int hi = clampi(ax.i1[xhi - 1 - d.left] + 1, lo + 1, d.w0);
        const int npix = min(hi - lo, in_cap);
        const unsigned char* frame = frames + d.src_offset;
        const int sa = stage_span(lds_a, frame + ((size_t)y0 * d.w0 + lo) * 3, npix * 3);
        const int sb = stage_span(lds_b, frame + ((size_t)y1 * d.w0 + lo) * 3, npix * 3);
        __syncthreads();
        if (inside) {
            const int x = X - d.left;
            const int x0 = clampi(ax.i0[x] - lo, 0, npix - 1), x1 = clampi(ax.i1[x] - lo, 0, npix - 1);
            const double wx0 = ax.w0[x], wx1 = ax.w1[x];
            const bool outside = ay.outside[y] || ax.outside[x];        // rounding pushed the coordinate past the edge: cval = 0
            const unsigned char* p00 = lds_a + sa + x0 * 3; const unsigned char* p01 = lds_a + sa + x1 * 3;
            const unsigned char* p10 = lds_b + sb + x0 * 3; const unsigned char* p11 = lds_b + sb + x1 * 3;
            int v[3];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                double t = ((double)p00[c] * wy0) * wx0;                // (value * w_y) * w_x, summed in scipy's order
                t = t + ((double)p01[c] * wy0) * wx1;
                t = t + ((double)p10[c] * wy1) * wx0;
                t = t + ((double)p11[c] * wy1) * wx1;
                if (outside) t = 0.0;
                t = t < 0.0 ? 0.0 : (t > 255.0 ? 255.0 : t);
                v[c] = (int)floor(t + 0.5);
            }
            r = v[0]; g = v[1]; bl = v[2];
        }
    } else {
        __syncthreads();                                                // s_lut
    }
    if (X < cw) store_pixel(out, b, Y, X, ch, cw, channels_last, s_lut[r], s_lut[256 + g], s_lut[512 + bl]);
}

size_t preprocess_h_lds_bytes(int in_cap) { return (size_t)(kPreRowBytes - 16) + (size_t)in_cap * 3 + 32; }
size_t preprocess_zoom_lds_bytes(int in_cap) { return 3 * 256 * sizeof(float) + 2 * (size_t)(((size_t)in_cap * 3 + 32 + 15) & ~(size_t)15); }

hipError_t launch_preprocess(const opa_pre_image* images, int batch, const unsigned char* frames, const int32_t* tables,
                             unsigned char* ws, const float* lut, float* out, int ch, int cw, int precise, int channels_last,
                             unsigned fill, unsigned h_blocks, int in_cap, hipStream_t st) {
    const dim3 grid((cw + kPreCols - 1) / kPreCols, ch, batch);
    if (precise) {
        hipLaunchKernelGGL(preprocess_zoom_kernel, grid, dim3(kPreCols), preprocess_zoom_lds_bytes(in_cap), st,
                           images, frames, tables, lut, out, ch, cw, channels_last, fill, in_cap);
        prof_mark(st, "preprocess_zoom_kernel");
        return hipGetLastError();
    }
    if (h_blocks) {
        hipLaunchKernelGGL(preprocess_h_kernel, dim3(h_blocks, batch), dim3(kPreCols), preprocess_h_lds_bytes(in_cap), st,
                           images, frames, tables, ws, in_cap);
        prof_mark(st, "preprocess_h_kernel");
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(preprocess_v_kernel, grid, dim3(kPreCols), 0, st, images, frames, tables, ws, lut, out, ch, cw,
                       channels_last, fill);
    prof_mark(st, "preprocess_v_kernel");
    return hipGetLastError();
}

}  // namespace opa
