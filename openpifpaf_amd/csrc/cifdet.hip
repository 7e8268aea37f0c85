// CifDet: detection decoding on gfx950.
//
// Replaces reference CifDet::call (csrc/src/cifdet.cpp:24-80).  CifDetHr accumulation and
// CifDetSeeds are the CifHr / CifSeeds kernels in their DET variants (cifhr.hip,
// cifseeds.hip); this file holds the last step: walk the score-sorted seeds, skip seeds
// whose cell is occupied, mark a box of 0.1*min(w,h) around accepted ones, emit
// (category, score, box) until max_detections_before_nms.  One wavefront per image: 64
// seeds are tested against the occupancy map per step (ballot + ctz picks the next live
// one); the occupancy box is filled by the wave's lanes.
// Behind it, cifdet_nms_kernel: the IoU NMS, score filter and xywh conversion that the reference leaves to host Python
// (decoder/cifdet.py:60-91), so that only final detections leave the device.
#include <atomic>

#include "common.hpp"

namespace opa {

__global__ __launch_bounds__(64) void cifdet_collect_kernel(DetArgs a, DevParams p) {
    const int b = blockIdx.x, lane = lane_id();
    const int occ_h = a.occ_h, occ_w = a.occ_w;
    unsigned char* occ = a.occ + (size_t)b * a.F * occ_h * occ_w;
    int n_seeds = a.seed_count[b];
    if (n_seeds > a.seed_cap) n_seeds = a.seed_cap;
    const int32_t* seed_f = a.seed_f + (size_t)b * a.seed_cap;
    const float* seed_v = a.seed_vxywh + (size_t)b * a.seed_cap * 5;
    int64_t* cat = a.categories + (size_t)b * a.max_det;
    float* sc = a.scores + (size_t)b * a.max_det;
    float* bx = a.boxes + (size_t)b * a.max_det * 4;
    const double red = p.occupancy_reduction;

    int n = 0, pos = 0;
    while (pos < n_seeds && n < a.max_det) {
        const int i = pos + lane;
        bool live = false; int f = 0; float v = 0.f, x = 0.f, y = 0.f, w = 0.f, h = 0.f;
        if (i < n_seeds) {
            f = seed_f[i];
            const float* r = seed_v + (size_t)i * 5;
            v = r[0]; x = r[1]; y = r[2]; w = r[3]; h = r[4];
            double xd = (double)x, yd = (double)y;                       // occupancy.cpp:32-43
            if (red != 1.0) { xd /= red; yd /= red; }
            const long long xi = clampll(trunc_ll(xd), 0, occ_w - 1);
            const long long yi = clampll(trunc_ll(yd), 0, occ_h - 1);
            live = occ[((size_t)f * occ_h + yi) * occ_w + xi] == 0;      // cifdet.cpp:58
        }
        const unsigned long long mask = __ballot(live);
        if (mask == 0) { pos += kWave; continue; }
        const int l = __builtin_ctzll(mask);
        const int sf = __shfl(f, l);
        const float sv = __shfl(v, l), sx = __shfl(x, l), sy = __shfl(y, l), sw = __shfl(w, l), sh = __shfl(h, l);
        // occupancy.set(f, x, y, 0.1 * fmin(w, h)), cifdet.cpp:60 / occupancy.cpp:13-29
        double xd = (double)sx, yd = (double)sy, sigma = 0.1 * (double)fminf(sw, sh);
        if (red != 1.0) { xd /= red; yd /= red; sigma = fmax(p.occupancy_min_scale_reduced, sigma / red); }
        const int minx = (int)clampll(trunc_ll(xd - sigma), 0, occ_w - 1);
        const int miny = (int)clampll(trunc_ll(yd - sigma), 0, occ_h - 1);
        const int maxx = (int)clampll(trunc_ll(xd + sigma), minx + 1, occ_w);
        const int maxy = (int)clampll(trunc_ll(yd + sigma), miny + 1, occ_h);
        unsigned char* plane = occ + (size_t)sf * occ_h * occ_w;
        for (int yy = miny; yy < maxy; yy++)
            for (int xx = minx + lane; xx < maxx; xx += kWave) plane[(size_t)yy * occ_w + xx] = 1;
        if (lane == 0) {                                                  // cifdet.cpp:61-63
            cat[n] = sf + 1;
            sc[n] = sv;
            bx[4 * n + 0] = sx - 0.5f * sw; bx[4 * n + 1] = sy - 0.5f * sh;
            bx[4 * n + 2] = sx + 0.5f * sw; bx[4 * n + 3] = sy + 0.5f * sh;
        }
        n++;
        __threadfence_block();
        pos += l + 1;
    }
    if (lane == 0) a.counts[b] = n;
}

hipError_t launch_cifdet_collect(const DetArgs& a, const DevParams& p, hipStream_t st) {
    cifdet_collect_kernel<<<a.B, 64, 0, st>>>(a, p);
    prof_mark(st, "cifdet_collect_kernel");
    return hipGetLastError();
}

// ---- IoU NMS, score filter, xywh conversion ------------------------------------------------------------------------------
// What the reference does on the host after CifDet::call (decoder/cifdet.py:60-91: torchvision batched_nms, suppressed scores
// x 0.1, instance threshold, xywh) and decoder.CifDet._post restates in numpy; _post is the model this kernel is held to.
// One workgroup per image, thread i owns candidate i (the launch has at least max_det threads):
//   1. rank: the stable descending-score position of every candidate (np.argsort(-scores, kind='stable'): candidates with a
//      larger score plus earlier ones with an equal score); boxes and categories are laid out in that order in LDS;
//   2. pairs: one wave per (row r, 64 later candidates): a lane computes one IoU in double from the float32 corners the way
//      _nms_keep does, the wave's ballot is the row's 64-bit word of "r suppresses j" in LDS;
//   3. sweep, one wave: the live mask lives in the lanes' registers (lane w = candidates 64 w ...); the next live candidate is
//      kept and its row is cleared from the mask;
//   4. epilogue: score' = kept ? s : s * suppression, the instance threshold, w = x1 - x0, h = y1 - y0, and an ORDERED compaction
//      in candidate order (_post masks, it does not sort).
// No atomics, no global scratch, nothing allocated: the decode stays capturable.
// by_category: a pair of different categories never suppresses -- what the host's offset of category * (max + 1) on the
// coordinates means.  Negative corners are the one place where the two can differ: with a corner below -1 the host's shifted
// boxes of neighbouring categories can still overlap (torchvision's batched_nms has the same property); the test cases keep
// their coordinates non-negative.  (Without by_category _post evaluates the same formula in float32, threshold included; the
// two agree on every pair whose IoU is further from the threshold than float32 rounding of the formula, about 1e-6 * IoU.)
static __host__ __device__ inline size_t nms_rows_bytes(int max_det) {
    return ((size_t)max_det * ((max_det + 63) >> 6) * sizeof(unsigned long long) + 15) & ~(size_t)15;
}

size_t cifdet_nms_lds_bytes(int max_det) {
    return nms_rows_bytes(max_det) + (size_t)max_det * (sizeof(float4) + sizeof(long long)) +
           (size_t)((max_det + 63) >> 6) * sizeof(unsigned long long);
}

// np.maximum: a NaN operand is the result
__device__ __forceinline__ double np_max(double a, double b) { return (a > b || a != a) ? a : b; }
// the order of np.argsort(-scores, kind='stable'): descending, NaN last
__device__ __forceinline__ bool score_before(float a, float b) { return a > b || (b != b && a == a); }
__device__ __forceinline__ bool score_same(float a, float b) { return a == b || (a != a && b != b); }

__global__ __launch_bounds__(1024) void cifdet_nms_kernel(DetNmsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char nms_lds[];
    __shared__ int wave_sum[16];
    const int b = blockIdx.x, tid = threadIdx.x, lane = lane_id(), wave = tid >> 6, n_waves = blockDim.x >> 6;
    const int M = a.max_det;
    int n = a.counts[b];
    n = n < 0 ? 0 : (n > M ? M : n);
    if (n == 0) {                                                          // (uniform: no barrier is skipped by a part of the group)
        if (tid == 0) a.out_counts[b] = 0;
        return;
    }
    const int W = (n + 63) >> 6;                                           // 64-bit words per row of this image
    unsigned long long* rows = (unsigned long long*)nms_lds;              // [n][W]: bit j of row r = r suppresses j (j > r, rank order)
    float* rank_scores = (float*)nms_lds;                                  // [n], step 1 only (the rows are written after it)
    float4* sbox = (float4*)(nms_lds + nms_rows_bytes(M));                 // [M] boxes in rank order
    long long* scat = (long long*)(sbox + M);                              // [M] categories in rank order
    unsigned long long* kept = (unsigned long long*)(scat + M);            // [ceil(M / 64)] kept candidates, rank order

    float s = 0.f;
    float4 box = make_float4(0.f, 0.f, 0.f, 0.f);
    long long cat = 0;
    if (tid < n) {
        const size_t i = (size_t)b * M + tid;
        s = a.scores[i];
        cat = a.categories[i];
        box = make_float4(a.boxes[4 * i + 0], a.boxes[4 * i + 1], a.boxes[4 * i + 2], a.boxes[4 * i + 3]);
        rank_scores[tid] = s;
    }
    __syncthreads();

    // 1. rank
    int rank = 0;
    if (tid < n) {
        for (int j = 0; j < n; j++) {
            const float t = rank_scores[j];
            rank += (score_before(t, s) || (j < tid && score_same(t, s))) ? 1 : 0;
        }
        sbox[rank] = box;                                                  // (the ranks are a permutation of 0 .. n-1)
        scat[rank] = cat;
    }
    __syncthreads();

    // 2. pairs
    for (int t = wave; t < n * W; t += n_waves) {
        const int r = t / W, w = t - r * W;
        if (w < (r >> 6)) continue;                                        // (words in front of r's own are never read)
        const int j = (w << 6) + lane;
        bool sup = false;
        if (j > r && j < n && (!a.by_category || scat[r] == scat[j])) {
            const float4 p = sbox[r], q = sbox[j];
            const double area_p = np_max(0.0, (double)p.z - (double)p.x) * np_max(0.0, (double)p.w - (double)p.y);
            const double area_q = np_max(0.0, (double)q.z - (double)q.x) * np_max(0.0, (double)q.w - (double)q.y);
            const double xx0 = np_max((double)p.x, (double)q.x), yy0 = np_max((double)p.y, (double)q.y);
            const double xx1 = -np_max(-(double)p.z, -(double)q.z), yy1 = -np_max(-(double)p.w, -(double)q.w);   // np.minimum
            const double inter = np_max(0.0, xx1 - xx0) * np_max(0.0, yy1 - yy0);
            const double denom = np_max(area_p + area_q - inter, 1e-12);
            // (disjoint boxes, most pairs: 0 / denom without the division)
            const double iou = (inter == 0.0 && denom == denom) ? 0.0 : inter / denom;
            sup = iou > a.iou_threshold;
        }
        const unsigned long long word = __ballot(sup);
        if (lane == 0) rows[(size_t)r * W + w] = word;
    }
    __syncthreads();

    // 3. sweep
    if (wave == 0) {
        unsigned long long live = 0ull, mine = 0ull;
        if (lane < W) live = n - (lane << 6) >= 64 ? ~0ull : (1ull << (n - (lane << 6))) - 1ull;
        for (int w = 0; w < W; w++) {
            unsigned long long cur = __shfl(live, w);
            while (cur != 0ull) {
                const int bit = __builtin_ctzll(cur);
                const int r = (w << 6) + bit;
                if (lane == w) mine |= 1ull << bit;
                if (lane >= w && lane < W) live &= ~rows[(size_t)r * W + lane];
                cur = __shfl(live, w) & (bit == 63 ? 0ull : ~0ull << (bit + 1));
            }
        }
        if (lane < W) kept[lane] = mine;
    }
    __syncthreads();

    // 4. epilogue.  score' > instance_threshold is a FLOAT32 comparison: _post compares a float32 array with a Python float, which
    // numpy converts to float32 first; the suppression factor is a float32 for the same reason.
    bool pass = false;
    float s2 = s;
    if (tid < n) {
        const bool is_kept = (kept[rank >> 6] >> (rank & 63)) & 1ull;
        s2 = is_kept ? s : s * a.suppression;
        pass = s2 > a.instance_threshold;
    }
    const unsigned long long passed = __ballot(pass);
    if (lane == 0) wave_sum[wave] = __popcll(passed);
    __syncthreads();
    int base = 0, total = 0;
    for (int v = 0; v < n_waves; v++) {
        const int c = wave_sum[v];
        base += v < wave ? c : 0;
        total += c;
    }
    if (pass) {
        const size_t o = (size_t)b * M + base + __popcll(passed & ((1ull << lane) - 1ull));
        a.out_categories[o] = cat;
        a.out_scores[o] = s2;
        a.out_boxes[4 * o + 0] = box.x; a.out_boxes[4 * o + 1] = box.y;
        a.out_boxes[4 * o + 2] = box.z - box.x; a.out_boxes[4 * o + 3] = box.w - box.y;
    }
    if (tid == 0) a.out_counts[b] = total;
}

hipError_t launch_cifdet_nms(const DetNmsArgs& a, hipStream_t st) {
    const size_t lds = cifdet_nms_lds_bytes(a.max_det);
    if (lds > 64 * 1024) {                                                 // above the default limit: allowed once per device (that
                                                                           // first call must not be inside a stream capture: header)
        static std::atomic<unsigned long long> done{0ull};
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        const unsigned long long bit = dev >= 0 && dev < 64 ? 1ull << dev : 0ull;
        if (!(done.load(std::memory_order_relaxed) & bit)) {
            e = hipFuncSetAttribute((const void*)cifdet_nms_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)cifdet_nms_lds_bytes(kDetNmsMax));
            if (e != hipSuccess) return e;
            done.fetch_or(bit, std::memory_order_relaxed);
        }
    }
    cifdet_nms_kernel<<<a.B, a.max_det <= 256 ? 256 : 1024, lds, st>>>(a);
    prof_mark(st, "cifdet_nms_kernel");
    return hipGetLastError();
}

}  // namespace opa
