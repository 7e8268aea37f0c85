// C ABI of the trunk's producer side (include/openpifpaf_amd.h): the argument checks that stand between a caller's pointer and a
// kernel, for the GEMM, convolution, pooling, squeeze-excite, interleave and head-epilogue launchers, and image preprocessing.
// Every entry point reads top to bottom: refusals, the empty call's return, the launch.
//
// The checks are UNEVEN between entry points, and tests/golden/capi_refusals.json pins them as they are: every status, every
// message byte for byte, and the order of the checks (which message wins when two arguments are bad).  Making them even is an
// ABI decision of its own.  What differs:
//   null / alignment   opa_gemm_bias_act_bf16 and opa_gemm_pro_bias_act_bf16 do not test bias_dev's alignment, the float32 GEMMs do.
//                      The Winograd entry points, opa_dwconv_*, opa_gconv3x3_* and opa_maxpool3x3_* accept a null bias.
//                      opa_fire_expand_f32x3 tests all four pointers.
//                      opa_dwconv_*, opa_channel_interleave and opa_head_epilogue test no alignment at all.  The unit mode asks
//                      8 bytes of a_dev, partner_dev and residual_dev, 16 of the rest (opa_gemm_unit_actp_bf16 / _f16: 4 and 16): one
//                      list of checks, unit_refusal, for its five entry points.  A null pointer is aligned everywhere.
//   act_param          one rule wherever an entry point takes it (bad_act_param); opa_dwconv_actp refuses code 3 before it.
//   empty calls        m == 0 (opa_bias_act: rows == 0) is OPA_OK for the GEMMs; an empty batch, h or w is OPA_OK for
//                      opa_conv3x3_dilated_f32x3, opa_maxpool3x3_bias_act, opa_maxpool3x3_ceil_bias_act, opa_fire_expand_f32x3 and
//                      opa_gconv3x3_bias_act_f32, after every check that does not need a size (all but the first test their grid
//                      only behind it); an empty batch alone (h and w must be positive) for opa_stem3x3_actp, after every check
//                      but those of the sizes' products, and for opa_groupnorm_actp (pixels, channels and groups must be positive),
//                      after every check of its arguments but the limits and the workspace; an empty batch, h or w for
//                      opa_conv3x3_act_bf16, opa_gconv3x3_act_bf16, opa_stem7x7_act_bf16 and opa_gemm2_bias_act_bf16 (and their _f16 twins), after every check
//                      but the grid's; an empty batch alone (the other sizes must be positive) for opa_head_conv_fields_bf16 / _f16,
//                      after every check but the grid's.
//                      opa_conv3x3_f32x3, opa_gemm2_bias_act_f32x3, opa_conv_rows_*, Winograd, dwconv, squeeze-excite, interleave and the head epilogue refuse empties.
//   last error         a call that succeeds leaves opa_last_error's text as it was.
//   marks              the entry points that pass a kernel's name to Entry::launched mark the profile here; the launchers of the
//                      others (dwconv, gconv, se, group norm, interleave, head epilogue, preprocessing) mark it themselves.
//   Winograd variants  opa_conv3x3_winograd_f32 lets the variants 11-18 past its checks and ..._f32x3 21-23 (timing experiments of
//                      OPA_WINO_DIAG builds); the production launcher answers hipErrorInvalidValue before it touches the device:
//                      OPA_ERR_HIP, "winograd_f23: invalid argument".
#include "capi_internal.hpp"

#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <string>

using namespace opa;

namespace {
struct Entry {                              // one C entry point: its name in every message, its stream
    const char* fn; hipStream_t st;
    Entry(const char* fn_, void* stream) : fn(fn_), st((hipStream_t)stream) {}
    int refuse(int code, const std::string& what) const { return fail(code, std::string(fn) + ": " + what); }
    int refuse(const char* what) const { return refuse(OPA_ERR_INVALID_ARGUMENT, what); }
    // the launcher's answer: fail_hip(where), or the profile's mark (where the launcher does not set it itself) and OPA_OK
    int launched(hipError_t e, const char* where, const char* mark = nullptr) const {
        if (e != hipSuccess) return fail_hip(e, where);
        if (mark) prof_mark(st, mark);
        return OPA_OK;
    }
};

bool misaligned(uintptr_t mask, std::initializer_list<const void*> pointers) {      // (null passes)
    uintptr_t bits = 0;
    for (const void* p : pointers) bits |= (uintptr_t)p;
    return (bits & mask) != 0;
}

bool bad_terms(int32_t terms) { return terms != 6 && terms != 9; }

// The parameter of an activation code: 3 (LeakyReLU) reads it as the slope, 4 (clipped ReLU) as the cap.  -> what is wrong with it, or null
const char* bad_act_param(int32_t act, float act_param) {
    if (!std::isfinite(act_param)) return "act_param must be finite";
    if (act == 3 && act_param < 0.0f) return "act_param must not be negative with act 3 (the LeakyReLU's slope)";
    if (act == 4 && act_param <= 0.0f) return "act_param must be positive with act 4 (the clipped ReLU's cap)";
    return nullptr;
}
}  // namespace

extern "C" {

int opa_bias_act(void* x_dev, const void* bias_dev, const void* residual_dev, int64_t rows, int32_t channels,
                 int32_t dtype, int32_t relu, void* stream) {
    const Entry E("opa_bias_act", stream);
    if (!x_dev || !bias_dev || rows < 0 || channels <= 0 || dtype < 0 || dtype > 2) return E.refuse("bad arguments");
    if (channels % (dtype == 0 ? 4 : 8) != 0 || misaligned(15, {x_dev, bias_dev, residual_dev}))
        return E.refuse("channels must fill 16-byte vectors and pointers be 16-B aligned");
    if (rows == 0) return OPA_OK;
    return E.launched(launch_bias_act(x_dev, bias_dev, residual_dev, rows, channels, dtype, relu, E.st), "bias_act", "bias_act_kernel");
}

// opa_gemm_bias_act_bf16 and opa_gemm_pro_bias_act_bf16 (`pro`: a_bias_dev is required; without, it is null), and their float16 twins
// (`dtype` 1: every operand float16, the kernel on the f16 MFMA)
static int gemm_bf16(const char* fn, int dtype, bool pro, const void* a_dev, const void* a_bias_dev, const void* w_dev, const void* bias_dev,
                     const void* residual_dev, void* out_dev, int64_t m, int32_t n, int32_t k, int32_t relu, void* stream) {
    const Entry E(fn, stream);
    if (!a_dev || (pro && !a_bias_dev) || !w_dev || !bias_dev || !out_dev || m < 0 || n <= 0 || k <= 0 || m > 0x7fffffffll)
        return E.refuse("bad arguments");
    if (k % 64 != 0 || n % 64 != 0) return E.refuse("K and N must be multiples of 64");
    if (misaligned(15, {a_dev, a_bias_dev, w_dev, out_dev, residual_dev})) return E.refuse("pointers must be 16-B aligned");
    if (m == 0) return OPA_OK;
    const hipError_t e = launch_gemm_bias_act(a_dev, w_dev, bias_dev, residual_dev, out_dev, (int)m, n, k, relu, E.st, a_bias_dev, dtype);
    if (dtype == 1)
        return E.launched(e, pro ? "gemm_pro_bias_act_f16" : "gemm_bias_act_f16", pro ? "gemm_pro_bias_act_f16_kernel" : "gemm_bias_act_f16_kernel");
    return E.launched(e, pro ? "gemm_pro_bias_act" : "gemm_bias_act", pro ? "gemm_pro_bias_act_kernel" : "gemm_bias_act_kernel");
}

int opa_gemm_bias_act_bf16(const void* a_dev, const void* w_dev, const void* bias_dev, const void* residual_dev,
                           void* out_dev, int64_t m, int32_t n, int32_t k, int32_t relu, void* stream) {
    return gemm_bf16("opa_gemm_bias_act_bf16", 2, false, a_dev, nullptr, w_dev, bias_dev, residual_dev, out_dev, m, n, k, relu, stream);
}

int opa_gemm_pro_bias_act_bf16(const void* a_dev, const void* a_bias_dev, const void* w_dev, const void* bias_dev,
                               const void* residual_dev, void* out_dev, int64_t m, int32_t n, int32_t k,
                               int32_t relu, void* stream) {
    return gemm_bf16("opa_gemm_pro_bias_act_bf16", 2, true, a_dev, a_bias_dev, w_dev, bias_dev, residual_dev, out_dev, m, n, k, relu, stream);
}

int opa_gemm_bias_act_f16(const void* a_dev, const void* w_dev, const void* bias_dev, const void* residual_dev,
                          void* out_dev, int64_t m, int32_t n, int32_t k, int32_t relu, void* stream) {
    return gemm_bf16("opa_gemm_bias_act_f16", 1, false, a_dev, nullptr, w_dev, bias_dev, residual_dev, out_dev, m, n, k, relu, stream);
}

int opa_gemm_pro_bias_act_f16(const void* a_dev, const void* a_bias_dev, const void* w_dev, const void* bias_dev,
                              const void* residual_dev, void* out_dev, int64_t m, int32_t n, int32_t k,
                              int32_t relu, void* stream) {
    return gemm_bf16("opa_gemm_pro_bias_act_f16", 1, true, a_dev, a_bias_dev, w_dev, bias_dev, residual_dev, out_dev, m, n, k, relu, stream);
}

int opa_gemm_bias_act_f32(const float* a_dev, const float* a_bias_dev, const float* w_dev, const float* bias_dev,
                          const float* residual_dev, float* out_dev, int64_t m, int32_t n, int32_t k,
                          int32_t relu, void* stream) {
    const Entry E("opa_gemm_bias_act_f32", stream);
    if (!a_dev || !w_dev || !bias_dev || !out_dev || m < 0 || n <= 0 || k <= 0 || m > 0x7fffffffll) return E.refuse("bad arguments");
    if (k % 32 != 0 || n % 64 != 0) return E.refuse("K must be a multiple of 32 and N of 64");
    if (misaligned(15, {a_dev, a_bias_dev, w_dev, out_dev, residual_dev, bias_dev})) return E.refuse("pointers must be 16-B aligned");
    if (m == 0) return OPA_OK;
    return E.launched(launch_gemm_f32_bias_act(a_dev, w_dev, bias_dev, residual_dev, out_dev, (int)m, n, k, relu, E.st, a_bias_dev),
                      "gemm_f32_bias_act", a_bias_dev ? "gemm_f32_pro_bias_act_kernel" : "gemm_f32_bias_act_kernel");
}

int opa_gemm_bias_act_f32x3(const float* a_dev, const float* a_bias_dev, const void* w3_dev, const float* bias_dev,
                            const float* residual_dev, float* out_dev, int64_t m, int32_t n, int32_t k,
                            int32_t relu, int32_t terms, void* stream) {
    const Entry E("opa_gemm_bias_act_f32x3", stream);
    if (!a_dev || !w3_dev || !bias_dev || !out_dev || m < 0 || n <= 0 || k <= 0 || m > 0x7fffffffll || bad_terms(terms))
        return E.refuse("bad arguments");
    if (k % 64 != 0 || n % 64 != 0) return E.refuse("K and N must be multiples of 64");
    if (misaligned(15, {a_dev, a_bias_dev, w3_dev, out_dev, residual_dev, bias_dev})) return E.refuse("pointers must be 16-B aligned");
    if (m == 0) return OPA_OK;
    return E.launched(launch_gemm_f32x3_bias_act(a_dev, (const unsigned short*)w3_dev, bias_dev, residual_dev, out_dev, (int)m, n, k, relu,
                                                 terms, E.st, a_bias_dev), "gemm_f32x3_bias_act", "gemm_f32x3_bias_act_kernel");
}

int opa_gemm2_bias_act_f32x3(const float* a1_dev, int32_t k1, const float* a2_dev, int32_t k2, int32_t batch, int32_t h_in,
                             int32_t w_in, int32_t stride, const float* a_bias_dev, const void* w3cat_dev, const float* bias_dev,
                             float* out_dev, int32_t n, int32_t relu, int32_t terms, void* stream) {
    const Entry E("opa_gemm2_bias_act_f32x3", stream);
    if (!a1_dev || !a2_dev || !w3cat_dev || !bias_dev || !out_dev || batch <= 0 || h_in <= 0 || w_in <= 0 || stride < 1 || n <= 0 ||
        k1 <= 0 || k2 <= 0 || bad_terms(terms))
        return E.refuse("bad arguments");
    if (k1 % 32 != 0 || (k1 + k2) % 64 != 0 || k2 % 4 != 0 || n % 64 != 0) return E.refuse("k1 % 32, (k1 + k2) % 64, k2 % 4, N % 64 must be 0");
    if (misaligned(15, {a1_dev, a2_dev, a_bias_dev, w3cat_dev, out_dev, bias_dev})) return E.refuse("pointers must be 16-B aligned");
    const long long ho = (h_in - 1) / stride + 1, wo = (w_in - 1) / stride + 1;
    if ((long long)batch * ho * wo > 0x7fffffffll || (long long)batch * h_in * w_in > 0x7fffffffll) return E.refuse("too many pixels");
    return E.launched(launch_gemm2_f32x3_bias_act(a1_dev, k1, a2_dev, k2, batch, h_in, w_in, stride, (const unsigned short*)w3cat_dev,
                                                  bias_dev, out_dev, n, relu, terms, E.st, a_bias_dev),
                      "gemm2_f32x3_bias_act", "gemm2_f32x3_bias_act_kernel");
}

int opa_conv_rows_f32x3(const float* x_dev, const void* w3_dev, const float* bias_dev, float* out_dev, int32_t batch, int32_t hp,
                        int32_t wp, int32_t pix, int32_t ho, int32_t wo, int32_t stride, int32_t ntaps, int32_t tap_floats,
                        int32_t c_out, int32_t relu, int32_t terms, void* stream) {
    const Entry E("opa_conv_rows_f32x3", stream);
    if (!x_dev || !w3_dev || !bias_dev || !out_dev || batch <= 0 || hp <= 0 || wp <= 0 || pix <= 0 || ho <= 0 || wo <= 0 || stride < 1 ||
        ntaps < 1 || ntaps > 32 || tap_floats <= 0 || c_out <= 0 || bad_terms(terms))
        return E.refuse("bad arguments");
    if (tap_floats % 32 != 0 || (ntaps * tap_floats) % 64 != 0 || c_out % 64 != 0 || pix % 4 != 0)
        return E.refuse("tap_floats % 32, ntaps * tap_floats % 64, c_out % 64, pix % 4 must be 0");
    if (misaligned(15, {x_dev, w3_dev, out_dev, bias_dev})) return E.refuse("pointers must be 16-B aligned");
    // every tap of the last output pixel inside the tensor
    if ((long long)(ho - 1) * stride + ntaps > hp || ((long long)(wo - 1) * stride) * pix + tap_floats > (long long)wp * pix ||
        (long long)batch * hp * wp * pix * 4 > 0x7fffffffll || (long long)batch * ho * wo > 0x7fffffffll)
        return E.refuse("the taps leave the (padded) input, or it is 2 GB or more");
    return E.launched(launch_convrows_f32x3(x_dev, batch, hp, wp, pix, ho, wo, stride, ntaps, tap_floats, (const unsigned short*)w3_dev,
                                            bias_dev, out_dev, c_out, relu, terms, E.st), "conv_rows_f32x3", "conv_rows_f32x3_kernel");
}

// opa_conv3x3_f32x3 and opa_conv3x3_dilated_f32x3
static int conv3x3_f32x3(const char* fn, const float* x_dev, const void* w3_dev, const float* bias_dev, float* out_dev, int32_t batch,
                         int32_t h_in, int32_t w_in, int32_t c_in, int32_t c_out, int32_t stride, int32_t dilation, int32_t relu,
                         int32_t terms, void* stream) {
    const Entry E(fn, stream);
    if (!x_dev || !w3_dev || !bias_dev || !out_dev || batch < 0 || h_in < 0 || w_in < 0 || stride < 1 || dilation < 1 || c_in <= 0 ||
        c_out <= 0 || bad_terms(terms))
        return E.refuse("bad arguments");
    if (c_in % 64 != 0 || c_out % 64 != 0) return E.refuse("c_in and c_out must be multiples of 64");
    if (misaligned(15, {x_dev, w3_dev, out_dev, bias_dev})) return E.refuse("pointers must be 16-B aligned");
    // (the buffer the kernel reads through begins dilation * (w_in + 1) pixels before the tensor: its size is a 32-bit count of bytes)
    // (in double: exact up to 2^53, and no product of four 32-bit arguments overflows it)
    if (((double)batch * h_in * w_in + (double)dilation * ((double)w_in + 1.0)) * c_in * 4.0 >= 2147483648.0)
        return E.refuse("the activation must be smaller than 2 GB");
    if (batch == 0 || h_in == 0 || w_in == 0) return OPA_OK;
    return E.launched(launch_conv3x3_f32x3(x_dev, batch, h_in, w_in, c_in, stride, dilation, (const unsigned short*)w3_dev, bias_dev,
                                           out_dev, c_out, relu, terms, E.st), "conv3x3_f32x3", "conv3x3_f32x3_kernel");
}

int opa_conv3x3_f32x3(const float* x_dev, const void* w3_dev, const float* bias_dev, float* out_dev, int32_t batch, int32_t h_in,
                      int32_t w_in, int32_t c_in, int32_t c_out, int32_t stride, int32_t relu, int32_t terms, void* stream) {
    if (batch <= 0 || h_in <= 0 || w_in <= 0)        // (this entry point has always refused an empty tensor)
        return Entry("opa_conv3x3_f32x3", stream).refuse("bad arguments");
    return conv3x3_f32x3("opa_conv3x3_f32x3", x_dev, w3_dev, bias_dev, out_dev, batch, h_in, w_in, c_in, c_out, stride, 1, relu, terms, stream);
}

int opa_conv3x3_dilated_f32x3(const float* x_dev, const void* w3_dev, const float* bias_dev, float* out_dev, int32_t batch, int32_t h_in,
                              int32_t w_in, int32_t c_in, int32_t c_out, int32_t stride, int32_t dilation, int32_t relu, int32_t terms,
                              void* stream) {
    return conv3x3_f32x3("opa_conv3x3_dilated_f32x3", x_dev, w3_dev, bias_dev, out_dev, batch, h_in, w_in, c_in, c_out, stride, dilation,
                         relu, terms, stream);
}

// opa_maxpool3x3_bias_act and opa_maxpool3x3_ceil_bias_act (`ceil_mode`: torch's ceil_mode=True output sizes, SqueezeNet's pools)
static int maxpool3x3(const char* fn, const char* where, int ceil_mode, const void* x_dev, const void* bias_dev, void* out_dev, int32_t dtype,
                      int32_t batch, int32_t h, int32_t w, int32_t c, int32_t stride, int32_t relu, void* stream) {
    const Entry E(fn, stream);
    if (!x_dev || !out_dev || batch < 0 || h < 0 || w < 0 || c <= 0) return E.refuse("bad arguments");
    if (dtype != 0 && dtype != 2) return E.refuse("dtype must be 0 (float32) or 2 (bfloat16)");
    if (stride != 2) return E.refuse("the stride must be 2");
    if (c % 8 != 0) return E.refuse("c must be a multiple of 8");
    if (misaligned(15, {x_dev, out_dev, bias_dev})) return E.refuse("pointers must be 16-B aligned");
    // 32-bit vector indices in the kernel, one thread per output vector
    if ((double)batch * h * w * c * (dtype == 0 ? 4.0 : 2.0) >= 2147483648.0)
        return E.refuse("the activation must be smaller than 2 GB (32-bit offsets)");
    if (batch == 0 || h == 0 || w == 0) return OPA_OK;
    if (maxpool3x3_blocks(batch, h, w, c, ceil_mode) > 0x7fffffffll) return E.refuse("too many output vectors for grid.x");
    return E.launched(launch_maxpool3x3(x_dev, bias_dev, out_dev, dtype, batch, h, w, c, relu, E.st, ceil_mode), where, "maxpool3x3s2_kernel");
}

int opa_maxpool3x3_bias_act(const void* x_dev, const void* bias_dev, void* out_dev, int32_t dtype, int32_t batch, int32_t h, int32_t w,
                            int32_t c, int32_t stride, int32_t relu, void* stream) {
    return maxpool3x3("opa_maxpool3x3_bias_act", "maxpool3x3_bias_act", 0, x_dev, bias_dev, out_dev, dtype, batch, h, w, c, stride, relu, stream);
}

int opa_maxpool3x3_ceil_bias_act(const void* x_dev, const void* bias_dev, void* out_dev, int32_t dtype, int32_t batch, int32_t h, int32_t w,
                                 int32_t c, int32_t stride, int32_t relu, void* stream) {
    return maxpool3x3("opa_maxpool3x3_ceil_bias_act", "maxpool3x3_ceil_bias_act", 1, x_dev, bias_dev, out_dev, dtype, batch, h, w, c, stride, relu,
                      stream);
}

int opa_fire_expand_f32x3(const float* h_dev, const void* w_dev, const float* bias_dev, float* out_dev, int32_t batch, int32_t h, int32_t w,
                          int32_t c_squeeze, int32_t c_e1, int32_t c_e3, int32_t terms, void* stream) {
    const Entry E("opa_fire_expand_f32x3", stream);
    if (!h_dev || !w_dev || !bias_dev || !out_dev || batch < 0 || h < 0 || w < 0 || c_squeeze <= 0 || c_e1 <= 0 || c_e3 <= 0 || bad_terms(terms))
        return E.refuse("bad arguments");
    if (c_squeeze % 16 != 0 || c_squeeze > 64) return E.refuse("c_squeeze must be 16, 32, 48 or 64");
    if (c_e1 % 64 != 0 || c_e3 % 64 != 0) return E.refuse("c_e1 and c_e3 must be multiples of 64");
    if (misaligned(15, {h_dev, w_dev, bias_dev, out_dev})) return E.refuse("pointers must be 16-B aligned");
    // 32-bit byte offsets into both tensors (in double: no product of 32-bit arguments overflows it)
    if ((double)batch * h * w * ((double)c_e1 + c_e3) * 4.0 >= 2147483648.0 || (double)batch * h * w * c_squeeze * 4.0 >= 2147483648.0)
        return E.refuse("the tensors must be smaller than 2 GB (32-bit offsets)");
    if (batch == 0 || h == 0 || w == 0) return OPA_OK;
    if (fire_expand_workgroups(batch, h, w) > 0x7fffffffll) return E.refuse("too many pixel tiles for grid.x");
    return E.launched(launch_fire_expand(h_dev, (const unsigned short*)w_dev, bias_dev, out_dev, batch, h, w, c_squeeze, c_e1, c_e3, terms,
                                         E.st), "fire_expand_f32x3", "fire_expand_kernel");
}

// The checks of the unit mode's five entry points -> what is wrong, or null.  What differs between them: `act_max`; `mask`, the alignment
// of a_dev / partner_dev / residual_dev (8 bytes, 4 for the 16-bit types), and `unaligned`, the message that names it; `terms`, null where the
// entry point has none.  The pitches count elements.  act 3 (LeakyReLU) and 4 (clipped ReLU) read act_param.
static const char* unit_refusal(int32_t act_max, uintptr_t mask, const char* unaligned, const int32_t* terms, const void* a_dev, int64_t a_pitch,
                                const void* w_dev, const float* bias_dev, const void* partner_dev, int64_t partner_pitch, const void* residual_dev,
                                int64_t residual_pitch, const void* out_dev, int64_t m, int32_t n, int32_t k, int32_t act, float act_param) {
    if (!a_dev || !w_dev || !bias_dev || !out_dev || m < 0 || n <= 0 || k <= 0 || m > 0x7fffffffll || (terms && bad_terms(*terms)) || act < 0 ||
        act > act_max)
        return "bad arguments";
    if (const char* why = bad_act_param(act, act_param)) return why;
    if (partner_dev && residual_dev) return "a residual cannot be combined with a partner";
    if (residual_dev && act > 2) return "a residual cannot be combined with act 3 or 4";
    if (n % 2 != 0 || k % 2 != 0) return "K and N must be even";
    // (a tile's 128 rows are addressed with 32-bit byte offsets: 2^21 elements per row leave room)
    if (a_pitch < k || a_pitch % 2 != 0 || a_pitch > (1 << 21) ||
        (partner_dev && (partner_pitch < n || partner_pitch % 2 != 0 || partner_pitch > 0x7fffffffll)) ||
        (residual_dev && (residual_pitch < n || residual_pitch % 2 != 0 || residual_pitch > 0x7fffffffll)))
        return "a row pitch is shorter than its row, odd, or too long";
    return misaligned(mask, {a_dev, partner_dev, residual_dev}) || misaligned(15, {w_dev, out_dev, bias_dev}) ? unaligned : nullptr;
}

// opa_gemm_unit_actp_f32x3; opa_gemm_unit_act_f32x3 as its call with act 0 .. 2 (`act_max`) and no parameter, and
// opa_gemm_unit_bias_act_f32x3 as that one's call without a residual and with act 0 / 1 (`eight`: the pointers the alignment message names, `where`: the launch in a HIP error's text)
static int gemm_unit_f32x3(const char* fn, const char* eight, const char* where, int32_t act_max, float act_param, const float* a_dev,
                           int64_t a_pitch, const void* w3_dev, const float* bias_dev, const float* partner_dev, int64_t partner_pitch,
                           const float* residual_dev, int64_t residual_pitch, float* out_dev, int64_t m, int32_t n, int32_t k, int32_t act,
                           int32_t terms, void* stream) {
    const Entry E(fn, stream);
    const std::string unaligned = std::string(eight) + " must be 8-B, w3_dev / bias_dev / out_dev 16-B aligned";
    if (const char* why = unit_refusal(act_max, 7, unaligned.c_str(), &terms, a_dev, a_pitch, w3_dev, bias_dev, partner_dev, partner_pitch, residual_dev,
                                       residual_pitch, out_dev, m, n, k, act, act_param))
        return E.refuse(why);
    if (m == 0) return OPA_OK;
    return E.launched(launch_gemm_unit_act_f32x3(a_dev, (int)a_pitch, (const unsigned short*)w3_dev, bias_dev, partner_dev,
                                                 partner_dev ? (int)partner_pitch : 0, residual_dev, residual_dev ? (int)residual_pitch : 0,
                                                 out_dev, (int)m, n, k, act, terms, E.st, act_param), where, "gemm_unit_f32x3_kernel");
}

int opa_gemm_unit_bias_act_f32x3(const float* a_dev, int64_t a_pitch, const void* w3_dev, const float* bias_dev,
                                 const float* partner_dev, int64_t partner_pitch, float* out_dev,
                                 int64_t m, int32_t n, int32_t k, int32_t relu, int32_t terms, void* stream) {
    return gemm_unit_f32x3("opa_gemm_unit_bias_act_f32x3", "a_dev / partner_dev", "gemm_unit_f32x3", 2, 0.0f, a_dev, a_pitch, w3_dev, bias_dev,
                           partner_dev, partner_pitch, nullptr, 0, out_dev, m, n, k, relu ? 1 : 0, terms, stream);
}

int opa_gemm_unit_act_f32x3(const float* a_dev, int64_t a_pitch, const void* w3_dev, const float* bias_dev,
                            const float* partner_dev, int64_t partner_pitch, const float* residual_dev, int64_t residual_pitch,
                            float* out_dev, int64_t m, int32_t n, int32_t k, int32_t act, int32_t terms, void* stream) {
    return gemm_unit_f32x3("opa_gemm_unit_act_f32x3", "a_dev / partner_dev / residual_dev", "gemm_unit_act_f32x3", 2, 0.0f, a_dev, a_pitch, w3_dev, bias_dev,
                           partner_dev, partner_pitch, residual_dev, residual_pitch, out_dev, m, n, k, act, terms, stream);
}

int opa_gemm_unit_actp_f32x3(const float* a_dev, int64_t a_pitch, const void* w3_dev, const float* bias_dev,
                             const float* partner_dev, int64_t partner_pitch, const float* residual_dev, int64_t residual_pitch,
                             float* out_dev, int64_t m, int32_t n, int32_t k, int32_t act, float act_param, int32_t terms, void* stream) {
    return gemm_unit_f32x3("opa_gemm_unit_actp_f32x3", "a_dev / partner_dev / residual_dev", "gemm_unit_actp_f32x3", 4, act_param, a_dev, a_pitch, w3_dev,
                           bias_dev, partner_dev, partner_pitch, residual_dev, residual_pitch, out_dev, m, n, k, act, terms, stream);
}

// the unit mode in 16 bits (csrc/gemm_unit_bf16.hip): no terms.  opa_gemm_unit_actp_bf16 and its float16 twin (`dtype` 1: a, w, the
// partner, the residual and out float16, the kernel on the f16 MFMA)
static int gemm_unit_16(const char* fn, int dtype, const void* a_dev, int64_t a_pitch, const void* w_dev, const float* bias_dev,
                        const void* partner_dev, int64_t partner_pitch, const void* residual_dev, int64_t residual_pitch,
                        void* out_dev, int64_t m, int32_t n, int32_t k, int32_t act, float act_param, void* stream) {
    const Entry E(fn, stream);
    if (const char* why = unit_refusal(4, 3, "a_dev / partner_dev / residual_dev must be 4-B, w_dev / bias_dev / out_dev 16-B aligned", nullptr,
                                       a_dev, a_pitch, w_dev, bias_dev, partner_dev, partner_pitch, residual_dev, residual_pitch, out_dev, m, n, k,
                                       act, act_param))
        return E.refuse(why);
    if (m == 0) return OPA_OK;
    return E.launched(launch_gemm_unit_act_bf16(a_dev, a_pitch, w_dev, bias_dev, partner_dev, partner_dev ? partner_pitch : 0, residual_dev,
                                                residual_dev ? residual_pitch : 0, out_dev, (int)m, n, k, act, act_param, E.st, dtype),
                      dtype == 1 ? "gemm_unit_actp_f16" : "gemm_unit_actp_bf16", dtype == 1 ? "gemm_unit_f16_kernel" : "gemm_unit_bf16_kernel");
}

int opa_gemm_unit_actp_bf16(const void* a_dev, int64_t a_pitch, const void* w_dev, const float* bias_dev,
                            const void* partner_dev, int64_t partner_pitch, const void* residual_dev, int64_t residual_pitch,
                            void* out_dev, int64_t m, int32_t n, int32_t k, int32_t act, float act_param, void* stream) {
    return gemm_unit_16("opa_gemm_unit_actp_bf16", 2, a_dev, a_pitch, w_dev, bias_dev, partner_dev, partner_pitch, residual_dev, residual_pitch,
                        out_dev, m, n, k, act, act_param, stream);
}

int opa_gemm_unit_actp_f16(const void* a_dev, int64_t a_pitch, const void* w_dev, const float* bias_dev,
                           const void* partner_dev, int64_t partner_pitch, const void* residual_dev, int64_t residual_pitch,
                           void* out_dev, int64_t m, int32_t n, int32_t k, int32_t act, float act_param, void* stream) {
    return gemm_unit_16("opa_gemm_unit_actp_f16", 1, a_dev, a_pitch, w_dev, bias_dev, partner_dev, partner_pitch, residual_dev, residual_pitch,
                        out_dev, m, n, k, act, act_param, stream);
}

// the 3x3 convolutions of a bfloat16 ResNet as an implicit GEMM on the bf16 MFMA (csrc/conv3x3_bf16.hip): one message per check.
// opa_conv3x3_act_bf16 and its float16 twin (`dtype` 1: x, w, residual and out float16, the kernel on the f16 MFMA)
static int conv3x3_16(const char* fn, int dtype, const void* x_dev, const void* w_dev, const float* bias_dev, const void* residual_dev,
                      void* out_dev, int32_t batch, int32_t h_in, int32_t w_in, int32_t c_in, int32_t c_out,
                      int32_t stride, int32_t dilation, int32_t relu, void* stream) {
    const Entry E(fn, stream);
    if (!x_dev || !w_dev || !out_dev) return E.refuse("x_dev, w_dev and out_dev must not be NULL");
    if (misaligned(15, {x_dev, w_dev, bias_dev, residual_dev, out_dev})) return E.refuse("pointers must be 16-B aligned");
    if (batch < 0 || h_in < 0 || w_in < 0) return E.refuse("negative batch, h_in or w_in");
    if (c_in <= 0 || c_out <= 0 || c_in % 64 != 0 || c_out % 64 != 0) return E.refuse("c_in and c_out must be positive multiples of 64");
    if (stride != 1 && stride != 2) return E.refuse("stride must be 1 or 2");
    if (dilation != 1 && dilation != 2 && dilation != 4) return E.refuse("dilation must be 1, 2 or 4");
    if (dilation > 1 && stride != 1) return E.refuse("a dilation above 1 needs stride 1");
    // 32-bit element offsets into both tensors (in double: exact up to 2^53, and no product of these arguments overflows it)
    const double ho = h_in > 0 ? (h_in - 1) / stride + 1 : 0, wo = w_in > 0 ? (w_in - 1) / stride + 1 : 0;
    if ((double)batch * h_in * w_in * c_in >= 2147483648.0) return E.refuse("x must hold fewer than 2^31 elements (32-bit offsets)");
    if ((double)batch * ho * wo * c_out >= 2147483648.0) return E.refuse("out must hold fewer than 2^31 elements (32-bit offsets)");
    if (batch == 0 || h_in == 0 || w_in == 0) return OPA_OK;
    // (grid.x; with out below 2^31 elements of at least 64 channels it holds today: it guards the launch should a limit above move)
    if (conv3x3_bf16_workgroups(batch, h_in, w_in, c_out, stride) > 0x7fffffffll) return E.refuse("too many tiles for grid.x");
    return E.launched(launch_conv3x3_bf16(x_dev, w_dev, bias_dev, residual_dev, out_dev, batch, h_in, w_in, c_in, c_out, stride, dilation,
                                          relu, E.st, dtype), dtype == 1 ? "conv3x3_act_f16" : "conv3x3_act_bf16",
                      dtype == 1 ? "conv3x3_f16_kernel" : "conv3x3_bf16_kernel");
}

int opa_conv3x3_act_bf16(const void* x_dev, const void* w_dev, const float* bias_dev, const void* residual_dev, void* out_dev,
                         int32_t batch, int32_t h_in, int32_t w_in, int32_t c_in, int32_t c_out,
                         int32_t stride, int32_t dilation, int32_t relu, void* stream) {
    return conv3x3_16("opa_conv3x3_act_bf16", 2, x_dev, w_dev, bias_dev, residual_dev, out_dev, batch, h_in, w_in, c_in, c_out, stride,
                      dilation, relu, stream);
}

int opa_conv3x3_act_f16(const void* x_dev, const void* w_dev, const float* bias_dev, const void* residual_dev, void* out_dev,
                        int32_t batch, int32_t h_in, int32_t w_in, int32_t c_in, int32_t c_out,
                        int32_t stride, int32_t dilation, int32_t relu, void* stream) {
    return conv3x3_16("opa_conv3x3_act_f16", 1, x_dev, w_dev, bias_dev, residual_dev, out_dev, batch, h_in, w_in, c_in, c_out, stride,
                      dilation, relu, stream);
}

// the grouped 3x3 convolution of a bfloat16 ResNeXt as an implicit GEMM per 64-channel chunk on the bf16 MFMA (csrc/gconv3x3_bf16.hip):
// one message per check, in this order: null pointers, alignment, negative sizes, channels, group_width, the stride, the dilation, x's
// size, out's size; then the empty call; then the grid.  opa_gconv3x3_act_bf16 and its float16 twin (`dtype` 1: x, w and out float16,
// the kernel on the f16 MFMA)
static int gconv3x3_16(const char* fn, int dtype, const void* x_dev, const void* w_dev, const float* bias_dev, void* out_dev,
                       int32_t batch, int32_t h_in, int32_t w_in, int32_t channels, int32_t group_width,
                       int32_t stride, int32_t dilation, int32_t relu, void* stream) {
    const Entry E(fn, stream);
    if (!x_dev || !w_dev || !out_dev) return E.refuse("x_dev, w_dev and out_dev must not be NULL");
    if (misaligned(15, {x_dev, w_dev, bias_dev, out_dev})) return E.refuse("pointers must be 16-B aligned");
    if (batch < 0 || h_in < 0 || w_in < 0) return E.refuse("negative batch, h_in or w_in");
    if (channels <= 0 || channels % 64 != 0) return E.refuse("channels must be a positive multiple of 64");
    if (group_width != 4 && group_width != 8 && group_width != 16 && group_width != 32 && group_width != 64)
        return E.refuse("group_width must be 4, 8, 16, 32 or 64");
    if (group_width == channels) return E.refuse("group_width must be below channels (one group is the dense convolution)");
    if (stride != 1 && stride != 2) return E.refuse("stride must be 1 or 2");
    if (dilation != 1 && dilation != 2 && dilation != 4) return E.refuse("dilation must be 1, 2 or 4");
    if (dilation > 1 && stride != 1) return E.refuse("a dilation above 1 needs stride 1");
    // 32-bit element offsets into both tensors (in double: exact up to 2^53, and no product of these arguments overflows it)
    const double ho = h_in > 0 ? (h_in - 1) / stride + 1 : 0, wo = w_in > 0 ? (w_in - 1) / stride + 1 : 0;
    if ((double)batch * h_in * w_in * channels >= 2147483648.0) return E.refuse("x must hold fewer than 2^31 elements (32-bit offsets)");
    if ((double)batch * ho * wo * channels >= 2147483648.0) return E.refuse("out must hold fewer than 2^31 elements (32-bit offsets)");
    if (batch == 0 || h_in == 0 || w_in == 0) return OPA_OK;
    // (grid.x; with out below 2^31 elements and 64 channels per tile it holds today: it guards the launch should a limit above move)
    if (gconv3x3_bf16_workgroups(batch, h_in, w_in, channels, stride) > 0x7fffffffll) return E.refuse("too many tiles for grid.x");
    return E.launched(launch_gconv3x3_bf16(x_dev, w_dev, bias_dev, out_dev, batch, h_in, w_in, channels, group_width, stride, dilation,
                                           relu, E.st, dtype), dtype == 1 ? "gconv3x3_act_f16" : "gconv3x3_act_bf16",
                      dtype == 1 ? "gconv3x3_f16_kernel" : "gconv3x3_bf16_kernel");
}

int opa_gconv3x3_act_bf16(const void* x_dev, const void* w_dev, const float* bias_dev, void* out_dev,
                          int32_t batch, int32_t h_in, int32_t w_in, int32_t channels, int32_t group_width,
                          int32_t stride, int32_t dilation, int32_t relu, void* stream) {
    return gconv3x3_16("opa_gconv3x3_act_bf16", 2, x_dev, w_dev, bias_dev, out_dev, batch, h_in, w_in, channels, group_width, stride,
                       dilation, relu, stream);
}

int opa_gconv3x3_act_f16(const void* x_dev, const void* w_dev, const float* bias_dev, void* out_dev,
                         int32_t batch, int32_t h_in, int32_t w_in, int32_t channels, int32_t group_width,
                         int32_t stride, int32_t dilation, int32_t relu, void* stream) {
    return gconv3x3_16("opa_gconv3x3_act_f16", 1, x_dev, w_dev, bias_dev, out_dev, batch, h_in, w_in, channels, group_width, stride,
                       dilation, relu, stream);
}

// the 7x7 RGB stem of a bfloat16 ResNet as an implicit GEMM on the bf16 MFMA (csrc/stem7x7_bf16.hip): one message per check, in this
// order: null pointers, alignment, negative sizes, c_out, the stride, x's strides, x's extent, out's size; then the empty call; then the
// grid.  opa_stem7x7_act_bf16 and its float16 twin (`dtype` 1: x, w and out float16, the kernel on the f16 MFMA)
static int stem7x7_16(const char* fn, int dtype, const void* x_dev, int64_t x_batch_stride, int64_t x_channel_stride, int64_t x_row_stride,
                      int64_t x_pixel_stride, const void* w_dev, const float* bias_dev, void* out_dev, int32_t batch, int32_t h, int32_t w,
                      int32_t c_out, int32_t stride, int32_t relu, void* stream) {
    const Entry E(fn, stream);
    if (!x_dev || !w_dev || !out_dev) return E.refuse("x_dev, w_dev and out_dev must not be NULL");
    if (misaligned(1, {x_dev}) || misaligned(15, {w_dev, bias_dev, out_dev}))
        return E.refuse("x_dev must be 2-B, w_dev / bias_dev / out_dev 16-B aligned");
    if (batch < 0 || h < 0 || w < 0) return E.refuse("negative batch, h or w");
    if (c_out <= 0 || c_out % 64 != 0) return E.refuse("c_out must be a positive multiple of 64");
    if (stride != 1 && stride != 2) return E.refuse("stride must be 1 or 2");
    if (x_batch_stride <= 0 || x_channel_stride <= 0 || x_row_stride <= 0 || x_pixel_stride <= 0)
        return E.refuse("the four strides of x must be positive");
    // 32-bit element offsets into both tensors (in double: no product of these arguments overflows it, and what it rounds is far
    // above 2^31); the stride of a dimension of one element -- or of none -- addresses nothing
    const double last = std::max(batch - 1.0, 0.0) * (double)x_batch_stride + 2.0 * (double)x_channel_stride +
                        std::max(h - 1.0, 0.0) * (double)x_row_stride + std::max(w - 1.0, 0.0) * (double)x_pixel_stride;
    if (last >= 2147483648.0) return E.refuse("x must span fewer than 2^31 elements, first to last addressed (32-bit offsets)");
    const double ho = h > 0 ? (h - 1) / stride + 1 : 0, wo = w > 0 ? (w - 1) / stride + 1 : 0;
    if ((double)batch * ho * wo * c_out >= 2147483648.0) return E.refuse("out must hold fewer than 2^31 elements (32-bit offsets)");
    if (batch == 0 || h == 0 || w == 0) return OPA_OK;
    // (grid.x; with out below 2^31 elements of at least 64 channels it holds today: it guards the launch should a limit above move)
    if (stem7x7_bf16_workgroups(batch, h, w, c_out, stride) > 0x7fffffffll) return E.refuse("too many tiles for grid.x");
    return E.launched(launch_stem7x7_bf16(x_dev, x_batch_stride, x_channel_stride, x_row_stride, x_pixel_stride, w_dev, bias_dev, out_dev,
                                          batch, h, w, c_out, stride, relu, E.st, dtype), dtype == 1 ? "stem7x7_act_f16" : "stem7x7_act_bf16",
                      dtype == 1 ? "stem7x7_f16_kernel" : "stem7x7_bf16_kernel");
}

int opa_stem7x7_act_bf16(const void* x_dev, int64_t x_batch_stride, int64_t x_channel_stride, int64_t x_row_stride, int64_t x_pixel_stride,
                         const void* w_dev, const float* bias_dev, void* out_dev, int32_t batch, int32_t h, int32_t w, int32_t c_out,
                         int32_t stride, int32_t relu, void* stream) {
    return stem7x7_16("opa_stem7x7_act_bf16", 2, x_dev, x_batch_stride, x_channel_stride, x_row_stride, x_pixel_stride, w_dev, bias_dev, out_dev,
                      batch, h, w, c_out, stride, relu, stream);
}

int opa_stem7x7_act_f16(const void* x_dev, int64_t x_batch_stride, int64_t x_channel_stride, int64_t x_row_stride, int64_t x_pixel_stride,
                        const void* w_dev, const float* bias_dev, void* out_dev, int32_t batch, int32_t h, int32_t w, int32_t c_out,
                        int32_t stride, int32_t relu, void* stream) {
    return stem7x7_16("opa_stem7x7_act_f16", 1, x_dev, x_batch_stride, x_channel_stride, x_row_stride, x_pixel_stride, w_dev, bias_dev, out_dev,
                      batch, h, w, c_out, stride, relu, stream);
}

// a bfloat16 block's last 1x1 convolution and its downsampling 1x1 convolution as one product on the bf16 MFMA (csrc/gemm2_bf16.hip):
// one message per check, in this order: null pointers, alignment, negative sizes, k1, k2, n, the stride, the sizes; then the empty call;
// then the grid.  opa_gemm2_bias_act_bf16 and its float16 twin (`dtype` 1: a1, a2, a_bias, wcat and out float16, the kernel on the f16 MFMA)
static int gemm2_16(const char* fn, int dtype, const void* a1_dev, int32_t k1, const void* a2_dev, int32_t k2, int32_t batch, int32_t h_in,
                    int32_t w_in, int32_t stride, const void* a_bias_dev, const void* wcat_dev, const float* bias_dev, void* out_dev,
                    int32_t n, int32_t relu, void* stream) {
    const Entry E(fn, stream);
    if (!a2_dev || !wcat_dev || !out_dev) return E.refuse("a2_dev, wcat_dev and out_dev must not be NULL");
    if ((a1_dev == nullptr) != (k1 == 0)) return E.refuse("a1_dev must be NULL with k1 == 0 and with no other k1");
    if (a_bias_dev && k1 <= 0) return E.refuse("a_bias_dev needs k1 > 0");
    if (misaligned(15, {a1_dev, a2_dev, a_bias_dev, wcat_dev, bias_dev, out_dev})) return E.refuse("pointers must be 16-B aligned");
    if (batch < 0 || h_in < 0 || w_in < 0) return E.refuse("negative batch, h_in or w_in");
    if (k1 < 0 || k1 % 64 != 0) return E.refuse("k1 must be 0 or a positive multiple of 64");
    if (k2 <= 0 || k2 % 64 != 0) return E.refuse("k2 must be a positive multiple of 64");
    if (n <= 0 || n % 64 != 0) return E.refuse("n must be a positive multiple of 64");
    if (stride != 1 && stride != 2) return E.refuse("stride must be 1 or 2");
    // 32-bit element offsets into the three tensors (in double: exact up to 2^53, and no product of these arguments overflows it)
    const double ho = h_in > 0 ? (h_in - 1) / stride + 1 : 0, wo = w_in > 0 ? (w_in - 1) / stride + 1 : 0;
    if ((double)batch * h_in * w_in * k2 >= 2147483648.0) return E.refuse("a2 must hold fewer than 2^31 elements (32-bit offsets)");
    if ((double)batch * ho * wo * k1 >= 2147483648.0) return E.refuse("a1 must hold fewer than 2^31 elements (32-bit offsets)");
    if ((double)batch * ho * wo * n >= 2147483648.0) return E.refuse("out must hold fewer than 2^31 elements (32-bit offsets)");
    if (batch == 0 || h_in == 0 || w_in == 0) return OPA_OK;
    // (grid.x; with out below 2^31 elements of at least 64 channels it holds today: it guards the launch should a limit above move)
    if (gemm2_bf16_workgroups(batch, h_in, w_in, n, stride) > 0x7fffffffll) return E.refuse("too many tiles for grid.x");
    const hipError_t e = launch_gemm2_bf16(a1_dev, k1, a2_dev, k2, batch, h_in, w_in, stride, a_bias_dev, wcat_dev, bias_dev, out_dev, n, relu,
                                           E.st, dtype);
    if (dtype == 1) return E.launched(e, "gemm2_bias_act_f16", a_bias_dev ? "gemm2_pro_f16_kernel" : "gemm2_f16_kernel");
    return E.launched(e, "gemm2_bias_act_bf16", a_bias_dev ? "gemm2_pro_bf16_kernel" : "gemm2_bf16_kernel");
}

int opa_gemm2_bias_act_bf16(const void* a1_dev, int32_t k1, const void* a2_dev, int32_t k2, int32_t batch, int32_t h_in, int32_t w_in,
                            int32_t stride, const void* a_bias_dev, const void* wcat_dev, const float* bias_dev, void* out_dev,
                            int32_t n, int32_t relu, void* stream) {
    return gemm2_16("opa_gemm2_bias_act_bf16", 2, a1_dev, k1, a2_dev, k2, batch, h_in, w_in, stride, a_bias_dev, wcat_dev, bias_dev, out_dev,
                    n, relu, stream);
}

int opa_gemm2_bias_act_f16(const void* a1_dev, int32_t k1, const void* a2_dev, int32_t k2, int32_t batch, int32_t h_in, int32_t w_in,
                           int32_t stride, const void* a_bias_dev, const void* wcat_dev, const float* bias_dev, void* out_dev,
                           int32_t n, int32_t relu, void* stream) {
    return gemm2_16("opa_gemm2_bias_act_f16", 1, a1_dev, k1, a2_dev, k2, batch, h_in, w_in, stride, a_bias_dev, wcat_dev, bias_dev, out_dev,
                    n, relu, stream);
}

// opa_conv3x3_winograd_f32 and opa_conv3x3_winograd_f32x3 (`x3`: u_dev holds the three bf16 planes of the filter)
static int conv3x3_winograd(const char* fn, bool x3, const float* x_dev, const void* u_dev, const float* bias_dev, float* out_dev,
                            int32_t batch, int32_t h, int32_t w, int32_t c_in, int32_t c_out, int32_t relu, int32_t variant,
                            int32_t order, void* stream) {
    const Entry E(fn, stream);
    // (x3's variant 5, the 128-channel workgroups forced, exists for c_out % 128 == 0 only)
    const bool known = x3 ? variant == 4 || (variant == 5 && c_out > 0 && c_out % 128 == 0) || (variant >= 21 && variant <= 23)
                          : (variant >= 0 && variant <= 3) || (variant >= 11 && variant <= 18);
    if (!x_dev || !u_dev || !out_dev || batch <= 0 || h <= 0 || w <= 0 || c_in <= 0 || c_out <= 0 || !known) return E.refuse("bad arguments");
    if (!x3 && variant == 1 ? (c_in % 8 != 0 || c_out % 32 != 0) : (c_in % 16 != 0 || c_out % 64 != 0))
        return E.refuse(x3 ? "c_in % 16 and c_out % 64 must be 0" : "channel counts do not fit the variant's tiles");
    if ((double)batch * h * w * c_in >= 1073741824.0 || (double)batch * ((h + 1) / 2) * ((w + 1) / 2) >= 2147483647.0)
        return E.refuse("the activation needs 32-bit byte offsets (fewer than 2^30 elements)");
    if (misaligned(15, {x_dev, u_dev, out_dev, bias_dev})) return E.refuse("pointers must be 16-B aligned");
    if (x3)
        return E.launched(launch_winograd_f23x3(x_dev, (const unsigned short*)u_dev, out_dev, bias_dev, batch, h, w, c_in, c_out, relu,
                                                variant, order, E.st), "winograd_f23x3", "winograd_f23_w8x3_kernel");
    return E.launched(launch_winograd_f23(x_dev, (const float*)u_dev, out_dev, bias_dev, batch, h, w, c_in, c_out, relu, variant, order, E.st),
                      "winograd_f23", "winograd_f23_kernel");
}

int opa_conv3x3_winograd_f32(const float* x_dev, const float* u_dev, const float* bias_dev, float* out_dev, int32_t batch,
                             int32_t h, int32_t w, int32_t c_in, int32_t c_out, int32_t relu, int32_t variant,
                             int32_t order, void* stream) {
    return conv3x3_winograd("opa_conv3x3_winograd_f32", false, x_dev, u_dev, bias_dev, out_dev, batch, h, w, c_in, c_out, relu, variant,
                            order, stream);
}

int opa_conv3x3_winograd_f32x3(const float* x_dev, const void* u3_dev, const float* bias_dev, float* out_dev, int32_t batch,
                               int32_t h, int32_t w, int32_t c_in, int32_t c_out, int32_t relu, int32_t variant,
                               int32_t order, void* stream) {
    return conv3x3_winograd("opa_conv3x3_winograd_f32x3", true, x_dev, u3_dev, bias_dev, out_dev, batch, h, w, c_in, c_out, relu, variant,
                            order, stream);
}

// opa_dwconv_act, opa_dwconv_bias_act as its call with act 0 / 1, opa_dwconv_dilated_act (`dilated`: k = 7 and a dilation of 2
// or 4 at stride 1 are accepted too; the other two pass dilation 1) and opa_dwconv_actp (`actp`: act 4, the ReLU clipped at
// act_param, is accepted too; the others pass no parameter).  These four take dtype 0 (float32) or 2 (bfloat16); opa_dwconv_actp_f16
// is opa_dwconv_actp's call for float16 tensors (`f16`: dtype 1, which no argument of the others reaches)
static int dwconv(const char* fn, bool dilated, bool actp, float act_param, const void* x_dev, int64_t x_pixel_stride, const void* w_dev, const void* bias_dev,
                  void* out_dev, int64_t out_pixel_stride, int32_t batch, int32_t h, int32_t w, int32_t channels, int32_t k, int32_t stride,
                  int32_t dilation, int32_t dtype, int32_t act, void* stream, bool f16 = false) {
    const Entry E(fn, stream);
    if (actp ? (act < 0 || act > 4 || act == 3) : (act < 0 || act > 2))
        return E.refuse(actp ? "act must be 0 (none), 1 (ReLU), 2 (hardswish) or 4 (clipped ReLU)" : "act must be 0 (none), 1 (ReLU) or 2 (hardswish)");
    if (const char* why = bad_act_param(act, act_param)) return E.refuse(why);          // (act 3 never gets here)
    const bool k_ok = k == 3 || k == 5 || (dilated && k == 7);
    const bool d_ok = dilation == 1 || (dilated && (dilation == 2 || dilation == 4) && stride == 1);
    if (!x_dev || !w_dev || !out_dev || batch <= 0 || h <= 0 || w <= 0 || channels <= 0 || x_pixel_stride < channels ||
        out_pixel_stride < channels || !k_ok || (stride != 1 && stride != 2) || !d_ok || (f16 ? dtype != 1 : (dtype != 0 && dtype != 2)))
        return E.refuse("bad arguments");
    // grid.y of the stencil kernel (dwconv.hip); the padding is (k / 2) * dilation, so the window takes dilation * (k - 1) rows off
    if ((int64_t)batch * (((int64_t)h + 2 * (k / 2) * dilation - dilation * (k - 1) - 1) / stride + 1) > 65535)
        return E.refuse("batch * output rows must not exceed 65535");
    return E.launched(launch_dwconv(x_dev, x_pixel_stride, w_dev, bias_dev, out_dev, out_pixel_stride, batch, h, w, channels, k, stride,
                                    dilation, dtype, act, E.st, act_param), "depthwise convolution");
}

int opa_dwconv_bias_act(const void* x_dev, int64_t x_pixel_stride, const void* w_dev, const void* bias_dev,
                        void* out_dev, int64_t out_pixel_stride, int32_t batch, int32_t h, int32_t w,
                        int32_t channels, int32_t k, int32_t stride, int32_t dtype, int32_t relu, void* stream) {
    return dwconv("opa_dwconv_bias_act", false, false, 0.0f, x_dev, x_pixel_stride, w_dev, bias_dev, out_dev, out_pixel_stride, batch, h, w, channels, k,
                  stride, 1, dtype, relu != 0, stream);                                   // (relu: any non-zero)
}

int opa_dwconv_act(const void* x_dev, int64_t x_pixel_stride, const void* w_dev, const void* bias_dev,
                   void* out_dev, int64_t out_pixel_stride, int32_t batch, int32_t h, int32_t w,
                   int32_t channels, int32_t k, int32_t stride, int32_t dtype, int32_t act, void* stream) {
    return dwconv("opa_dwconv_act", false, false, 0.0f, x_dev, x_pixel_stride, w_dev, bias_dev, out_dev, out_pixel_stride, batch, h, w, channels, k,
                  stride, 1, dtype, act, stream);
}

int opa_dwconv_dilated_act(const void* x_dev, int64_t x_pixel_stride, const void* w_dev, const void* bias_dev,
                           void* out_dev, int64_t out_pixel_stride, int32_t batch, int32_t h, int32_t w,
                           int32_t channels, int32_t k, int32_t stride, int32_t dilation, int32_t dtype, int32_t act, void* stream) {
    return dwconv("opa_dwconv_dilated_act", true, false, 0.0f, x_dev, x_pixel_stride, w_dev, bias_dev, out_dev, out_pixel_stride, batch, h, w, channels,
                  k, stride, dilation, dtype, act, stream);
}

int opa_dwconv_actp(const void* x_dev, int64_t x_pixel_stride, const void* w_dev, const void* bias_dev,
                    void* out_dev, int64_t out_pixel_stride, int32_t batch, int32_t h, int32_t w,
                    int32_t channels, int32_t k, int32_t stride, int32_t dilation, int32_t dtype, int32_t act, float act_param, void* stream) {
    return dwconv("opa_dwconv_actp", true, true, act_param, x_dev, x_pixel_stride, w_dev, bias_dev, out_dev, out_pixel_stride, batch, h, w, channels,
                  k, stride, dilation, dtype, act, stream);
}

int opa_dwconv_actp_f16(const void* x_dev, int64_t x_pixel_stride, const void* w_dev, const void* bias_dev,
                        void* out_dev, int64_t out_pixel_stride, int32_t batch, int32_t h, int32_t w,
                        int32_t channels, int32_t k, int32_t stride, int32_t dilation, int32_t act, float act_param, void* stream) {
    return dwconv("opa_dwconv_actp_f16", true, true, act_param, x_dev, x_pixel_stride, w_dev, bias_dev, out_dev, out_pixel_stride, batch, h, w, channels,
                  k, stride, dilation, 1, act, stream, true);
}

int opa_gconv3x3_bias_act_f32(const float* x_dev, int64_t x_pixel_stride, const float* wt_dev, const float* bias_dev,
                              float* out_dev, int64_t out_pixel_stride, int32_t batch, int32_t h, int32_t w, int32_t channels,
                              int32_t group_width, int32_t stride, int32_t relu, void* stream) {
    const Entry E("opa_gconv3x3_bias_act_f32", stream);
    if (!x_dev || !wt_dev || !out_dev) return E.refuse("x, wt and out must not be NULL");
    if (group_width != 4 && group_width != 8 && group_width != 16 && group_width != 32 && group_width != 64)
        return E.refuse("group_width must be 4, 8, 16, 32 or 64");
    if (channels <= 0 || channels % group_width != 0) return E.refuse("channels must be a positive multiple of group_width");
    if (stride != 1 && stride != 2) return E.refuse("stride must be 1 or 2");
    if (x_pixel_stride < channels || out_pixel_stride < channels || x_pixel_stride % 4 != 0 || out_pixel_stride % 4 != 0)
        return E.refuse("pixel strides must be multiples of 4 and at least channels");
    if (misaligned(15, {x_dev, wt_dev, out_dev, bias_dev})) return E.refuse("pointers must be 16-B aligned");
    if (batch < 0 || h < 0 || w < 0) return E.refuse("negative batch, h or w");
    if (batch == 0 || h == 0 || w == 0) return OPA_OK;                                   // nothing to compute
    if (batch > 65535) return E.refuse("batch must not exceed 65535 (grid.y)");
    if (gconv3x3_workgroups(h, w, channels, stride) > 2147483647ll)                      // (offsets are 64-bit: no limit on the elements)
        return E.refuse("tiles * channel chunks of one image must not exceed 2^31 - 1 (grid.x)");
    return E.launched(launch_gconv3x3(x_dev, x_pixel_stride, wt_dev, bias_dev, out_dev, out_pixel_stride, batch, h, w, channels,
                                      group_width, stride, relu != 0, E.st), "grouped 3x3 convolution");
}

int opa_stem3x3_actp(const float* x_dev, int64_t x_batch_stride, int64_t x_channel_stride, int64_t x_row_stride,
                     int64_t x_pixel_stride, const float* w_dev, const float* bias_dev, float* out_dev,
                     int32_t batch, int32_t h, int32_t w, int32_t channels_out, int32_t stride,
                     int32_t act, float act_param, void* stream) {
    const Entry E("opa_stem3x3_actp", stream);
    if (!x_dev || !w_dev || !out_dev) return E.refuse("x_dev, w_dev and out_dev must not be NULL");
    if (misaligned(3, {x_dev}) || misaligned(15, {w_dev, bias_dev, out_dev}))
        return E.refuse("x_dev must be 4-B, w_dev / bias_dev / out_dev 16-B aligned");
    if (batch < 0 || h <= 0 || w <= 0) return E.refuse("batch must not be negative, h and w must be positive");
    if (x_batch_stride <= 0 || x_channel_stride <= 0 || x_row_stride <= 0 || x_pixel_stride <= 0)
        return E.refuse("the four strides of x must be positive");
    if (stride != 1 && stride != 2) return E.refuse("stride must be 1 or 2");
    if (!stem3x3_channels_ok(channels_out)) return E.refuse("channels_out must be 16, 24, 32, 42 or 64");
    if (act < 0 || act > 4) return E.refuse("act must be 0 (none), 1 (ReLU), 2 (hardswish), 3 (LeakyReLU) or 4 (clipped ReLU)");
    if (const char* why = bad_act_param(act, act_param)) return E.refuse(why);
    if (batch == 0) return OPA_OK;
    // 32-bit element indices in the kernel (in double: exact up to 2^53, and no product of these arguments overflows it); the
    // stride of a dimension of one element addresses nothing
    const double last = ((double)batch - 1.0) * (double)x_batch_stride + 2.0 * (double)x_channel_stride +
                        ((double)h - 1.0) * (double)x_row_stride + ((double)w - 1.0) * (double)x_pixel_stride;
    if (last >= 2147483648.0) return E.refuse("x must span fewer than 2^31 elements (32-bit indices)");
    const double ho = (h - 1) / stride + 1, wo = (w - 1) / stride + 1;
    if ((double)batch * ho * wo * channels_out >= 2147483648.0) return E.refuse("out must hold fewer than 2^31 elements (32-bit indices)");
    if (batch > 65535) return E.refuse("batch must not exceed 65535 (grid.y)");
    return E.launched(launch_stem3x3(x_dev, x_batch_stride, x_channel_stride, x_row_stride, x_pixel_stride, w_dev, bias_dev, out_dev, batch,
                                     h, w, channels_out, stride, act, act_param, E.st), "stem3x3", "stem3x3_kernel");
}

static const char* se_check(int64_t x_pixel_stride, int32_t batch, int64_t pixels, int32_t channels) {
    if (batch <= 0 || batch > 65535 || pixels <= 0 || pixels > 65535ll * kSePoolPixels || channels <= 0 || channels > 8192)
        return "batch, pixels or channels out of range";
    if (channels % 4 != 0 || x_pixel_stride % 4 != 0 || x_pixel_stride < channels) return "channels and the pixel stride must be multiples of 4, the stride >= channels";
    return nullptr;
}

size_t opa_se_workspace_bytes(int32_t batch, int64_t pixels, int32_t channels) {
    if (batch <= 0 || pixels <= 0 || channels <= 0) return 0;
    return (size_t)batch * (size_t)se_pool_chunks(pixels) * (size_t)channels * sizeof(double);
}

int opa_se_pool(const float* x_dev, int64_t x_pixel_stride, int32_t batch, int64_t pixels, int32_t channels,
                void* workspace_dev, size_t workspace_bytes, void* stream) {
    const Entry E("opa_se_pool", stream);
    if (!x_dev || !workspace_dev) return E.refuse("bad arguments");
    if (const char* why = se_check(x_pixel_stride, batch, pixels, channels)) return E.refuse(why);
    if (misaligned(15, {x_dev, workspace_dev})) return E.refuse("pointers must be 16-B aligned");
    if (workspace_bytes < opa_se_workspace_bytes(batch, pixels, channels)) return E.refuse(OPA_ERR_WORKSPACE, "the workspace is too small");
    return E.launched(launch_se_pool(x_dev, x_pixel_stride, batch, pixels, channels, (double*)workspace_dev, E.st), "se pool");
}

int opa_se_gate(const void* workspace_dev, size_t workspace_bytes, int32_t batch, int64_t pixels, int32_t channels, int32_t squeeze,
                const float* w1_dev, const float* b1_dev, const float* w2_dev, const float* b2_dev, float* gate_dev, float* mean_dev,
                void* stream) {
    const Entry E("opa_se_gate", stream);
    if (!workspace_dev || !w1_dev || !b1_dev || !w2_dev || !b2_dev || !gate_dev || squeeze <= 0 || squeeze > 4096)
        return E.refuse("bad arguments");
    if (const char* why = se_check(channels, batch, pixels, channels)) return E.refuse(why);
    if (misaligned(15, {workspace_dev})) return E.refuse("workspace_dev must be 16-B aligned");
    if (workspace_bytes < opa_se_workspace_bytes(batch, pixels, channels)) return E.refuse(OPA_ERR_WORKSPACE, "the workspace is too small");
    return E.launched(launch_se_gate((const double*)workspace_dev, batch, pixels, channels, squeeze, w1_dev, b1_dev, w2_dev, b2_dev,
                                     gate_dev, mean_dev, E.st), "se gate");
}

int opa_se_scale(float* x_dev, int64_t x_pixel_stride, int32_t batch, int64_t pixels, int32_t channels, const float* gate_dev,
                 void* stream) {
    const Entry E("opa_se_scale", stream);
    if (!x_dev || !gate_dev) return E.refuse("bad arguments");
    if (const char* why = se_check(x_pixel_stride, batch, pixels, channels)) return E.refuse(why);
    if (misaligned(15, {x_dev, gate_dev})) return E.refuse("pointers must be 16-B aligned");
    return E.launched(launch_se_scale(x_dev, x_pixel_stride, batch, pixels, channels, gate_dev, E.st), "se scale");
}

size_t opa_groupnorm_workspace_bytes(int32_t batch, int64_t pixels, int32_t channels) {
    if (batch <= 0 || pixels <= 0 || channels <= 0) return 0;
    return groupnorm_partial_bytes(batch, pixels, channels) + (size_t)batch * (size_t)channels * 2 * sizeof(float);
}

int opa_groupnorm_actp(const float* x_dev, int64_t x_pixel_stride, const float* gamma_dev, const float* beta_dev, float* out_dev,
                       int64_t out_pixel_stride, int32_t batch, int64_t pixels, int32_t channels, int32_t groups, float eps,
                       int32_t act, float act_param, void* workspace_dev, size_t workspace_bytes, void* stream) {
    const Entry E("opa_groupnorm_actp", stream);
    if (!x_dev || !out_dev) return E.refuse("x_dev and out_dev must not be NULL");
    if (misaligned(7, {x_dev, out_dev}) || misaligned(3, {gamma_dev, beta_dev}) || misaligned(15, {workspace_dev}))
        return E.refuse("x_dev / out_dev must be 8-B, gamma_dev / beta_dev 4-B, workspace_dev 16-B aligned");
    if (batch < 0 || pixels <= 0 || channels <= 0 || groups <= 0)
        return E.refuse("batch must not be negative, pixels, channels and groups must be positive");
    if (channels % groups != 0) return E.refuse("channels must be a multiple of groups");
    if ((channels / groups) % 2 != 0) return E.refuse("channels / groups must be even");
    if (x_pixel_stride % 2 != 0 || out_pixel_stride % 2 != 0 || x_pixel_stride < channels || out_pixel_stride < channels)
        return E.refuse("pixel strides must be even and at least channels");
    if (!std::isfinite(eps) || eps < 0.0f) return E.refuse("eps must be finite and not negative");
    if (act < 0 || act > 4) return E.refuse("act must be 0 (none), 1 (ReLU), 2 (hardswish), 3 (LeakyReLU) or 4 (clipped ReLU)");
    if (const char* why = bad_act_param(act, act_param)) return E.refuse(why);
    if (out_dev == x_dev && out_pixel_stride != x_pixel_stride) return E.refuse("out_dev == x_dev (in place) needs equal pixel strides");
    if (batch == 0) return OPA_OK;
    // the grids and the indices first: behind them the workspace's size is a product that fits
    if (batch > 65535) return E.refuse("batch must not exceed 65535 (grid.y)");
    if (pixels > 65535ll * kGnChunkPixels) return E.refuse("pixels must not exceed 65535 * OPA_GN_CHUNK_PIXELS (grid.y)");
    if (channels / groups > kGnMaxGroupWidth) return E.refuse("channels / groups must not exceed 2048");
    // (in double: exact up to 2^53, and no product of these arguments overflows it)
    if ((double)pixels * (double)(channels / 2) >= 2147483648.0)
        return E.refuse("pixels * channels / 2 must stay below 2^31 (32-bit vector indices within an image)");
    if (!workspace_dev) return E.refuse(OPA_ERR_WORKSPACE, "workspace_dev must not be NULL");
    if (workspace_bytes < opa_groupnorm_workspace_bytes(batch, pixels, channels)) return E.refuse(OPA_ERR_WORKSPACE, "the workspace is too small");
    return E.launched(launch_groupnorm(x_dev, x_pixel_stride, gamma_dev, beta_dev, out_dev, out_pixel_stride, batch, pixels, channels, groups,
                                       eps, act, act_param, workspace_dev, E.st), "group norm");
}

int opa_channel_interleave(const void* a_dev, int64_t a_pixel_stride, const void* b_dev, int64_t b_pixel_stride,
                           void* out_dev, int64_t rows, int32_t half, int32_t dtype, void* stream) {
    const Entry E("opa_channel_interleave", stream);
    if (!a_dev || !b_dev || !out_dev || rows <= 0 || half <= 0 || a_pixel_stride < half || b_pixel_stride < half ||
        dtype < 0 || dtype > 2)
        return E.refuse("bad arguments");
    return E.launched(launch_channel_interleave(a_dev, a_pixel_stride, b_dev, b_pixel_stride, out_dev, rows, half, dtype, E.st),
                      "channel interleave");
}

int opa_head_epilogue(const void* conv_dev, int32_t dtype, int32_t batch, int32_t hc, int32_t wc,
                      int32_t n_fields, int32_t n_components, int32_t upsample, int32_t n_confidences,
                      int32_t n_vectors, uint32_t vector_offset_mask, int32_t n_scales, float* out_dev, void* stream) {
    const Entry E("opa_head_epilogue", stream);
    if (!conv_dev || !out_dev || batch <= 0 || hc <= 0 || wc <= 0 || n_fields <= 0 || n_components <= 0 ||
        dtype < 0 || dtype > 2 || (upsample != 1 && upsample != 2) || n_confidences < 0 || n_vectors < 0 || n_scales < 0 ||
        1 + n_confidences + 2 * n_vectors + n_scales > n_components)
        return E.refuse("bad arguments");
    return E.launched(launch_head_epilogue(conv_dev, dtype, batch, hc, wc, n_fields, n_components, upsample, n_confidences,
                                           n_vectors, vector_offset_mask, n_scales, out_dev, E.st), "head epilogue");
}

// a 16-bit head's 1x1 convolution and the head epilogue as one kernel on the 16-bit MFMA (csrc/head16.hip): one message per check, in
// this order: null pointers, alignment, a negative batch, the sizes, k, upsample, the component counts, x's size, the weight's rows,
// out's size; then the empty call; then the grid.  opa_head_conv_fields_bf16 and its float16 twin (`dtype` 1: x and w float16, the
// kernel on the f16 MFMA)
static int head_conv_fields_16(const char* fn, int dtype, const void* x_dev, const void* w_dev, const float* bias_dev, float* out_dev,
                               int32_t batch, int32_t hc, int32_t wc, int32_t k, int32_t n_fields, int32_t n_components, int32_t upsample,
                               int32_t n_confidences, int32_t n_vectors, uint32_t vector_offset_mask, int32_t n_scales, void* stream) {
    const Entry E(fn, stream);
    if (!x_dev || !w_dev || !bias_dev || !out_dev) return E.refuse("x_dev, w_dev, bias_dev and out_dev must not be NULL");
    if (misaligned(15, {x_dev, w_dev}) || misaligned(3, {bias_dev, out_dev}))
        return E.refuse("x_dev / w_dev must be 16-B, bias_dev / out_dev 4-B aligned");
    if (batch < 0) return E.refuse("negative batch");
    if (hc <= 0 || wc <= 0 || k <= 0 || n_fields <= 0 || n_components <= 0) return E.refuse("hc, wc, k, n_fields and n_components must be positive");
    if (k % 64 != 0) return E.refuse("k must be a multiple of 64");
    if (upsample != 1 && upsample != 2) return E.refuse("upsample must be 1 or 2");
    // (in 64 bits: the counts are 32-bit)
    if (n_confidences < 0 || n_vectors < 0 || n_scales < 0 || 1ll + n_confidences + 2ll * n_vectors + n_scales != n_components)
        return E.refuse("n_components must be 1 + n_confidences + 2 * n_vectors + n_scales, no count negative");
    // 32-bit element offsets into x and out, a 32-bit column count (in double: exact up to 2^53, and no product of these arguments
    // overflows it); the weight's rows are addressed in 64 bits
    const double pixels = (double)batch * hc * wc, n = (double)n_fields * n_components * upsample * upsample;
    if (pixels * k >= 2147483648.0) return E.refuse("x must hold fewer than 2^31 elements (32-bit offsets)");
    if (n > 2147483584.0) return E.refuse("n_fields * n_components * upsample^2 must not exceed 2^31 - 64");
    const double ho = (double)hc * upsample - (upsample - 1), wo = (double)wc * upsample - (upsample - 1);
    if ((double)batch * n_fields * n_components * ho * wo >= 2147483648.0) return E.refuse("out must hold fewer than 2^31 elements (32-bit offsets)");
    if (batch == 0) return OPA_OK;
    // (grid.x: tiles of 128 pixels x 64 columns)
    if (head16_workgroups(batch, hc, wc, n_fields, n_components, upsample) > 0x7fffffffll) return E.refuse("too many tiles for grid.x");
    return E.launched(launch_head16(x_dev, w_dev, bias_dev, out_dev, batch, hc, wc, k, n_fields, n_components, upsample, n_confidences, n_vectors,
                                    vector_offset_mask, n_scales, E.st, dtype), dtype == 1 ? "head_conv_fields_f16" : "head_conv_fields_bf16",
                      dtype == 1 ? "head16_f16_kernel" : "head16_bf16_kernel");
}

int opa_head_conv_fields_bf16(const void* x_dev, const void* w_dev, const float* bias_dev, float* out_dev,
                              int32_t batch, int32_t hc, int32_t wc, int32_t k,
                              int32_t n_fields, int32_t n_components, int32_t upsample, int32_t n_confidences,
                              int32_t n_vectors, uint32_t vector_offset_mask, int32_t n_scales, void* stream) {
    return head_conv_fields_16("opa_head_conv_fields_bf16", 2, x_dev, w_dev, bias_dev, out_dev, batch, hc, wc, k, n_fields, n_components, upsample,
                               n_confidences, n_vectors, vector_offset_mask, n_scales, stream);
}

int opa_head_conv_fields_f16(const void* x_dev, const void* w_dev, const float* bias_dev, float* out_dev,
                             int32_t batch, int32_t hc, int32_t wc, int32_t k,
                             int32_t n_fields, int32_t n_components, int32_t upsample, int32_t n_confidences,
                             int32_t n_vectors, uint32_t vector_offset_mask, int32_t n_scales, void* stream) {
    return head_conv_fields_16("opa_head_conv_fields_f16", 1, x_dev, w_dev, bias_dev, out_dev, batch, hc, wc, k, n_fields, n_components, upsample,
                               n_confidences, n_vectors, vector_offset_mask, n_scales, stream);
}

size_t opa_pre_image_bytes(void) { return sizeof(opa_pre_image); }

static size_t pre_mid_bytes(const opa_pre_image& d) { return align_up((size_t)d.h0 * (((size_t)d.tw * 3 + 15) & ~(size_t)15)); }

// the sizes of one descriptor row; `why` names the field
static bool check_pre_sizes(const opa_pre_image* images, int32_t batch, const char* who, std::string* why) {
    if (!images) { *why = std::string(who) + ": images_host is null"; return false; }
    if (batch < 1 || batch > 65535) { *why = std::string(who) + ": batch must be 1..65535"; return false; }
    for (int32_t b = 0; b < batch; b++) {
        const opa_pre_image& d = images[b];
        const char* field = d.h0 < 1 ? "h0" : d.w0 < 1 ? "w0" : d.th < 1 ? "th" : d.tw < 1 ? "tw" : nullptr;
        if (field) { *why = std::string(who) + ": images[" + std::to_string(b) + "]." + field + " must be at least 1"; return false; }
        if ((int64_t)d.h0 * d.w0 > 0x3fffffff || (int64_t)d.h0 * d.tw > 0x3fffffff) {
            *why = std::string(who) + ": images[" + std::to_string(b) + "]: h0 * w0 and h0 * tw must stay below 2^30"; return false;
        }
    }
    return true;
}

size_t opa_preprocess_workspace_bytes(const opa_pre_image* images_host, int32_t batch, int32_t mode) {
    std::string why;
    if (!check_pre_sizes(images_host, batch, "opa_preprocess_workspace_bytes", &why)) { fail(0, why); return 0; }
    if (mode != 0 && mode != 1) { fail(0, "opa_preprocess_workspace_bytes: mode must be 0 or 1"); return 0; }
    size_t total = 0;
    if (mode == 0)
        for (int32_t b = 0; b < batch; b++)
            if (images_host[b].tw != images_host[b].w0) total += pre_mid_bytes(images_host[b]);
    return total;
}

int opa_preprocess_u8(const opa_pre_image* images_host, const opa_pre_image* images_dev, int32_t batch,
                      const uint8_t* frames_dev, size_t frames_bytes, const int32_t* tables_dev, size_t tables_words,
                      uint8_t* workspace_dev, size_t workspace_bytes, const float* lut_dev, float* out_dev,
                      int32_t canvas_h, int32_t canvas_w, int32_t mode, int32_t channels_last, uint32_t fill_rgb,
                      void* stream) {
    const char* who = "opa_preprocess_u8";
    auto bad = [&](const std::string& what) { return fail(OPA_ERR_INVALID_ARGUMENT, std::string(who) + ": " + what); };
    if (!images_dev) return bad("images_dev is null");
    if (!frames_dev) return bad("frames_dev is null");
    if (!tables_dev) return bad("tables_dev is null");
    if (!lut_dev) return bad("lut_dev is null");
    if (!out_dev) return bad("out_dev is null");
    std::string why;
    if (!check_pre_sizes(images_host, batch, who, &why)) return fail(OPA_ERR_INVALID_ARGUMENT, why);
    if (mode != 0 && mode != 1) return bad("mode must be 0 (Pillow) or 1 (zoom)");
    if (canvas_h < 1 || canvas_h > 65535) return bad("canvas_h must be 1..65535");
    if (canvas_w < 1) return bad("canvas_w must be at least 1");
    if (((uintptr_t)frames_dev | (uintptr_t)tables_dev | (uintptr_t)workspace_dev | (uintptr_t)images_dev) & 15)
        return bad("frames_dev, tables_dev, workspace_dev and images_dev must be 16-B aligned");
    if (frames_bytes % 16) return bad("frames_bytes must be a multiple of 16");
    unsigned h_blocks = 0;
    int in_cap = 1;
    size_t ws_need = 0;
    for (int32_t b = 0; b < batch; b++) {
        const opa_pre_image& d = images_host[b];
        const std::string at = "images[" + std::to_string(b) + "].";
        if (d.top < 0 || d.left < 0 || (int64_t)d.top + d.th > canvas_h || (int64_t)d.left + d.tw > canvas_w)
            return bad(at + "top / left: the placement lies outside the canvas");
        if (d.x_ksize < 1) return bad(at + "x_ksize must be at least 1");
        if (d.y_ksize < 1) return bad(at + "y_ksize must be at least 1");
        if (d.src_offset < 0 || (uint64_t)d.src_offset + (uint64_t)d.h0 * d.w0 * 3 > frames_bytes)
            return bad(at + "src_offset: the frame lies outside frames_bytes");
        const size_t x_words = mode ? ((3 * (size_t)d.tw + 1) & ~(size_t)1) + 4 * (size_t)d.tw : (size_t)(1 + d.x_ksize) * d.tw;
        const size_t y_words = mode ? ((3 * (size_t)d.th + 1) & ~(size_t)1) + 4 * (size_t)d.th : (size_t)(1 + d.y_ksize) * d.th;
        if (d.x_table < 0 || d.x_table % 4 || (size_t)d.x_table + x_words > tables_words)
            return bad(at + "x_table: the table lies outside tables_words or is not a multiple of 4 words");
        if (d.y_table < 0 || d.y_table % 4 || (size_t)d.y_table + y_words > tables_words)
            return bad(at + "y_table: the table lies outside tables_words or is not a multiple of 4 words");
        // source pixels of one row that 256 neighbouring output columns reach (sizes the kernels' LDS)
        double span;
        if (mode) {
            if (d.x_ksize != 2 || d.y_ksize != 2) return bad(at + "x_ksize / y_ksize must be 2 in mode 1");
            span = std::ceil(255.0 * (d.tw > 1 ? (double)(d.w0 - 1) / (d.tw - 1) : 0.0)) + 3.0;
        } else if (d.tw != d.w0) {
            const double scale = (double)d.w0 / d.tw;
            span = std::ceil(255.0 * scale) + 2.0 * std::ceil(std::max(scale, 1.0)) + 4.0;
            if (d.mid_offset < 0 || d.mid_offset % 16) return bad(at + "mid_offset must be a non-negative multiple of 16");
            ws_need = std::max(ws_need, (size_t)d.mid_offset + pre_mid_bytes(d));
            const unsigned chunks = ((unsigned)d.tw + 255u) / 256u;
            h_blocks = std::max(h_blocks, (unsigned)d.h0 * chunks);
        } else {
            span = 1.0;
        }
        in_cap = std::max(in_cap, (int)std::min(span, (double)d.w0));
    }
    const size_t lds = mode ? preprocess_zoom_lds_bytes(in_cap) : preprocess_h_lds_bytes(in_cap);
    if (lds > 65536) return bad("w0 / tw: 256 output columns reach more source pixels than 64 KB of LDS hold");
    if (ws_need > 0 && !workspace_dev) return bad("workspace_dev is null");
    if (ws_need > workspace_bytes)
        return fail(OPA_ERR_WORKSPACE, std::string(who) + ": workspace_bytes is " + std::to_string(workspace_bytes) + ", the batch needs " + std::to_string(ws_need));
    hipError_t e = launch_preprocess(images_dev, batch, frames_dev, tables_dev, workspace_dev, lut_dev, out_dev, canvas_h, canvas_w,
                                     mode, channels_last, fill_rgb, h_blocks, in_cap, (hipStream_t)stream);
    if (e != hipSuccess) return fail_hip(e, "image preprocessing");
    return OPA_OK;
}

}  // extern "C"
