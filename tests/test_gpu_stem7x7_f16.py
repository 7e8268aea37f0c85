"""The 7x7 stem implicit GEMM instantiated for float16 (csrc/stem7x7_bf16.hip with DT = 1 on v_mfma_f32_32x32x16_f16,
``opa_stem7x7_act_f16``, behind ``fused.STEM7_F16``): the RGB stem of a ResNet cast with ``.half()``.  Shapes and cases are
``test_gpu_stem7x7_bf16.py``'s: ``(B, h, w)`` = (3, 23, 19) gives M = 1311 rows at stride 1 and 360 at stride 2 (neither a multiple of
the 128-row tile), (2, 7, 5) is less than one tile and its 7-wide window overhangs the 5-wide image on both sides at once, (1, 1, 1)
leaves only the centre tap; ``c_out`` = 64 is one N tile, 128 two; ``x`` is NCHW, channels-last, or a view cropped out of a larger
channels-last image whose other pixels hold NaN.

Known answers are demanded bit for bit, among them integers that only float16 holds (odd ones between 257 and 2047).  Random
operands are held, per element, to ``|got - ref| <= 2 n 2^-24 S + ulp16(ref) / 2``: n = 192 + 2 additions in float32 in any order (the
kernel's K is 192), doubled (truncating adders), S the float64 sum of magnitudes with the bias,
ulp16(v) = 2^(max(floor(log2 |v|), -14) - 10) for the one rounding of the store -- derived, not measured -- and to the project's
relative bar, 1.05 x the error of torch's own float16 convolution.  The store is checked at float16's edges against
``accumulator.to(torch.float16)`` computed on the CPU.  Every reference is float64, formed from 49 shifted products -- never torch's
GPU convolution."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

CL = torch.channels_last
F16 = torch.float16
SHAPES = [(3, 23, 19), (2, 7, 5), (1, 1, 1)]
LAYOUTS = ['nchw', 'cl', 'crop']
CASES = [pytest.param(n, s, layout, id='n%d-s%d-%s' % (n, s, layout)) for n in (64, 128) for s in (1, 2) for layout in LAYOUTS]
assert 3 * 23 * 19 == 1311 and 1311 % 128 != 0 and 3 * 12 * 10 == 360 and 360 % 128 != 0


def _bits(t):
    return t.contiguous().view(torch.int16)


def _out_hw(h, w, s):
    return (h - 1) // s + 1, (w - 1) // s + 1


def _taps(x, s):
    """``x`` [B, 3, h, w] -> the 49 shifted views [B, 3, ho, wo] (tap 7 ky + kx; zeros in the padding), the plain definition."""
    b, c, h, w = x.shape
    ho, wo = _out_hw(h, w, s)
    xp = torch.zeros((b, c, h + 6, w + 6), dtype=x.dtype, device=x.device)
    xp[:, :, 3:3 + h, 3:3 + w] = x
    return [xp[:, :, ky:ky + s * (ho - 1) + 1:s, kx:kx + s * (wo - 1) + 1:s] for ky in range(7) for kx in range(7)]


def _conv64(x, w, s, absolute=False):
    """sum over the 49 taps of [M, 3] @ [3, N] in float64 -> [M, N]; ``absolute``: of the magnitudes (the bound's S).
    ``x`` [B, 3, h, w], ``w`` [N, 3, 7, 7]."""
    x, w = x.double(), w.double()
    if absolute:
        x, w = x.abs(), w.abs()
    total = None
    for tap, view in enumerate(_taps(x, s)):
        part = view.permute(0, 2, 3, 1).reshape(-1, 3) @ w[:, :, tap // 7, tap % 7].t()
        total = part if total is None else total + part
    return total


def _held(marks, s):
    """``marks`` [B, 3, h, w] of 0 / 1 -> [M]: how many marked elements the output pixel's window holds."""
    return sum(view.permute(0, 2, 3, 1).reshape(-1, 3).sum(1) for view in _taps(marks.double(), s))


def _conv_of(w, s):
    """A float16 7x7 convolution with the weight ``w`` [N, 3, 7, 7] (values exact in float16), stride s, padding 3."""
    conv = torch.nn.Conv2d(3, w.shape[0], 7, s, 3, bias=False).cuda().to(F16).requires_grad_(False)
    conv.weight.copy_(w)
    assert torch.equal(conv.weight.double(), w.double())
    return conv


def _image(x, layout):
    """``x`` [B, 3, h, w] (float16-exact values) -> the float16 tensor of these values in ``layout``.  'crop': a view of a
    channels-last [B, 3, h + 5, w + 4] whose other pixels hold NaN."""
    x = x.to(F16)
    if layout == 'nchw':
        return x.contiguous()
    if layout == 'cl':
        return x.contiguous(memory_format=CL)
    b, c, h, w = x.shape
    big = torch.full((b, c, h + 5, w + 4), float('nan'), dtype=F16, device=x.device).contiguous(memory_format=CL)
    view = big[:, :, 2:2 + h, 1:1 + w]
    view.copy_(x)
    assert not view.is_contiguous() and not view.is_contiguous(memory_format=CL) or h * w == 1
    return view


def _run(x, w, bias, s, layout, relu=False):
    """``x`` [B, 3, h, w], ``w`` [N, 3, 7, 7], ``bias`` [N] or None (all float16-exact) -> [M, N] float16 through the launcher."""
    from openpifpaf_amd import fused
    b, _, h, wd = x.shape
    n = w.shape[0]
    ho, wo = _out_hw(h, wd, s)
    conv, xi = _conv_of(w, s), _image(x, layout)
    bi = None if bias is None else bias.to(F16)
    old, fused.STEM7_F16 = fused.STEM7_F16, True
    try:
        assert fused.stem7x7_bf16_supported(conv, xi, bi)
    finally:
        fused.STEM7_F16 = old
    out = fused.stem7x7_bias_act_bf16(conv, xi, bi, relu=relu)
    torch.cuda.synchronize()
    assert out.dtype == F16 and out.is_contiguous(memory_format=CL) and tuple(out.shape) == (b, n, ho, wo)
    return out.permute(0, 2, 3, 1).reshape(-1, n)


@pytest.mark.parametrize('n,s,layout', CASES)
def test_impulses_bit_for_bit(n, s, layout):
    """x is zero but for single 1.0 elements, each in one channel, 7 apart in both directions -- so that no window holds two --, the
    first image's at the corner (0, 0) and on both edges through it; w is an integer in [-8, 8] drawn independently per
    (co, ci, ky, kx), the bias an integer in [-4, 4]: every output is ``w[co][ci][ky][kx] + bias[co]`` of the one impulse in its
    window, or the bias alone -- a wrong tap, channel, stride, K order or fragment order is a wrong integer.  With and without ReLU.
    A second pass takes a bias only float16 holds -- odd integers of magnitude 257 .. 2039 --: every output is then an integer of
    magnitude <= 2047, exact in float16 and in no coarser format, odd ones among them (asserted)."""
    for b, h, wd in SHAPES:
        g = torch.Generator(device='cuda').manual_seed(11 + n + 7 * h)
        w = torch.randint(-8, 9, (n, 3, 7, 7), device='cuda', generator=g).double()
        bias = torch.randint(-4, 5, (n,), device='cuda', generator=g).double()
        x = torch.zeros((b, 3, h, wd), device='cuda', dtype=torch.float64)
        count = 0
        for i in range(b):
            for y in range(i % 7, h, 7):
                for xx in range(2 * i % 7, wd, 7):
                    x[i, count % 3, y, xx] = 1.0
                    count += 1
        assert x[0, :, 0, 0].sum() == 1 and (h < 8 or x[0, :, 7, 0].sum() == 1) and (wd < 8 or x[0, :, 0, 7].sum() == 1)   # corner, edges
        held = _held(x, s)
        assert float(held.max()) == 1 and (float(held.min()) == 0 or h * wd <= 35)
        plain = _conv64(x, w, s) + bias
        assert float(plain.abs().max()) <= 12
        odd = (2 * torch.randint(128, 1020, (n,), device='cuda', generator=g) + 1).double()               # 257 .. 2039
        odd = odd * (2 * torch.randint(0, 2, (n,), device='cuda', generator=g) - 1).double()
        wide = _conv64(x, w, s) + odd
        assert float(odd.abs().min()) >= 257 and float(wide.abs().max()) <= 2047
        assert bool(((wide.abs() > 256) & (wide % 2 == 1)).any()) and not torch.equal(wide.to(torch.bfloat16).double(), wide)
        for relu in (False, True):
            for ref, bias_used in ((plain, bias), (wide, odd)):
                want = ref.clamp(min=0) if relu else ref
                got = _run(x, w, bias_used, s, layout, relu)
                assert torch.equal(_bits(got), _bits(want.to(F16))) and torch.equal(got.double(), want), ((b, h, wd), relu)


def _exact_operands(b, h, wd, n):
    """x in {0, 1}, w in {-1, 0, 1}, bias in [-4, 4], from numpy's generator."""
    rng = np.random.default_rng(1000 + n + h)
    x = rng.integers(0, 2, (b, 3, h, wd))
    w = rng.integers(-1, 2, (n, 3, 7, 7))
    bias = rng.integers(-4, 5, n)
    return x.astype(np.float64), w.astype(np.float64), bias.astype(np.float64)


@pytest.mark.parametrize('n,s,layout', CASES)
def test_dense_exact_sums_bit_for_bit(n, s, layout):
    """Every element of x and w takes part: sums of up to 147 products of {0, 1} x {-1, 0, 1} and a bias in [-4, 4], so
    |sum| <= 147 + 4 < 256 (asserted on the int64 reference), where every integer is a float16 and every partial sum a float32: the
    result must be that integer."""
    for b, h, wd in SHAPES:
        x, w, bias = (torch.from_numpy(t).cuda() for t in _exact_operands(b, h, wd, n))
        want = (_conv64(x, w, s) + bias).long()
        assert int(want.abs().max()) <= 147 + 4 < 256
        got = _run(x, w, bias, s, layout)
        assert torch.equal(_bits(got), _bits(want.to(F16))) and torch.equal(got.long(), want), (b, h, wd)


_RANDOM = {}


def _random_case(b, h, wd, n, s):
    """(x, w, bias, p, S) for the random case, computed once per key and left unchanged: float16-exact operands as float64,
    p = sum x w + bias and S = sum |x w| + |bias| in float64, [M, N]."""
    key = (b, h, wd, n, s)
    if key not in _RANDOM:
        g = torch.Generator(device='cuda').manual_seed(1 + sum(k * 31 ** i for i, k in enumerate(key)))
        x = torch.randn((b, 3, h, wd), device='cuda', generator=g).to(F16).double()
        w = (torch.randn((n, 3, 7, 7), device='cuda', generator=g) * (2.0 / 147) ** 0.5).to(F16).double()
        bias = (torch.randn((n,), device='cuda', generator=g) * 0.5).to(F16).double()
        _RANDOM[key] = (x, w, bias, _conv64(x, w, s) + bias, _conv64(x, w, s, absolute=True) + bias.abs())
    return _RANDOM[key]


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('n,s,layout', CASES)
def test_random_operands_against_float64(n, s, layout, relu):
    """|got - want| <= E + ulp16(want) / 2 for EVERY element: E = 2 (192 + 2) 2^-24 S bounds the float32 accumulation of the kernel's
    192 products (45 of them with a zero weight) and the bias in any order (u = 2^-24 per addition, doubled for adders that
    truncate), S = sum |x w| + |bias|; ulp16(v) = 2^(max(floor(log2 |v|), -14) - 10) is float16's spacing at v, half of it for the one
    rounding; the ReLU's Lipschitz constant is 1.  The operands are scaled so that no result comes near +-65504 (asserted)."""
    for b, h, wd in SHAPES:
        x, w, bias, p, sabs = _random_case(b, h, wd, n, s)
        want = p.clamp(min=0) if relu else p
        got = _run(x, w, bias, s, layout, relu).double()
        e = 2.0 * (192 + 2) * 2.0 ** -24 * sabs
        assert float(p.abs().max()) + float(e.max()) < 60000
        excess = (got - want).abs() - (e + 0.5 * _ulp16(want))
        print('stem7x7 f16 %s c_out=%d s=%d %s relu=%d: max |error| %.3e, largest error - bound %.3e'
              % ((b, h, wd), n, s, layout, relu, float((got - want).abs().max()), float(excess.max())))
        assert float(excess.max()) <= 0.0, (b, h, wd)


def _ulp16(v):
    """float16's spacing at ``v`` (float64 tensor): 2^(max(floor(log2 |v|), -14) - 10); at zero the subnormal spacing 2^-24."""
    exponent = torch.frexp(v.abs())[1].double() - 1                             # floor(log2 |v|); frexp(0) gives exponent 0
    return torch.exp2(torch.where(v == 0, torch.full_like(v, -14.0), exponent.clamp(min=-14.0)) - 10)


def _rms(got, ref):
    return float((got.double() - ref).pow(2).mean().sqrt())


@pytest.mark.parametrize('n,s,layout', CASES)
def test_rms_error_no_worse_than_torch_float16(n, s, layout):
    """The project's relative bar (``test_gpu_conv3x3_bf16.py``, ``test_gpu_unit_gemm.py``): the rms error against float64 is no more
    than 1.05 x that of torch's own float16 ``conv2d`` + bias + ReLU on the same operands."""
    for b, h, wd in SHAPES:
        x, w, bias, p, _ = _random_case(b, h, wd, n, s)
        ref = p.clamp(min=0)
        got = _run(x, w, bias, s, layout, True)
        theirs = torch.relu(torch.nn.functional.conv2d(x.to(F16).contiguous(memory_format=CL), w.to(F16), bias.to(F16), stride=s, padding=3))
        theirs = theirs.permute(0, 2, 3, 1).reshape(-1, n)
        e_got, e_theirs = _rms(got, ref), _rms(theirs, ref)
        print('stem7x7 f16 %s c_out=%d s=%d %s: rms %.3e | torch float16 rms %.3e' % ((b, h, wd), n, s, layout, e_got, e_theirs))
        assert e_got <= 1.05 * e_theirs, ((b, h, wd), e_got, e_theirs)


@pytest.mark.parametrize('n,s,layout', CASES)
def test_padding_and_non_finite_values(n, s, layout):
    """One NaN element at a corner and one Inf element in the interior of x: exactly the outputs whose window holds one of them are
    NaN or Inf, every other output has the bits of the run without them -- the padding is not loaded, so nothing multiplies a zero
    with them.  With the ReLU the NaN stays NaN (a select)."""
    for b, h, wd in SHAPES:
        x, w, bias, _, _ = _random_case(b, h, wd, n, s)
        assert bool((w != 0).all())
        clean = _run(x, w, bias, s, layout)
        assert clean.isfinite().all()
        special = x.clone()
        special[0, 1, 0, 0] = float('nan')
        special[b - 1, 2, h // 2, wd // 2] = float('inf')
        nan_mark = torch.zeros_like(x)
        nan_mark[0, 1, 0, 0] = 1.0
        marks = nan_mark.clone()
        marks[b - 1, 2, h // 2, wd // 2] = 1.0
        held, holds_nan = _held(marks, s) > 0, _held(nan_mark, s) > 0
        assert 0 < int(held.sum()) and (int(held.sum()) < held.numel() or held.numel() <= 35)
        got = _run(special, w, bias, s, layout)
        assert torch.equal(~got.isfinite(), held.unsqueeze(1).expand(-1, n)), (b, h, wd)
        assert got[holds_nan].isnan().all()
        assert torch.equal(_bits(got[~held]), _bits(clean[~held])), (b, h, wd)
        with_relu = _run(special, w, bias, s, layout, True)
        assert with_relu[holds_nan].isnan().all()
        assert torch.equal(_bits(with_relu[~held]), _bits(torch.where(clean < 0, torch.zeros_like(clean), clean)[~held]))


def _centre(n, wv):
    """[N, 3, 7, 7] float64: output channel co reads channel 0 of its centre pixel alone, with the weight ``wv[co]``."""
    w = torch.zeros((n, 3, 7, 7), dtype=torch.float64, device='cuda')
    w[:, 0, 3, 3] = wv
    return w


def _run32(x, w, bias32, s, layout, relu=False):
    """``_run`` with a FLOAT32 bias handed over as it is (the predicate takes one; the kernel's bias is float32 anyway)."""
    from openpifpaf_amd import fused
    conv, xi = _conv_of(w, s), _image(x, layout)
    old, fused.STEM7_F16 = fused.STEM7_F16, True
    try:
        assert fused.stem7x7_bf16_supported(conv, xi, bias32)
    finally:
        fused.STEM7_F16 = old
    out = fused.stem7x7_bias_act_bf16(conv, xi, bias32, relu=relu)
    torch.cuda.synchronize()
    return out.permute(0, 2, 3, 1).reshape(-1, w.shape[0])


# x -> [(w, bias)]: a float16 activation, float16 weights and float32 biases whose accumulator x * w + bias is EXACT in float32 (one
# product of two float16s, one addition whose result has at most 17 significant bits), at float16's edges
EDGES = {
    2.0: [(32752.0, 0.0),                   # 65504, the largest float16
          (32752.0, 15.0),                  # 65519 -> 65504
          (32752.0, 16.0),                  # 65520, the tie -> even -> inf
          (-32752.0, -16.0),                # -65520 -> -inf (ReLU: 0)
          (32752.0, 17.0)],                 # 65521 -> inf
    1.0: [(2047.0, 0.0), (1025.0, 0.0),                                        # odd integers only float16 holds
          (0.0, 2.0 ** -25), (0.0, 2.0 ** -25 + 2.0 ** -40)],                  # half a subnormal unit -> 0, just above -> 1 unit
    3.0: [(683.0, 0.0), (683.0, 2.0)],                                         # 2049 -> 2048 (tie to even), 2051 -> 2052
    2.0 ** -12: [(2.0 ** -12, 0.0), (3 * 2.0 ** -12, 0.0), (1023 * 2.0 ** -12, 0.0),          # k 2^-24: subnormal results
                 (2.0 ** -12, 2.0 ** -25), (3 * 2.0 ** -12, 2.0 ** -25), (2.0 ** -12, -2.0 ** -25),   # ties: 1.5 -> 2, 3.5 -> 4, 0.5 -> 0 units
                 (0.25, -2.0 ** -25)],                                          # 2^-14 - 2^-25: the tie at the smallest normal
}


@pytest.mark.parametrize('n,s,layout', CASES)
def test_the_store_at_the_edges_of_float16(n, s, layout):
    """Per activation value of ``EDGES``: channel 0 of every pixel holds it, output channel co takes the pair ``co % len`` of its
    list -- a centre-tap weight and a float32 bias.  The float32 accumulator is exact (asserted in float64), so the output must be
    ``accumulator.to(torch.float16)`` as the CPU computes it, bit for bit: round to nearest even, beyond 65504 +-inf, subnormal
    results kept.  With the ReLU the negative ones are +0."""
    b, h, wd = SHAPES[1]
    m = b * _out_hw(h, wd, s)[0] * _out_hw(h, wd, s)[1]
    seen = []
    for xv, pairs in EDGES.items():
        rows = torch.tensor(pairs, dtype=torch.float64)[torch.arange(n) % len(pairs)]
        wv, bv = rows[:, 0], rows[:, 1]
        assert torch.equal(wv.to(F16).double(), wv) and float(torch.tensor(xv).to(F16)) == xv
        acc32 = xv * wv.float() + bv.float()
        assert torch.equal(acc32.double(), xv * wv + bv) and torch.equal(bv.float().double(), bv)
        want = acc32.to(F16)                                                    # the CPU's conversion
        seen.append(want)
        x = torch.zeros((b, 3, h, wd), dtype=torch.float64, device='cuda')
        x[:, 0] = xv
        got = _run32(x, _centre(n, wv.cuda()), bv.float().cuda(), s, layout)
        assert torch.equal(_bits(got.cpu()), _bits(want.expand(m, n))), xv
        got = _run32(x, _centre(n, wv.cuda()), bv.float().cuda(), s, layout, True)
        relued = torch.where(acc32 < 0, torch.zeros_like(acc32), acc32).to(F16)
        assert torch.equal(_bits(got.cpu()), _bits(relued.expand(m, n))), xv
    seen = torch.cat(seen)
    assert bool(seen.isinf().any()) and bool(((seen != 0) & (seen.abs() < 2.0 ** -14)).any()) and bool((seen == 65504.0).any())


@pytest.mark.parametrize('n,s,layout', CASES)
def test_subnormal_operands(n, s, layout):
    """A subnormal ACTIVATION 2^-20 against a weight 2^10 contributes its exact 2^-10 (the A operand's subnormals are
    kept).  A subnormal WEIGHT 2^-20 against an activation 2^10: kept (2^-10) or flushed (0) are both accepted, but the same in
    EVERY element; which one is printed."""
    b, h, wd = SHAPES[1]
    ones = torch.ones(n, dtype=torch.float64, device='cuda')
    x = torch.zeros((b, 3, h, wd), dtype=torch.float64, device='cuda')
    x[:, 0] = 2.0 ** -20
    got = _run(x, _centre(n, ones * 2.0 ** 10), None, s, layout)
    assert torch.equal(got.double(), torch.full_like(got, 2.0 ** -10).double())
    x[:, 0] = 2.0 ** 10
    got = _run(x, _centre(n, ones * 2.0 ** -20), None, s, layout).double()
    kept, flushed = bool((got == 2.0 ** -10).all()), bool((got == 0).all())
    print('stem7x7 f16 c_out=%d s=%d %s: a subnormal weight 2^-20 against 2^10 is %s'
          % (n, s, layout, 'KEPT' if kept else 'FLUSHED' if flushed else 'MIXED'))
    assert kept or flushed


def _raw(xi, wk, b32, out_ptr, n, s, relu, x_ptr=None, batch=None, h=None, w=None, strides=None):
    from openpifpaf_amd import _lib
    b0, _, h0, w0 = xi.shape
    sb, sc, sr, sp = xi.stride() if strides is None else strides
    return _lib.lib().opa_stem7x7_act_f16(
        ctypes.c_void_p(xi.data_ptr() if x_ptr is None else x_ptr), sb, sc, sr, sp, ctypes.c_void_p(wk.data_ptr()),
        ctypes.c_void_p(b32.data_ptr()) if b32 is not None else None, ctypes.c_void_p(out_ptr),
        b0 if batch is None else batch, h0 if h is None else h, w0 if w is None else w, n, s, relu, None)


@pytest.mark.parametrize('n,s,layout', CASES)
def test_sentinels_repeatability_and_relu(n, s, layout):
    """The raw entry point writes into a buffer with 4096 sentinel elements on both sides, and they stay; two calls give equal bits;
    relu = 1 is ``where(out < 0, 0, out)`` of the relu = 0 result bit for bit (the select commutes with the rounding); whatever the
    layout -- a cropped view lies among NaN pixels -- the bits are those of the same image made dense channels-last."""
    from openpifpaf_amd import fused
    pad, sentinel = 4096, 12344.0
    for b, h, wd in SHAPES:
        x, w, bias, p, _ = _random_case(b, h, wd, n, s)
        m = p.shape[0]
        wk, b32 = fused.stem7x7_bf16_weight_of(_conv_of(w, s), bias.to(F16))
        xi = _image(x, layout)
        dense = xi.contiguous(memory_format=CL)
        assert torch.equal(_bits(dense), _bits(x.to(F16).contiguous(memory_format=CL)))
        outs = {}
        for image in (xi, dense):
            for relu in (0, 1):
                for again in (0, 1):
                    buf = torch.full((pad + m * n + pad,), sentinel, device='cuda', dtype=F16)
                    assert (buf.data_ptr() + pad * 2) % 16 == 0
                    rc = _raw(image, wk, b32, buf.data_ptr() + pad * 2, n, s, relu)
                    torch.cuda.synchronize()
                    assert rc == 0
                    assert (buf[:pad] == sentinel).all() and (buf[pad + m * n:] == sentinel).all()
                    out = buf[pad:pad + m * n].view(m, n).clone()
                    assert torch.equal(_bits(outs.setdefault(relu, out)), _bits(out)), ((b, h, wd), image is dense, relu, again)
        plain, relued = outs[0], outs[1]
        assert plain.isfinite().all() and bool((plain < 0).any())
        assert torch.equal(_bits(relued), _bits(torch.where(plain < 0, torch.zeros_like(plain), plain)))
        assert torch.equal(_bits(plain), _bits(_run(x, w, bias, s, layout)))             # the launcher hands over the same call


def test_an_empty_call_and_a_refused_one_launch_nothing():
    from openpifpaf_amd import fused
    b, h, wd, n = 2, 7, 5, 64
    x, w, bias, _, _ = _random_case(b, h, wd, n, 1)
    wk, b32 = fused.stem7x7_bf16_weight_of(_conv_of(w, 1), bias.to(F16))
    xi = _image(x, 'cl')
    out = torch.full((b * h * wd * n,), 12344.0, device='cuda', dtype=F16)

    def raw(nn=n, s=1, **kw):
        return _raw(xi, wk, b32, out.data_ptr(), nn, s, 1, **kw)
    assert raw(batch=0) == 0 and raw(h=0) == 0 and raw(w=0) == 0
    for case in (dict(x_ptr=xi.data_ptr() + 1), dict(x_ptr=0), dict(nn=32), dict(nn=0), dict(s=3), dict(s=0), dict(batch=-1),
                 dict(strides=(105, 1, 15, 0)), dict(strides=(105, -1, 15, 3)), dict(strides=(2 ** 31, 1, 15, 3)),
                 dict(batch=2 ** 20, h=2 ** 10, strides=(1, 1, 1, 1))):
        assert raw(**case) != 0, case
    torch.cuda.synchronize()
    assert (out == 12344.0).all()
