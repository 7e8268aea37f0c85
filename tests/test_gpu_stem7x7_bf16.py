"""The bf16 7x7 stem implicit GEMM (csrc/stem7x7_bf16.hip, ``opa_stem7x7_act_bf16``): the RGB stem of a ResNet cast to bfloat16 --
stride 1 or 2, padding 3, the folded bias and the ReLU inside, one rounding at the store, the image read where it lies.  Kernel level:
``(B, h, w)`` = (3, 23, 19) gives M = 1311 rows at stride 1 and 360 at stride 2 (neither a multiple of the 128-row tile; the rows of
one tile span several output rows and images), (2, 7, 5) is less than one tile and its 7-wide window overhangs the 5-wide image on
both sides at once, (1, 1, 1) leaves only the centre tap; ``c_out`` = 64 is one N tile, 128 two; ``x`` is NCHW, channels-last, or a
view cropped out of a larger channels-last image whose other pixels hold NaN.

Known answers are demanded bit for bit: every product and sum of the first two tests is a small integer, exact in float32 and in
bfloat16 whatever the order of summation.  Random operands are held to the float32 accumulation bound of ANY summation order,
doubled (truncating adders), plus half an ulp of bfloat16 -- and to the project's relative bar, 1.05 x the error of torch's own
bfloat16 convolution.  Every reference is float64, formed from 49 shifted products -- never torch's GPU convolution."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

CL = torch.channels_last
BF = torch.bfloat16
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
    """A bfloat16 7x7 convolution with the weight ``w`` [N, 3, 7, 7] (values exact in bfloat16), stride s, padding 3."""
    conv = torch.nn.Conv2d(3, w.shape[0], 7, s, 3, bias=False).cuda().to(BF).requires_grad_(False)
    conv.weight.copy_(w)
    assert torch.equal(conv.weight.double(), w.double())
    return conv


def _image(x, layout):
    """``x`` [B, 3, h, w] (bfloat16-exact values) -> the bfloat16 tensor of these values in ``layout``.  'crop': a view of a
    channels-last [B, 3, h + 5, w + 4] whose other pixels hold NaN."""
    x = x.to(BF)
    if layout == 'nchw':
        return x.contiguous()
    if layout == 'cl':
        return x.contiguous(memory_format=CL)
    b, c, h, w = x.shape
    big = torch.full((b, c, h + 5, w + 4), float('nan'), dtype=BF, device=x.device).contiguous(memory_format=CL)
    view = big[:, :, 2:2 + h, 1:1 + w]
    view.copy_(x)
    assert not view.is_contiguous() and not view.is_contiguous(memory_format=CL) or h * w == 1
    return view


def _run(x, w, bias, s, layout, relu=False):
    """``x`` [B, 3, h, w], ``w`` [N, 3, 7, 7], ``bias`` [N] or None (all bfloat16-exact) -> [M, N] bfloat16 through the launcher."""
    from openpifpaf_amd import fused
    b, _, h, wd = x.shape
    n = w.shape[0]
    ho, wo = _out_hw(h, wd, s)
    conv, xi = _conv_of(w, s), _image(x, layout)
    bi = None if bias is None else bias.to(BF)
    old, fused.STEM7_BF16 = fused.STEM7_BF16, True
    try:
        assert fused.stem7x7_bf16_supported(conv, xi, bi)
    finally:
        fused.STEM7_BF16 = old
    out = fused.stem7x7_bias_act_bf16(conv, xi, bi, relu=relu)
    torch.cuda.synchronize()
    assert out.dtype == BF and out.is_contiguous(memory_format=CL) and tuple(out.shape) == (b, n, ho, wo)
    return out.permute(0, 2, 3, 1).reshape(-1, n)


@pytest.mark.parametrize('n,s,layout', CASES)
def test_impulses_bit_for_bit(n, s, layout):
    """x is zero but for single 1.0 elements, each in one channel, 7 apart in both directions -- so that no window holds two --, the
    first image's at the corner (0, 0) and on both edges through it; w is an integer in [-8, 8] drawn independently per
    (co, ci, ky, kx), the bias an integer in [-4, 4]: every output is ``w[co][ci][ky][kx] + bias[co]`` of the one impulse in its
    window, or the bias alone -- a wrong tap, channel, stride, K order or fragment order is a wrong integer.  With and without ReLU."""
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
        for relu in (False, True):
            want = plain.clamp(min=0) if relu else plain
            got = _run(x, w, bias, s, layout, relu)
            assert torch.equal(_bits(got), _bits(want.to(BF))) and torch.equal(got.double(), want), ((b, h, wd), relu)


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
    |sum| <= 147 + 4 < 256 (asserted on the int64 reference), where every integer is a bfloat16 and every partial sum a float32: the
    result must be that integer."""
    for b, h, wd in SHAPES:
        x, w, bias = (torch.from_numpy(t).cuda() for t in _exact_operands(b, h, wd, n))
        want = (_conv64(x, w, s) + bias).long()
        assert int(want.abs().max()) <= 147 + 4 < 256
        got = _run(x, w, bias, s, layout)
        assert torch.equal(_bits(got), _bits(want.to(BF))) and torch.equal(got.long(), want), (b, h, wd)


_RANDOM = {}


def _random_case(b, h, wd, n, s):
    """(x, w, bias, p, S) for the random case, computed once per key and left unchanged: bfloat16-exact operands as float64,
    p = sum x w + bias and S = sum |x w| + |bias| in float64, [M, N]."""
    key = (b, h, wd, n, s)
    if key not in _RANDOM:
        g = torch.Generator(device='cuda').manual_seed(1 + sum(k * 31 ** i for i, k in enumerate(key)))
        x = torch.randn((b, 3, h, wd), device='cuda', generator=g).to(BF).double()
        w = (torch.randn((n, 3, 7, 7), device='cuda', generator=g) * (2.0 / 147) ** 0.5).to(BF).double()
        bias = (torch.randn((n,), device='cuda', generator=g) * 0.5).to(BF).double()
        _RANDOM[key] = (x, w, bias, _conv64(x, w, s) + bias, _conv64(x, w, s, absolute=True) + bias.abs())
    return _RANDOM[key]


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('n,s,layout', CASES)
def test_random_operands_against_float64(n, s, layout, relu):
    """|got - want| <= E + 2^-8 (|want| + E) for EVERY element: E = 2 (147 + 1) 2^-24 S bounds the float32 accumulation of the 147
    products and the bias in any order (u = 2^-24 per addition, doubled for adders that truncate), S = sum |x w| + |bias|; 2^-8 is
    half an ulp of bfloat16, relative, for the one rounding; the ReLU's Lipschitz constant is 1."""
    for b, h, wd in SHAPES:
        x, w, bias, p, sabs = _random_case(b, h, wd, n, s)
        want = p.clamp(min=0) if relu else p
        got = _run(x, w, bias, s, layout, relu).double()
        e = 2.0 * (147 + 1) * 2.0 ** -24 * sabs
        excess = (got - want).abs() - (e + 2.0 ** -8 * (want.abs() + e))
        print('stem7x7 bf16 %s c_out=%d s=%d %s relu=%d: max |error| %.3e, largest error - bound %.3e'
              % ((b, h, wd), n, s, layout, relu, float((got - want).abs().max()), float(excess.max())))
        assert float(excess.max()) <= 0.0, (b, h, wd)


def _rms(got, ref):
    return float((got.double() - ref).pow(2).mean().sqrt())


@pytest.mark.parametrize('n,s,layout', CASES)
def test_rms_error_no_worse_than_torch_bfloat16(n, s, layout):
    """The project's relative bar (``test_gpu_conv3x3_bf16.py``, ``test_gpu_unit_gemm.py``): the rms error against float64 is no more
    than 1.05 x that of torch's own bfloat16 ``conv2d`` + bias + ReLU on the same operands."""
    for b, h, wd in SHAPES:
        x, w, bias, p, _ = _random_case(b, h, wd, n, s)
        ref = p.clamp(min=0)
        got = _run(x, w, bias, s, layout, True)
        theirs = torch.relu(torch.nn.functional.conv2d(x.to(BF).contiguous(memory_format=CL), w.to(BF), bias.to(BF), stride=s, padding=3))
        theirs = theirs.permute(0, 2, 3, 1).reshape(-1, n)
        e_got, e_theirs = _rms(got, ref), _rms(theirs, ref)
        print('stem7x7 bf16 %s c_out=%d s=%d %s: rms %.3e | torch bfloat16 rms %.3e' % ((b, h, wd), n, s, layout, e_got, e_theirs))
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


def _raw(xi, wk, b32, out_ptr, n, s, relu, x_ptr=None, batch=None, h=None, w=None, strides=None):
    from openpifpaf_amd import _lib
    b0, _, h0, w0 = xi.shape
    sb, sc, sr, sp = xi.stride() if strides is None else strides
    return _lib.lib().opa_stem7x7_act_bf16(
        ctypes.c_void_p(xi.data_ptr() if x_ptr is None else x_ptr), sb, sc, sr, sp, ctypes.c_void_p(wk.data_ptr()),
        ctypes.c_void_p(b32.data_ptr()) if b32 is not None else None, ctypes.c_void_p(out_ptr),
        b0 if batch is None else batch, h0 if h is None else h, w0 if w is None else w, n, s, relu, None)


@pytest.mark.parametrize('n,s,layout', CASES)
def test_sentinels_repeatability_and_relu(n, s, layout):
    """The raw entry point writes into a buffer with 4096 sentinel elements on both sides, and they stay; two calls give equal bits;
    relu = 1 is ``where(out < 0, 0, out)`` of the relu = 0 result bit for bit (the select commutes with the rounding); whatever the
    layout -- a cropped view lies among NaN pixels -- the bits are those of the same image made dense channels-last."""
    from openpifpaf_amd import fused
    pad, sentinel = 4096, 12345.0
    for b, h, wd in SHAPES:
        x, w, bias, p, _ = _random_case(b, h, wd, n, s)
        m = p.shape[0]
        wk, b32 = fused.stem7x7_bf16_weight_of(_conv_of(w, s), bias.to(BF))
        xi = _image(x, layout)
        dense = xi.contiguous(memory_format=CL)
        assert torch.equal(_bits(dense), _bits(x.to(BF).contiguous(memory_format=CL)))
        outs = {}
        for image in (xi, dense):
            for relu in (0, 1):
                for again in (0, 1):
                    buf = torch.full((pad + m * n + pad,), sentinel, device='cuda', dtype=BF)
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
    wk, b32 = fused.stem7x7_bf16_weight_of(_conv_of(w, 1), bias.to(BF))
    xi = _image(x, 'cl')
    out = torch.full((b * h * wd * n,), 12345.0, device='cuda', dtype=BF)

    def raw(nn=n, s=1, **kw):
        return _raw(xi, wk, b32, out.data_ptr(), nn, s, 1, **kw)
    assert raw(batch=0) == 0 and raw(h=0) == 0 and raw(w=0) == 0
    for case in (dict(x_ptr=xi.data_ptr() + 1), dict(x_ptr=0), dict(nn=32), dict(nn=0), dict(s=3), dict(s=0), dict(batch=-1),
                 dict(strides=(105, 1, 15, 0)), dict(strides=(105, -1, 15, 3)), dict(strides=(2 ** 31, 1, 15, 3)),
                 dict(batch=2 ** 20, h=2 ** 10, strides=(1, 1, 1, 1))):
        assert raw(**case) != 0, case
    torch.cuda.synchronize()
    assert (out == 12345.0).all()
