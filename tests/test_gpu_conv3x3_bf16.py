"""The bf16 3x3 implicit GEMM (csrc/conv3x3_bf16.hip, ``opa_conv3x3_act_bf16``): the 3x3 convolutions of a ResNet cast to bfloat16 --
stride 1 or 2, dilation = padding 1, 2 or 4, the folded bias, a residual and the ReLU inside, one rounding at the store.  Kernel
level: ``(B, h, w)`` = (3, 23, 19) gives M = 1311 rows at stride 1 and 360 at stride 2 (neither a multiple of the 128-row tile),
(2, 7, 5) is less than one tile, and (1, 3, 3) at dilation 4 leaves only the centre tap inside the image; ``(c_in, c_out)`` =
(64, 64) is one K-step per tap and one 64-wide N tile, (128, 192) two K-steps per tap and three N tiles.

Known answers are demanded bit for bit: every product and sum of the first two tests is a small integer, exact in float32 and in
bfloat16 whatever the order of summation.  Random operands are held to the float32 accumulation bound of ANY summation order,
doubled (truncating adders), plus half an ulp of bfloat16 -- and to the project's relative bar, 1.05 x the error of torch's own
bfloat16 convolution.  Every reference is float64, formed from nine shifted matrix products -- never torch's GPU convolution."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

CL = torch.channels_last
BF = torch.bfloat16
SHAPES = [(3, 23, 19), (2, 7, 5), (1, 3, 3)]
CHANNELS = [(64, 64), (128, 192)]
MODES = [(1, 1), (2, 1), (1, 2), (1, 4)]                 # (stride, dilation)
CASES = [pytest.param(c, n, s, d, id='c%d-n%d-s%d-d%d' % (c, n, s, d)) for c, n in CHANNELS for s, d in MODES]
assert 3 * 23 * 19 == 1311 and 1311 % 128 != 0 and 3 * 12 * 10 == 360 and 360 % 128 != 0


def _bits(t):
    return t.contiguous().view(torch.int16)


def _out_hw(h, w, s):
    return (h - 1) // s + 1, (w - 1) // s + 1


def _taps(x, s, d):
    """``x`` [B, h, w, C] -> the nine shifted views [B, ho, wo, C] (tap 3 ky + kx; zeros in the padding), the plain definition."""
    b, h, w, c = x.shape
    ho, wo = _out_hw(h, w, s)
    xp = torch.zeros((b, h + 2 * d, w + 2 * d, c), dtype=x.dtype, device=x.device)
    xp[:, d:d + h, d:d + w] = x
    return [xp[:, ky * d:ky * d + s * (ho - 1) + 1:s, kx * d:kx * d + s * (wo - 1) + 1:s] for ky in range(3) for kx in range(3)]


def _conv64(x, w, s, d, absolute=False):
    """sum over the taps of [M, C] @ [C, N] in float64 -> [M, N]; ``absolute``: of the magnitudes (the bound's S).  ``w`` [N, 3, 3, C]."""
    x, w = x.double(), w.double()
    if absolute:
        x, w = x.abs(), w.abs()
    n = w.shape[0]
    total = None
    for tap, view in enumerate(_taps(x, s, d)):
        part = view.reshape(-1, x.shape[3]) @ w[:, tap // 3, tap % 3].t()
        total = part if total is None else total + part
    return total.reshape(-1, n)


def _conv_of(w, s, d):
    """A bfloat16 3x3 convolution with the weight ``w`` [N, 3, 3, C] (values exact in bfloat16), stride s, dilation = padding d."""
    n, c = w.shape[0], w.shape[3]
    conv = torch.nn.Conv2d(c, n, 3, s, d, dilation=d, bias=False).cuda().to(BF).requires_grad_(False)
    conv.weight.copy_(w.permute(0, 3, 1, 2))
    assert torch.equal(conv.weight.double(), w.permute(0, 3, 1, 2).double())
    return conv


def _image(rows_nhwc):
    """[B, h, w, C] (contiguous) -> the [B, C, h, w] channels-last view of the same memory."""
    return rows_nhwc.contiguous().permute(0, 3, 1, 2)


def _run(x, w, bias, s, d, residual=None, relu=False):
    """``x`` [B, h, w, C], ``w`` [N, 3, 3, C], ``bias`` [N] or None, ``residual`` [M, N] or None (all bfloat16-exact) -> [M, N] bfloat16."""
    from openpifpaf_amd import fused
    b, h, wd, _ = x.shape
    n = w.shape[0]
    ho, wo = _out_hw(h, wd, s)
    conv, xi = _conv_of(w, s, d), _image(x.to(BF))
    bi = None if bias is None else bias.to(BF)
    ri = None if residual is None else _image(residual.to(BF).reshape(b, ho, wo, n))
    old, fused.CONV3_BF16 = fused.CONV3_BF16, True
    try:
        assert fused.conv3x3_bf16_supported(conv, xi, bi, ri)
    finally:
        fused.CONV3_BF16 = old
    out = fused.conv3x3_bias_act_bf16(conv, xi, bi, ri, relu=relu)
    torch.cuda.synchronize()
    assert out.dtype == BF and out.is_contiguous(memory_format=CL) and tuple(out.shape) == (b, n, ho, wo)
    return out.permute(0, 2, 3, 1).reshape(-1, n)


@pytest.mark.parametrize('c,n,s,d', CASES)
def test_tap_selection_bit_for_bit(c, n, s, d):
    """Pixel p (linear index) holds 1.0 at channel p mod c_in and 2.0 at (7 p + 3) mod c_in (the 2.0 wins where they coincide); w, the
    bias and the residual are integers in [-8, 8]: every output is an integer of magnitude <= 9 * 24 + 8 + 8 = 232, exact in float32
    and bfloat16 in any order -- a wrong tap, pixel, channel, padding decision or fragment order is a wrong integer.  With and without
    the residual, with and without the ReLU."""
    for b, h, wd in SHAPES:
        g = torch.Generator(device='cuda').manual_seed(11 + c + n + 7 * h)
        w = torch.randint(-8, 9, (n, 3, 3, c), device='cuda', generator=g).double()
        bias = torch.randint(-8, 9, (n,), device='cuda', generator=g).double()
        p = torch.arange(b * h * wd, device='cuda')
        x = torch.zeros((b * h * wd, c), device='cuda', dtype=torch.float64)
        x[p, p % c] = 1.0
        x[p, (7 * p + 3) % c] = 2.0
        x = x.reshape(b, h, wd, c)
        ho, wo = _out_hw(h, wd, s)
        res = torch.randint(-8, 9, (b * ho * wo, n), device='cuda', generator=g).double()
        plain = _conv64(x, w, s, d) + bias
        assert float(plain.abs().max()) <= 224 and float((plain + res).abs().max()) <= 232
        for residual in (None, res):
            for relu in (False, True):
                want = plain if residual is None else plain + residual
                want = want.clamp(min=0) if relu else want
                got = _run(x, w, bias, s, d, residual, relu)
                assert torch.equal(want.to(BF).double(), want)                      # (an integer <= 256: a bfloat16)
                assert torch.equal(_bits(got), _bits(want.to(BF))), ((b, h, wd), residual is not None, relu)


def _exact_operands(b, h, wd, c, n):
    """x in {0, 1}, w in {-1, 0, 1}, bias in [-4, 4], from numpy's generator (so that the bound below can be checked without a GPU)."""
    rng = np.random.default_rng(1000 * c + n)
    x = rng.integers(0, 2, (b, h, wd, c))
    w = rng.integers(-1, 2, (n, 3, 3, c))
    bias = rng.integers(-4, 5, n)
    return x.astype(np.float64), w.astype(np.float64), bias.astype(np.float64)


@pytest.mark.parametrize('c,n,s,d', CASES)
def test_dense_exact_sums_bit_for_bit(c, n, s, d):
    """Every element of x and w takes part: sums of up to 9 c_in products of {0, 1} x {-1, 0, 1}.  The int64 reference stays within
    +-256 (asserted; checked with numpy for (3, 23, 19) and this seed: the largest magnitudes are 59 / 54 / 58 / 56 for (64, 64) and
    85 / 81 / 89 / 83 for (128, 192) over the four (stride, dilation) pairs), where every integer is a bfloat16 and every partial sum
    a float32: the result must be that integer."""
    for b, h, wd in SHAPES:
        x, w, bias = (torch.from_numpy(t).cuda() for t in _exact_operands(b, h, wd, c, n))
        want = (_conv64(x, w, s, d) + bias).long()
        assert int(want.abs().max()) <= 256
        got = _run(x, w, bias, s, d)
        assert torch.equal(_bits(got), _bits(want.to(BF))) and torch.equal(got.long(), want), (b, h, wd)


_RANDOM = {}


def _random_case(b, h, wd, c, n, s, d):
    """(x, w, bias, residual, p, S) for the random case, computed once per key and left unchanged: bfloat16-exact operands as float64,
    p = sum x w + bias and S = sum |x w| + |bias| in float64, [M, N]; the residual's share is added by the caller."""
    key = (b, h, wd, c, n, s, d)
    if key not in _RANDOM:
        g = torch.Generator(device='cuda').manual_seed(1 + sum(k * 31 ** i for i, k in enumerate(key)))
        x = torch.randn((b, h, wd, c), device='cuda', generator=g).to(BF).double()
        w = (torch.randn((n, 3, 3, c), device='cuda', generator=g) * (2.0 / (9 * c)) ** 0.5).to(BF).double()
        bias = (torch.randn((n,), device='cuda', generator=g) * 0.5).to(BF).double()
        ho, wo = _out_hw(h, wd, s)
        res = torch.randn((b * ho * wo, n), device='cuda', generator=g).to(BF).double()
        _RANDOM[key] = (x, w, bias, res, _conv64(x, w, s, d) + bias, _conv64(x, w, s, d, absolute=True) + bias.abs())
    return _RANDOM[key]


@pytest.mark.parametrize('with_residual,relu', [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize('c,n,s,d', CASES)
def test_random_operands_against_float64(c, n, s, d, with_residual, relu):
    """|got - want| <= E + 2^-8 (|want| + E) for EVERY element: E = 2 (9 c_in + 2) 2^-24 S bounds the float32 accumulation of the
    9 c_in products, the bias and the residual in any order (u = 2^-24 per addition, doubled for adders that truncate), S = sum |x w|
    + |bias| (+ |residual|); 2^-8 is half an ulp of bfloat16, relative, for the one rounding; the ReLU's Lipschitz constant is 1."""
    for b, h, wd in SHAPES:
        x, w, bias, res, p, sabs = _random_case(b, h, wd, c, n, s, d)
        if with_residual:
            p, sabs = p + res, sabs + res.abs()
        want = p.clamp(min=0) if relu else p
        got = _run(x, w, bias, s, d, res if with_residual else None, relu).double()
        e = 2.0 * (9 * c + 2) * 2.0 ** -24 * sabs
        excess = (got - want).abs() - (e + 2.0 ** -8 * (want.abs() + e))
        print('conv3x3 bf16 %s c_in=%d c_out=%d s=%d d=%d residual=%d relu=%d: max |error| %.3e, largest error - bound %.3e'
              % ((b, h, wd), c, n, s, d, with_residual, relu, float((got - want).abs().max()), float(excess.max())))
        assert float(excess.max()) <= 0.0, (b, h, wd)


def _rms(got, ref):
    return float((got.double() - ref).pow(2).mean().sqrt())


@pytest.mark.parametrize('c,n,s,d', CASES)
def test_rms_error_no_worse_than_torch_bfloat16(c, n, s, d):
    """The project's relative bar (``test_gpu_unit_gemm.py``, ``test_gpu_gemm_x3.py``): the rms error against float64 is no more than
    1.05 x that of torch's own bfloat16 ``conv2d`` + bias + ReLU on the same operands."""
    for b, h, wd in SHAPES:
        x, w, bias, _, p, _ = _random_case(b, h, wd, c, n, s, d)
        ref = p.clamp(min=0)
        got = _run(x, w, bias, s, d, None, True)
        conv = _conv_of(w, s, d)
        theirs = torch.relu(torch.nn.functional.conv2d(_image(x.to(BF)), conv.weight, bias.to(BF), stride=s, padding=d, dilation=d))
        theirs = theirs.permute(0, 2, 3, 1).reshape(-1, n)
        e_got, e_theirs = _rms(got, ref), _rms(theirs, ref)
        print('conv3x3 bf16 %s c_in=%d c_out=%d s=%d d=%d: rms %.3e | torch bfloat16 rms %.3e' % ((b, h, wd), c, n, s, d, e_got, e_theirs))
        assert e_got <= 1.05 * e_theirs, ((b, h, wd), e_got, e_theirs)


@pytest.mark.parametrize('c,n,s,d', CASES)
def test_padding_and_non_finite_values(c, n, s, d):
    """One NaN pixel at a corner and one Inf pixel in the interior of x: exactly the outputs whose window holds one of them are NaN or
    Inf, every other output has the bits of the run without them -- the padding is not loaded, so nothing multiplies a zero with
    them.  With the ReLU the NaN stays NaN (a select)."""
    for b, h, wd in SHAPES:
        x, w, bias, _, _, _ = _random_case(b, h, wd, c, n, s, d)
        clean = _run(x, w, bias, s, d)
        assert clean.isfinite().all()
        special = x.clone()
        special[0, 0, 0, 3] = float('nan')
        special[b - 1, h // 2, wd // 2, 5] = float('inf')
        marks = torch.zeros_like(x)
        marks[0, 0, 0, 3], marks[b - 1, h // 2, wd // 2, 5] = 1.0, 1.0
        held = sum(view.reshape(-1, c).sum(1) for view in _taps(marks, s, d)) > 0      # [M]: the window holds a special pixel
        nan_mark = torch.zeros_like(x)
        nan_mark[0, 0, 0, 3] = 1.0
        holds_nan = sum(view.reshape(-1, c).sum(1) for view in _taps(nan_mark, s, d)) > 0
        assert 0 < int(held.sum()) and (int(held.sum()) < held.numel() or held.numel() <= 9)
        got = _run(special, w, bias, s, d)
        assert torch.equal(~got.isfinite(), held.unsqueeze(1).expand(-1, n)), (b, h, wd)
        assert got[holds_nan].isnan().all()
        assert torch.equal(_bits(got[~held]), _bits(clean[~held])), (b, h, wd)
        with_relu = _run(special, w, bias, s, d, None, True)
        assert with_relu[holds_nan].isnan().all()
        assert torch.equal(_bits(with_relu[~held]), _bits(torch.where(clean < 0, torch.zeros_like(clean), clean)[~held]))


def _raw(x, w9, b32, res, out_ptr, b, h, wd, c, n, s, d, relu):
    from openpifpaf_amd import _lib
    return _lib.lib().opa_conv3x3_act_bf16(
        ctypes.c_void_p(x), ctypes.c_void_p(w9.data_ptr()), ctypes.c_void_p(b32.data_ptr()) if b32 is not None else None,
        ctypes.c_void_p(res.data_ptr()) if res is not None else None, ctypes.c_void_p(out_ptr), b, h, wd, c, n, s, d, relu, None)


@pytest.mark.parametrize('c,n,s,d', CASES)
def test_sentinels_repeatability_and_relu(c, n, s, d):
    """The raw entry point writes into a buffer with 4096 sentinel elements on both sides, and they stay; two calls give equal bits;
    relu = 1 is ``where(out < 0, 0, out)`` of the relu = 0 result bit for bit (the select commutes with the rounding)."""
    from openpifpaf_amd import fused
    pad, sentinel = 4096, 12345.0
    for b, h, wd in SHAPES:
        x, w, bias, res, _, _ = _random_case(b, h, wd, c, n, s, d)
        m = res.shape[0]
        w9, b32 = fused.conv3x3_bf16_weight_of(_conv_of(w, s, d), bias.to(BF))
        xb, rb = x.to(BF).contiguous(), res.to(BF).contiguous()
        outs = {}
        for residual in (None, rb):
            for relu in (0, 1):
                for again in (0, 1):
                    buf = torch.full((pad + m * n + pad,), sentinel, device='cuda', dtype=BF)
                    assert (buf.data_ptr() + pad * 2) % 16 == 0
                    rc = _raw(xb.data_ptr(), w9, b32, residual, buf.data_ptr() + pad * 2, b, h, wd, c, n, s, d, relu)
                    torch.cuda.synchronize()
                    assert rc == 0
                    assert (buf[:pad] == sentinel).all() and (buf[pad + m * n:] == sentinel).all()
                    out = buf[pad:pad + m * n].view(m, n).clone()
                    assert torch.equal(_bits(outs.setdefault((residual is not None, relu), out)), _bits(out))
        for with_residual in (False, True):
            plain, relued = outs[(with_residual, 0)], outs[(with_residual, 1)]
            assert plain.isfinite().all() and bool((plain < 0).any())
            assert torch.equal(_bits(relued), _bits(torch.where(plain < 0, torch.zeros_like(plain), plain)))
        assert torch.equal(_bits(outs[(False, 0)]), _bits(_run(x, w, bias, s, d)))       # the launcher hands over the same call


def test_an_empty_call_and_a_refused_one_launch_nothing():
    from openpifpaf_amd import fused
    b, h, wd, c, n = 2, 7, 5, 64, 64
    x, w, bias, _, _, _ = _random_case(b, h, wd, c, n, 1, 1)
    w9, b32 = fused.conv3x3_bf16_weight_of(_conv_of(w, 1, 1), bias.to(BF))
    xb = x.to(BF).contiguous()
    out = torch.full((b * h * wd * n,), 12345.0, device='cuda', dtype=BF)

    def raw(x_ptr=xb.data_ptr(), batch=b, hh=h, ww=wd, cc=c, nn=n, s=1, d=1):
        return _raw(x_ptr, w9, b32, None, out.data_ptr(), batch, hh, ww, cc, nn, s, d, 1)
    assert raw(batch=0) == 0 and raw(hh=0) == 0 and raw(ww=0) == 0
    for case in (dict(x_ptr=xb.data_ptr() + 2), dict(x_ptr=0), dict(cc=63), dict(nn=32), dict(s=3), dict(d=3), dict(s=2, d=2), dict(batch=-1),
                 dict(batch=2 ** 20, hh=2 ** 10)):
        assert raw(**case) != 0, case
    torch.cuda.synchronize()
    assert (out == 12345.0).all()
