"""The depthwise stencil in FLOAT16 (``csrc/dwconv.hip``: ``DwVec<_Float16, V>``, ``opa_dwconv_actp_f16``): the depthwise convolutions of
a ShuffleNetV2K cast with ``.half()``.  The shapes are the smallest at which each path can go wrong, in the notation of the ``_dw``
cases of ``pointwise_common.py``: 8 / 6 / 5 channels (V = 4 / 2 / 1: 8-, 4- and 2-byte loads and stores), an input narrower than the
window, widths that are no multiple of the 4-pixel strip, pixel strides above C with a slice offset on either side, every
(K, S) of 3 / 5 x 1 / 2, the 7 x 7 window, dilation 2 and 4, more than one block along x.

Integer operands whose sums stay within 2048 -- every such integer is a float16 and every partial sum a float32 -- are demanded bit for
bit.  Random operands are held to the DERIVED bound of ``test_gpu_shufflenetv2k_options.dw_reference`` for a float32 accumulation in
any order (``gamma_n (sum |x| |w| + |b|)``, ``n = k * k + 1``, ``u = 2^-24``; ReLU and the clipped ReLU are 1-Lipschitz; hardswish
``1.5 bound + 4 u |ref|``) plus the ONE float16 rounding, ``2^-11 (|ref| + bound)``.  The output lies in a sentinel buffer: in front
of it, behind it and in the channels of a wider pixel that are not its own nothing may be written."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from openpifpaf_amd import _lib, fused

import pointwise_common as pc

pytestmark = pytest.mark.gpu

F16 = torch.float16
CL = torch.channels_last
_vp = ctypes.c_void_p
CAP = 0.5                                      # of the clipped ReLU: inside the range of the outputs, so that it clips


def _case(k, s, B, H, W, C, d=1, **layout):
    return pc._dw('float16', k, s, B, H, W, C, **layout) + (d,)


CASES = (
    # V = 4 / 2 / 1 x every (K, S) of 3 / 5 x 1 / 2; B 1 and 3; widths 13, 7, 10: no multiples of the strip
    [_case(k, s, (1, 3)[i % 2], H, W, C) for i, (k, s) in enumerate(pc.DW_KS) for C, (H, W) in ((8, (9, 13)), (6, (6, 7)), (5, (5, 10)))] +
    [
        # inputs narrower than the window: 3 x 1 and 1 x 3
        _case(5, 1, 3, 3, 1, 8), _case(3, 1, 1, 1, 3, 5), _case(5, 2, 1, 1, 3, 6),
        # more than one block along x
        _case(5, 1, 1, 2, 13, 348),
        # pixel strides above C: V from the input's stride and pointer (8, 4 and 2 bytes off a 16-byte boundary), the second half
        _case(3, 2, 1, 5, 6, 8, xs=11), _case(5, 1, 1, 5, 6, 8, xs=10), _case(5, 2, 3, 5, 6, 8, xs=16, x_off=8),
        _case(3, 1, 1, 5, 6, 8, xs=16, x_off=4), _case(5, 2, 1, 5, 6, 8, xs=16, x_off=2), _case(5, 1, 1, 5, 6, 8, xs=16, x_off=1),
        # ... and from the output's: the other half of a sliced output holds the sentinel
        _case(5, 1, 1, 5, 6, 8, os=10), _case(3, 2, 1, 5, 6, 8, os=11), _case(5, 2, 1, 5, 6, 8, os=16, o_off=2),
        _case(3, 1, 3, 5, 6, 8, os=16, o_off=1), _case(3, 2, 3, 5, 7, 8, os=16), _case(5, 1, 1, 4, 5, 8, os=24, o_off=8),
        _case(5, 1, 3, 5, 6, 8, xs=16, x_off=8, os=16, o_off=8),
        # no bias
        _case(5, 2, 1, 6, 5, 6, bias=False), _case(3, 1, 3, 4, 4, 8, xs=16, x_off=8, bias=False),
        # 7 x 7, and an input smaller than it
        _case(7, 1, 1, 9, 13, 8), _case(7, 2, 3, 6, 7, 6), _case(7, 1, 1, 2, 2, 5), _case(7, 2, 1, 5, 10, 5),
    ] +
    # dilation 2 and 4 (stride 1), each window; 4 x 9 is smaller than the dilated window
    [_case(k, 1, (1, 3)[i % 2], H, W, C, d=d) for i, (k, d) in enumerate((k, d) for k in (3, 5, 7) for d in (2, 4))
     for C, (H, W) in ((8, (4, 9)), (6, (13, 11)), (5, (3, 5)))])


def _id(case):
    dtype, k, s, B, H, W, C, xs, x_off, os_, o_off, has_bias, d = case
    return 'k%ds%dd%d-%dx%dx%dx%d-xs%d+%d-os%d+%d-b%d' % (k, s, d, B, H, W, C, xs, x_off, os_, o_off, has_bias)


def _regime(case):
    """V of the launch, as ``pointwise_common.dwconv_regime`` derives it (2-byte elements)."""
    return pc.dwconv_regime(case[:12])[0]


def test_the_cases_cover_every_vector_width_and_window():
    assert {_regime(c) for c in CASES} == {4, 2, 1}
    assert {(c[1], c[2], c[12]) for c in CASES} == {(k, s, 1) for k in (3, 5, 7) for s in (1, 2)} | {(k, 1, d) for k in (3, 5, 7) for d in (2, 4)}
    for v in (4, 2, 1):                        # each width with a slice on the input side and on the output side
        assert any(_regime(c) == v and c[7] > c[6] for c in CASES) and any(_regime(c) == v and c[9] > c[6] for c in CASES), v


def _inputs(case, seed=0):
    """-> (x [B, C, H, W], w_taps [k*k, C], bias [C] or None) on the CPU, rounded to float16: ``pointwise_common.dw_inputs`` with a
    power of two per channel from 2^-4 to 2^4, inside float16's range."""
    dtype, k, s, B, H, W, C, xs, x_off, os_, o_off, has_bias, d = case
    g = torch.Generator().manual_seed(seed)
    scale = torch.tensor([2.0 ** ((7 * c) % 9 - 4) for c in range(C)], dtype=torch.float64)
    x = (torch.randn((B, C, H, W), generator=g, dtype=torch.float64) * scale.view(1, C, 1, 1)).to(F16)
    w = (torch.randn((k * k, C), generator=g, dtype=torch.float64) / k).to(F16)
    b = (torch.randn((C,), generator=g, dtype=torch.float64) * scale).to(F16) if has_bias else None
    assert bool(x.isfinite().all())
    return x, w, b


def _reference(x, w_taps, bias, k, s, act, d):
    """Float64 convolution of the operands as stored, and the bound of the module docstring -> (ref, bound), float64."""
    C = x.shape[1]
    w4 = w_taps.double().t().reshape(C, 1, k, k)
    b = None if bias is None else bias.double()
    pad = k // 2 * d
    ref = F.conv2d(x.double(), w4, b, stride=s, padding=pad, dilation=d, groups=C)
    mag = F.conv2d(x.double().abs(), w4.abs(), None if b is None else b.abs(), stride=s, padding=pad, dilation=d, groups=C)
    n, u = k * k + 1, 2.0 ** -24
    bound = n * u / (1 - n * u) * mag
    if act == 1:
        ref = ref.clamp_min(0)
    elif act == 2:
        ref = ref * (ref + 3).clamp(0, 6) / 6
        bound = 1.5 * bound + 4 * u * ref.abs()
    elif act == 4:
        ref = ref.clamp(0, CAP)
    return ref, bound + 2.0 ** -11 * (ref.abs() + bound)


def _run(case, x, w, b, act, expect=0):
    """``opa_dwconv_actp_f16`` on the case's layout: the input inside a NaN-filled pixel grid, the output inside a sentinel buffer.
    -> (the output [B, C, Ho, Wo] on the CPU, the input view); everything outside the output's own elements was checked to hold the
    sentinel -- in front, behind, and between the pixels of a sliced output."""
    dtype, k, s, B, H, W, C, xs, x_off, os_, o_off, has_bias, d = case
    Ho, Wo = fused.dwconv_out_hw(H, W, k, s, d)
    xbuf = torch.full((B * H * W * xs + 2 * pc.PAD,), float('nan'), dtype=F16, device='cuda')
    xv = xbuf.as_strided((B, C, H, W), (H * W * xs, 1, W * xs, xs), pc.PAD + x_off)
    xv.copy_(x)
    obuf = torch.full((B * Ho * Wo * os_ + 2 * pc.PAD,), pc.SENTINEL, dtype=F16, device='cuda')
    ov = obuf.as_strided((B, C, Ho, Wo), (Ho * Wo * os_, 1, Wo * os_, os_), pc.PAD + o_off)
    wg, bg = w.cuda(), (b.cuda() if b is not None else None)
    assert xbuf.data_ptr() % 256 == 0 and obuf.data_ptr() % 256 == 0 and wg.data_ptr() % 16 == 0
    rc = _lib.lib().opa_dwconv_actp_f16(_vp(xv.data_ptr()), xs, _vp(wg.data_ptr()), _vp(bg.data_ptr()) if bg is not None else None,
                                        _vp(ov.data_ptr()), os_, B, H, W, C, k, s, d, act, CAP if act == 4 else 0.0, None)
    torch.cuda.synchronize()
    assert rc == expect, _lib.lib().opa_last_error()
    got = ov.cpu()
    if expect == 0:
        ov.fill_(pc.SENTINEL)
    assert (obuf == pc.SENTINEL).all(), 'written outside the output pixels'
    return got, xv


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_integer_operands_bit_for_bit(case):
    """Inputs, taps and bias integers in [-3, 3]: at most 49 x 9 + 3 = 444 in magnitude, every partial sum exact -- the stored bits
    are those of the exact sum, with no activation, the ReLU and the ReLU clipped at 6."""
    dtype, k, s, B, H, W, C, xs, x_off, os_, o_off, has_bias, d = case
    g = torch.Generator().manual_seed(100 + k + 10 * s + 100 * d + C)
    x = torch.randint(-3, 4, (B, C, H, W), generator=g).double()
    w = torch.randint(-3, 4, (k * k, C), generator=g).double()
    b = torch.randint(-3, 4, (C,), generator=g).double() if has_bias else None
    exact = F.conv2d(x, w.t().reshape(C, 1, k, k), b, stride=s, padding=k // 2 * d, dilation=d, groups=C)
    assert float(exact.abs().max()) <= 2048 and torch.equal(exact.to(F16).double(), exact)
    xh, wh, bh = x.to(F16), w.to(F16), None if b is None else b.to(F16)
    got, _ = _run(case, xh, wh, bh, 0)
    assert torch.equal(pc.bits(got), pc.bits(exact.to(F16)))
    got, _ = _run(case, xh, wh, bh, 1)
    assert torch.equal(pc.bits(got), pc.bits(exact.clamp_min(0).to(F16)))
    out6 = _run_cap6(case, xh, wh, bh)
    assert torch.equal(pc.bits(out6), pc.bits(exact.clamp(0, 6).to(F16)))


def _run_cap6(case, x, w, b):
    """Code 4 with the cap 6 (ReLU6) on a dense copy of the layout's operands -> the output on the CPU."""
    dtype, k, s, B, H, W, C, xs, x_off, os_, o_off, has_bias, d = case
    Ho, Wo = fused.dwconv_out_hw(H, W, k, s, d)
    xg = x.cuda().contiguous(memory_format=CL)
    out = torch.empty((B, C, Ho, Wo), dtype=F16, device='cuda').contiguous(memory_format=CL)
    wg, bg = w.cuda(), (b.cuda() if b is not None else None)
    rc = _lib.lib().opa_dwconv_actp_f16(_vp(xg.data_ptr()), C, _vp(wg.data_ptr()), _vp(bg.data_ptr()) if bg is not None else None,
                                        _vp(out.data_ptr()), C, B, H, W, C, k, s, d, 4, 6.0, None)
    torch.cuda.synchronize()
    assert rc == 0, _lib.lib().opa_last_error()
    return out.cpu()


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_random_operands_against_float64(case, monkeypatch):
    dtype, k, s, B, H, W, C, xs, x_off, os_, o_off, has_bias, d = case
    x, w, b = _inputs(case)
    worst = 0.0
    for act in (0, 1, 2, 4):
        got, xv = _run(case, x, w, b, act)
        ref, bound = _reference(x, w, b, k, s, act, d)
        assert got.shape == ref.shape and bool(got.isfinite().all())
        ratio = float(((got.double() - ref).abs() / bound.clamp_min(1e-300)).max())
        worst = max(worst, ratio)
        print('dwconv f16 %s act %d: worst |err| / bound %.3f' % (_id(case), act, ratio))
        assert ratio <= 1.0, (act, ratio)
        # the same bits from a dense copy of the operands
        dense, _ = _run(_case(k, s, B, H, W, C, d=d, bias=has_bias), x, w, b, act)
        assert torch.equal(pc.bits(got), pc.bits(dense))
        # ... and through the Python entry point, which is the route for a float16 tensor behind the switch alone
        if os_ == C and o_off == 0 and fused._pixel_stride(xv) is not None:
            monkeypatch.setattr(fused, 'UNIT_F16', False)
            assert not fused.dwconv_supported(xv, k, s, d)
            monkeypatch.setattr(fused, 'UNIT_F16', True)
            assert fused.dwconv_supported(xv, k, s, d) and fused._pixel_stride(xv) == xs
            py = fused.dwconv_bias_act(xv, w.cuda(), b.cuda() if b is not None else None, k, s, act=act, dilation=d,
                                       act_param=CAP if act == 4 else 0.0)
            assert py.dtype == F16 and py.is_contiguous(memory_format=CL) and torch.equal(pc.bits(py.cpu()), pc.bits(got))


def test_the_store_is_float16s_rounding():
    """One tap of 1.0 and a bias of 0: the output is the input's own value through float32 and back, bit for bit -- a subnormal, the
    last finite value and its negative, inf, and a NaN stays NaN; 40000 + 40000 through the bias rounds beyond 65504 to inf."""
    k, C = 3, 8
    case = _case(k, 1, 1, 1, 4, C, bias=True)
    x = torch.zeros((1, C, 1, 4), dtype=F16)
    x.view(torch.int16)[0, :, 0, 1] = torch.tensor([0x0001, 0x7BFF, -0x0401, 0x7C00, 0x7E55, 0x03FF, 0x0400, 0x3C01], dtype=torch.int16)
    w = torch.zeros((k * k, C), dtype=F16)
    w[4] = 1.0                                                       # the centre tap
    got, _ = _run(case, x, w, torch.zeros(C, dtype=F16), 0)
    assert torch.equal(pc.bits(got[0, :4, 0, 1]), pc.bits(x[0, :4, 0, 1])) and bool(got[0, 4, 0, 1].isnan())
    assert torch.equal(pc.bits(got[0, 5:, 0, 1]), pc.bits(x[0, 5:, 0, 1]))
    finite = [0, 1, 2, 5, 6, 7]                                      # (a neighbour of the inf or the NaN multiplies it with a zero tap)
    assert bool((got[0, finite, 0, 0] == 0).all()) and bool((got[0, finite, 0, 2:] == 0).all())
    x = torch.full((1, C, 1, 4), 40000.0, dtype=F16)
    got, _ = _run(case, x, w, torch.full((C,), 40000.0, dtype=F16), 0)
    assert bool((got == float('inf')).all())
    got, _ = _run(case, x, w, torch.full((C,), 25504.0, dtype=F16), 0)
    assert bool((got == 65504.0).all())


def test_a_refused_call_writes_nothing():
    """What ``opa_dwconv_actp`` refuses, the twin refuses: windows, strides and dilations outside the list, code 3, a cap of 0."""
    case = _case(5, 1, 2, 5, 9, 8)
    x, w, b = _inputs(case, seed=1)
    w_any = torch.zeros((81, 8), dtype=F16)
    for k, s, d, act in ((9, 1, 1, 0), (5, 1, 3, 0), (5, 2, 2, 0), (5, 1, 2, 3), (4, 1, 1, 0), (5, 3, 1, 0)):
        B, H, W, C = 2, 5, 9, 8
        obuf = torch.full((B * H * W * C + 2 * pc.PAD,), pc.SENTINEL, dtype=F16, device='cuda')
        xg = x.cuda().contiguous(memory_format=CL)
        rc = _lib.lib().opa_dwconv_actp_f16(_vp(xg.data_ptr()), C, _vp(w_any.cuda().data_ptr()), None, _vp(obuf.data_ptr() + 2 * pc.PAD), C,
                                            B, H, W, C, k, s, d, act, 0.0, None)
        torch.cuda.synchronize()
        assert rc == 1 and (obuf == pc.SENTINEL).all(), (k, s, d, act)
    # the other entry points keep refusing dtype 1
    out = torch.full((2 * 5 * 9 * 8,), pc.SENTINEL, dtype=F16, device='cuda')
    xg, wg = x.cuda().contiguous(memory_format=CL), w.cuda()
    assert _lib.lib().opa_dwconv_actp(_vp(xg.data_ptr()), 8, _vp(wg.data_ptr()), None, _vp(out.data_ptr()), 8, 2, 5, 9, 8, 5, 1, 1, 1, 0, 0.0, None) == 1
    assert _lib.lib().opa_dwconv_act(_vp(xg.data_ptr()), 8, _vp(wg.data_ptr()), None, _vp(out.data_ptr()), 8, 2, 5, 9, 8, 5, 1, 1, 0, None) == 1
    torch.cuda.synchronize()
    assert (out == pc.SENTINEL).all()
    assert torch.cuda.current_stream().query() and float(torch.ones(1, device='cuda').sum()) == 1.0      # no sticky launch error
