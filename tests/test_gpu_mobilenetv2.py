"""MobileNetV2, ShuffleNetV2 x1 / x2 and the LeakyReLU ShuffleNetV2K units on the project's kernels (real kernels, MI355X): the
activation codes with a parameter -- 3 LeakyReLU(slope), 4 clipped ReLU(cap) -- in the unit-mode GEMM and the depthwise stencil,
the two entry points that take them, the block and unit routes built from them and the whole networks.

Two criteria.  A KERNEL with a new code: its result is torch's float32 ``leaky_relu(y, slope)`` / ``clamp(y, 0, cap)`` of ``y``, the
``act = 0`` output of the same entry point on the same operands -- equal value for value, NaN where torch has NaN, no tolerance: the
activation is the kernel's last float32 operation (in bfloat16: 0 and the caps 6 and 1.5 are representable and rounding is
monotone, so clipping before the rounding is clipping behind it).  A ROUTE: the criterion of ``test_gpu_unit_routes.py`` and
``test_gpu_mobilenetv3.py`` -- ``ref64`` the unfused module in ``double()``; ``e0`` the error against ``ref64`` of the SAME unfused float32
torch module (the median of nine calls), never of the code under test; required ``err <= 2 * e0``, as a maximum and as an rms.
Every route case prints an ``MBV2`` line (``pytest -s``); the lines of a run are kept in ``profiles/mobilenetv2/route_errors.log``.
Both routes are off by default (``fused.MBV2``, ``fused.UNIT_LEAKY``); the ``rec`` fixture switches them on."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from openpifpaf_amd import _lib, fused, network

import trunk_common as tc

pytestmark = pytest.mark.gpu

SEEDS = (0, 1, 2)
CL = torch.channels_last
SENTINEL = 12345.5
LEAKY, CLIP = fused.ACT_LEAKY_RELU, fused.ACT_RELU6
_LAUNCHERS = {'conv1x1_unit_x3': 'unit', 'dwconv_bias_act': 'dwconv', 'channel_interleave': 'interleave', 'bias_act_': 'bias_act',
              'conv1x1_bias_act': 'gemm', 'conv1x1_bias_act_x3': 'gemm3', 'head_conv_x3': 'head_x3', 'head_epilogue': 'head_epilogue'}


_report = functools.partial(tc.report, 'MBV2')


def _same(got, want):
    """Equal value for value, NaN exactly where ``want`` has NaN."""
    nan = want.isnan()
    return bool(torch.equal(got.isnan(), nan)) and bool(torch.equal(got[~nan], want[~nan]))


def _torch_act(y, act, param):
    return F.leaky_relu(y, param) if act == LEAKY else torch.clamp(y, 0.0, param)


def _pieces(y, act, param):
    """Does ``y`` reach every piece of the activation?"""
    y = y[y.isfinite()]
    if act == LEAKY:
        return bool((y < 0).any()) and bool((y > 0).any())
    return bool((y < 0).any()) and bool((y > param).any()) and bool(((y > 0) & (y < param)).any())


@pytest.fixture
def rec(monkeypatch):
    """Launch recorder; nothing may be timed; both new routes switched on, every ``pick`` forced to the project's kernel (the shapes
    here are far below the size from which it is chosen); the switches and the choice table restored after."""
    return tc.recorder(monkeypatch, _LAUNCHERS, ('X3_UNIT', 'MBV2', 'UNIT_LEAKY'), force_pick='x3')


# ---- 1. the unit GEMM with the two new codes -------------------------------------------------------------------------------------

def _unit_actp(conv, x, act, param, terms, partner=None, residual=None):
    """``opa_gemm_unit_actp_f32x3``, raw, into a sentinel-filled output."""
    w3, bp = fused._unit_weight_of(conv)
    n, (B, K, H, W) = conv.out_channels, x.shape
    out = torch.full((B, 2 * n if partner is not None else n, H, W), SENTINEL, device='cuda').contiguous(memory_format=CL)
    vp = ctypes.c_void_p

    def operand(t):
        return (None, 0) if t is None else (vp(t.data_ptr()), fused._pixel_stride(t))
    status = _lib.lib().opa_gemm_unit_actp_f32x3(vp(x.data_ptr()), fused._pixel_stride(x), vp(w3.data_ptr()), vp(bp.data_ptr()), *operand(partner),
                                                 *operand(residual), vp(out.data_ptr()), B * H * W, n, K, act, float(param), terms, None)
    assert status == 0, _lib.lib().opa_last_error().decode()
    torch.cuda.synchronize()
    return out


# M, K, N, layout: `dense` -- x a dense tensor of [*, K, h, w]; `half` -- x the SECOND half of a 2K-channel tensor (4 K bytes into a
# pixel: on an 8-byte, not a 16-byte boundary for K = 58 and 122) with the first half as the partner
UNIT_SHAPES = {'126x16x96': ((2, 9, 7), 16, 96, 'dense'), '144x16x96': ((2, 9, 8), 16, 96, 'dense'), '63x58x58': ((1, 9, 7), 58, 58, 'half'),
               '63x122x122': ((1, 9, 7), 122, 122, 'half'), '12x320x1280': ((1, 3, 4), 320, 1280, 'dense')}


def _unit_operands(shape, seed, non_finite=False):
    (B, H, W), K, N, layout = UNIT_SHAPES[shape]
    conv = tc.randomize_(nn.Conv2d(K, N, 1), seed).cuda()
    wide = (torch.randn((B, 2 * K if layout == 'half' else K, H, W), generator=tc.gen(seed + 1)) * 3.0).cuda().contiguous(memory_format=CL)
    if non_finite:                       # a +Inf row and a NaN row of x (pixels 3 and 5): their output rows are NaN, no other is touched
        wide[0, :, 0, 3] = float('inf')
        wide[0, :, 0, 5] = float('nan')
    if layout == 'half':
        x, partner = wide[:, K:], wide[:, :K]
        assert x.data_ptr() % 16 == 8 and fused.unit_conv_x3_supported(conv, x, partner=partner)
        return conv, x, partner
    assert fused.unit_conv_x3_supported(conv, wide)
    return conv, wide, None


@pytest.mark.parametrize('terms', [6, 9])
@pytest.mark.parametrize('act,param', [(LEAKY, 0.01), (LEAKY, 0.3), (CLIP, 6.0), (CLIP, 1.5)])
@pytest.mark.parametrize('shape', list(UNIT_SHAPES))
def test_unit_gemm_with_a_parameter(shape, act, param, terms, monkeypatch):
    conv, x, partner = _unit_operands(shape, 7)
    n = conv.out_channels
    if act == CLIP:
        partner = None                                             # (the clipped ReLU is plain: MobileNetV2 has no shuffle)
    x0 = x.clone()
    y = _unit_actp(conv, x, 0, 0.0, terms, partner)
    got = _unit_actp(conv, x, act, param, terms, partner)
    assert torch.equal(x, x0) and y.isfinite().all() and not bool((y == SENTINEL).any()) and not bool((got == SENTINEL).any())
    lin = y if partner is None else y[:, 1::2]
    assert tuple(lin.shape[1:2]) == (n,) and _pieces(lin, act, param), 'the data does not reach every piece of the activation'
    if partner is None:
        assert _same(got, _torch_act(y, act, param))
    else:                                                          # the odd channels; the even ones are the partner's bits
        assert _same(got[:, 1::2], _torch_act(lin, act, param))
        assert torch.equal(got[:, 0::2].contiguous().view(torch.int32), partner.contiguous().view(torch.int32))
    assert not torch.equal(got, y)
    # the launcher reaches the same kernel with the same arguments
    monkeypatch.setattr(fused, 'X3_TERMS', terms)
    assert torch.equal(fused.conv1x1_unit_x3(conv, x, act=act, act_param=param, partner=partner), got)


@pytest.mark.parametrize('act,param', [(LEAKY, 0.01), (CLIP, 6.0)])
def test_unit_gemm_with_a_parameter_keeps_nan(act, param):
    """A +Inf row and a NaN row in ``x``: the split turns both into NaN rows of ``y`` (``csrc/gemm_f32x3.hip``), which the selects
    pass on; every other row is what it is without them."""
    conv, x, _ = _unit_operands('126x16x96', 7, non_finite=True)
    clean = _unit_operands('126x16x96', 7)[1]
    y = _unit_actp(conv, x, 0, 0.0, 6)
    got = _unit_actp(conv, x, act, param, 6)
    assert bool(y[0, :, 0, 3].isnan().all()) and bool(y[0, :, 0, 5].isnan().all()) and int(y.isnan().sum()) == 2 * conv.out_channels
    assert _same(got, _torch_act(y, act, param)) and _pieces(y, act, param)
    finite = ~y.isnan()
    assert torch.equal(got[finite], _unit_actp(conv, clean, act, param, 6)[finite])


def test_unit_gemm_refuses_a_residual_with_a_parameter():
    conv, x, _ = _unit_operands('126x16x96', 7)
    res = torch.zeros((2, 96, 9, 7), device='cuda').contiguous(memory_format=CL)
    w3, bp = fused._unit_weight_of(conv)
    out = torch.full((2, 96, 9, 7), 7.0, device='cuda').contiguous(memory_format=CL)
    vp = ctypes.c_void_p
    for act, param in ((LEAKY, 0.01), (CLIP, 6.0), (CLIP, float('nan')), (CLIP, 0.0), (LEAKY, -0.01)):
        rc = _lib.lib().opa_gemm_unit_actp_f32x3(vp(x.data_ptr()), 16, vp(w3.data_ptr()), vp(bp.data_ptr()), None, 0, vp(res.data_ptr()), 96,
                                                 vp(out.data_ptr()), 126, 96, 16, act, param, 6, None)
        assert rc == 1, (act, param)                               # OPA_ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), 'something was launched'


# ---- 2. the depthwise stencil with the clipped ReLU ----------------------------------------------------------------------------------

def _dw_actp(x, taps, bias, k, stride, dilation, act, param, symbol='opa_dwconv_actp'):
    """``opa_dwconv_actp`` (or an older entry point, without the parameter), raw, into a sentinel-filled output."""
    B, C, H, W = x.shape
    ho, wo = fused.dwconv_out_hw(H, W, k, stride, dilation)
    out = torch.full((B, C, ho, wo), SENTINEL, dtype=x.dtype, device='cuda').contiguous(memory_format=CL)
    vp = ctypes.c_void_p
    args = [vp(x.data_ptr()), fused._pixel_stride(x), vp(taps.data_ptr()), vp(bias.data_ptr()), vp(out.data_ptr()), C, B, H, W, C, k, stride]
    if symbol == 'opa_dwconv_actp':
        args += [dilation, fused._DTYPES[x.dtype], act, float(param)]
    else:
        args += ([dilation] if symbol == 'opa_dwconv_dilated_act' else []) + [fused._DTYPES[x.dtype], act]
    status = getattr(_lib.lib(), symbol)(*args, None)
    assert status == 0, _lib.lib().opa_last_error().decode()
    torch.cuda.synchronize()
    return out


def _dw_operands(C, H, W, k, dtype, seed):
    g = tc.gen(seed)
    x = (torch.randn((2, C, H, W), generator=g) * 4.0).to(dtype).cuda().contiguous(memory_format=CL)
    taps = (torch.randn((k * k, C), generator=g) * (2.0 / (k * k)) ** 0.5).to(dtype).cuda()
    bias = (torch.randn(C, generator=g) * 0.5).to(dtype).cuda()
    return x, taps, bias


# C, H, W, k, stride, dilation
DW_CASES = {'C32-k3-s1': (32, 9, 7, 3, 1, 1), 'C96-k3-s2': (96, 9, 7, 3, 2, 1), 'C960-3x3': (960, 3, 3, 3, 1, 1), 'C40-k5-s2': (40, 9, 7, 5, 2, 1),
            'C32-k3-d2': (32, 9, 7, 3, 1, 2)}


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['float32', 'bfloat16'])
@pytest.mark.parametrize('cap', [6.0, 1.5])
@pytest.mark.parametrize('case', list(DW_CASES))
def test_depthwise_with_clipped_relu(case, cap, dtype):
    C, H, W, k, stride, dilation = DW_CASES[case]
    x, taps, bias = _dw_operands(C, H, W, k, dtype, 100 * C + k)
    assert fused.dwconv_supported(x, k, stride, dilation)
    x0 = x.clone()
    y = _dw_actp(x, taps, bias, k, stride, dilation, 0, 0.0)
    got = _dw_actp(x, taps, bias, k, stride, dilation, CLIP, cap)
    sentinel = torch.full((1,), SENTINEL, dtype=dtype, device='cuda')
    assert torch.equal(x, x0) and y.isfinite().all() and not bool((y == sentinel).any()) and not bool((got == sentinel).any())
    assert _pieces(y.float(), CLIP, cap), 'the data does not reach every piece of the activation'
    assert _same(got, torch.clamp(y, 0.0, cap)) and not torch.equal(got, y)
    assert torch.equal(fused.dwconv_bias_act(x, taps, bias, k, stride, act=CLIP, act_param=cap, dilation=dilation), got)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['float32', 'bfloat16'])
def test_depthwise_with_clipped_relu_keeps_nan(dtype):
    """A +Inf, a -Inf and a NaN input pixel, far enough apart that no window holds two of them: +-Inf reach the outputs around them
    with the sign of the tap (clipped to the cap or to 0), NaN stays NaN."""
    C, H, W, k, stride, dilation = DW_CASES['C32-k3-s1']
    x, taps, bias = _dw_operands(C, H, W, k, dtype, 5)
    x[0, :, 0, 0], x[0, :, 5, 4], x[1, :, 4, 3] = float('inf'), float('-inf'), float('nan')
    y = _dw_actp(x, taps, bias, k, stride, dilation, 0, 0.0)
    got = _dw_actp(x, taps, bias, k, stride, dilation, CLIP, 6.0)
    assert bool((y == float('inf')).any()) and bool((y == float('-inf')).any()) and int(y[1].isnan().sum()) == 9 * C
    assert _same(got, torch.clamp(y, 0.0, 6.0)) and bool(got[1, :, 3:6, 2:5].isnan().all()) and not bool(got[0].isnan().any())
    assert float(got[~got.isnan()].max()) == 6.0 and float(got[~got.isnan()].min()) == 0.0


def test_depthwise_refuses_code_3():
    x, taps, bias = _dw_operands(8, 4, 4, 3, torch.float32, 0)
    out = torch.full((2, 8, 4, 4), 7.0, device='cuda').contiguous(memory_format=CL)
    vp = ctypes.c_void_p
    for act, param in ((LEAKY, 0.01), (CLIP, 0.0), (CLIP, float('inf'))):
        rc = _lib.lib().opa_dwconv_actp(vp(x.data_ptr()), 8, vp(taps.data_ptr()), vp(bias.data_ptr()), vp(out.data_ptr()), 8, 2, 4, 4, 8, 3, 1, 1, 0,
                                        act, param, None)
        assert rc == 1, (act, param)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), 'something was launched'


# ---- 3. the entry points with the older codes ARE the older entry points ------------------------------------------------------------------

@pytest.mark.parametrize('third', ['alone', 'partner', 'residual'])
@pytest.mark.parametrize('act', [0, 1, 2])
@pytest.mark.parametrize('N,terms', [(40, 6), (128, 6), (40, 9)])
def test_unit_gemm_entry_points_are_one_kernel(N, terms, act, third):
    """``opa_gemm_unit_act_f32x3(act=a)`` against ``opa_gemm_unit_actp_f32x3(act=a, any parameter)``, raw, each into its own
    sentinel-filled output: bit for bit.  K = 72 (a K tail), M = 286 (two full 128-row tiles and a tail); N = 40: the 64-wide tile
    with an N tail, N = 128: the 128-wide tile."""
    K = 72
    conv = tc.randomize_(nn.Conv2d(K, N, 1), K + N).cuda()
    x = torch.randn((2, K, 13, 11), generator=tc.gen(K)).cuda().contiguous(memory_format=CL)
    t = torch.randn((2, N, 13, 11), generator=tc.gen(N)).cuda().contiguous(memory_format=CL)
    partner, residual = (t if third == 'partner' else None), (t if third == 'residual' else None)
    w3, bp = fused._unit_weight_of(conv)
    old = torch.full((2, 2 * N if partner is not None else N, 13, 11), SENTINEL, device='cuda').contiguous(memory_format=CL)
    vp = ctypes.c_void_p
    assert _lib.lib().opa_gemm_unit_act_f32x3(vp(x.data_ptr()), K, vp(w3.data_ptr()), vp(bp.data_ptr()), vp(t.data_ptr()) if partner is not None else None,
                                              N if partner is not None else 0, vp(t.data_ptr()) if residual is not None else None,
                                              N if residual is not None else 0, vp(old.data_ptr()), 286, N, K, act, terms, None) == 0
    torch.cuda.synchronize()
    new = _unit_actp(conv, x, act, 0.25, terms, partner, residual)
    assert torch.equal(old.view(torch.int32), new.view(torch.int32)) and old.isfinite().all() and not bool((old == SENTINEL).any())
    lin = old[:, 1::2] if partner is not None else old
    assert bool(lin.lt(0).any()) == (act != 1)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['float32', 'bfloat16'])
@pytest.mark.parametrize('act', [0, 1, 2])
@pytest.mark.parametrize('k,stride,dilation', [(3, 1, 1), (5, 2, 1), (7, 1, 1), (3, 1, 2)])
def test_depthwise_entry_points_are_one_kernel(k, stride, dilation, act, dtype):
    """``opa_dwconv_actp(act=a, any parameter)`` against ``opa_dwconv_dilated_act(act=a)`` -- and ``opa_dwconv_act(act=a)`` where that
    takes the window -- raw, each into its own sentinel-filled output: bit for bit."""
    x, taps, bias = _dw_operands(8, 7, 5, k, dtype, 10 * k + stride)
    new = _dw_actp(x, taps, bias, k, stride, dilation, act, 0.25)
    olds = [_dw_actp(x, taps, bias, k, stride, dilation, act, None, 'opa_dwconv_dilated_act')]
    if k in (3, 5) and dilation == 1:
        olds.append(_dw_actp(x, taps, bias, k, stride, dilation, act, None, 'opa_dwconv_act'))
    sentinel = torch.full((1,), SENTINEL, dtype=dtype, device='cuda')
    for old in olds:
        assert torch.equal(old, new) and old.isfinite().all() and not bool((old == sentinel).any())
    assert bool((new < 0).any()) == (act != 1)


# ---- 4. block and unit routes ------------------------------------------------------------------------------------------------------

# MobileNetV2 blocks (inp, oup, stride, t): t = 1 (backbone.1), stride 2 (backbone.2), stride 1 with the residual (backbone.3)
# ShuffleNetV2 / K units (inp, oup, first in stage, stride, kernel, leaky): x1 and x2 stage 2, k16 stage 2 with LeakyReLU
MODULES = {'mbv2-t1': ('mbv2', (32, 16, 1, 1)), 'mbv2-stride2': ('mbv2', (16, 24, 2, 6)), 'mbv2-residual': ('mbv2', (24, 24, 1, 6)),
           'x1-first': ('unit', (24, 116, True, 2, 3, False)), 'x1-plain': ('unit', (116, 116, False, 1, 3, False)),
           'x2-first': ('unit', (24, 244, True, 2, 3, False)), 'x2-plain': ('unit', (244, 244, False, 1, 3, False)),
           'k16-leaky-first': ('unit', (24, 348, True, 2, 5, True)), 'k16-leaky-plain': ('unit', (348, 348, False, 1, 5, True))}
UNIT_NEW = {False: ['unit', 'dwconv', 'unit'], True: ['dwconv', 'unit', 'unit', 'dwconv', 'unit']}
UNIT_OLD = {False: ['miopen:branch2.0', 'dwconv', 'miopen:branch2.5', 'interleave'],
            True: ['dwconv', 'miopen:branch1.2', 'miopen:branch2.0', 'dwconv', 'miopen:branch2.5', 'interleave']}


def _make(name, seed):
    kind, spec = MODULES[name]
    if kind == 'mbv2':
        return tc.randomize_(network._MBV2Block(*spec), seed)
    inp, oup, first, stride, k, leaky = spec
    return tc.randomize_(network._InvertedResidualK(inp, oup, first, stride=stride, kernel_size=k, leaky_relu=leaky), seed)


def _trace_of(name):
    kind, spec = MODULES[name]
    return (['unit'] if spec[3] != 1 else []) + ['dwconv', 'unit'] if kind == 'mbv2' else UNIT_NEW[spec[2]]


@functools.lru_cache(maxsize=None)
def _reference(name, seed):
    """-> (the unfused module on the CPU, x, ref64, e0, the largest input of a ReLU6)."""
    module = _make(name, seed)
    x = (torch.randn((2, MODULES[name][1][0], 9, 7), generator=tc.gen(1000 + seed)) * 2.0).cuda().contiguous(memory_format=CL)
    seen = []
    with torch.no_grad():
        m64 = copy.deepcopy(module).double().cuda()
        for m in m64.modules():
            if isinstance(m, nn.ReLU6):
                m.register_forward_pre_hook(lambda mod, args: seen.append(float(args[0].max())))
        ref64 = m64(x.double())
        plain = copy.deepcopy(module).cuda().to(memory_format=CL)
        e0 = tc.e0(lambda: plain(x), ref64)
    assert e0[0] > 0 and ref64.isfinite().all()
    return module, x, ref64, e0, max(seen, default=0.0)


@pytest.mark.parametrize('name', list(MODULES))
def test_route(rec, name):
    ok = True
    for seed in SEEDS:
        module, x, ref64, e0, largest = _reference(name, seed)
        if MODULES[name][0] == 'mbv2':
            assert largest > 6.0, 'no pre-activation exceeds 6: the clip is not exercised (%.3f)' % largest
        elif MODULES[name][1][5]:
            assert bool((ref64 < 0).any()), 'no negative output: the LeakyReLU is not exercised'
        opt = rec.watch(tc.optimized(module).cuda().to(memory_format=CL))
        got, trace = tc.forward_checks(opt, x, rec)
        assert trace == _trace_of(name), trace
        assert fused.choices() == {}, 'the route made a choice-table entry'
        assert got.is_contiguous(memory_format=CL) and got.shape == ref64.shape
        ok &= _report('%s | %s | seed %d' % (name, ' '.join(trace), seed), tc.errors(got, ref64), e0)
    assert ok


@pytest.mark.parametrize('name', ['mbv2-stride2', 'mbv2-residual', 'mbv2-t1'])
def test_mbv2_route_selection(rec, name):
    """On with the switch, torch's forward convolution for convolution without it; bfloat16, autocast and a tensor that is not
    channels-last take torch's forward."""
    module, x, _, _, _ = _reference(name, 0)
    opt = rec.watch(tc.optimized(module).cuda().to(memory_format=CL))
    got, trace = tc.forward_checks(opt, x, rec)
    assert trace == _trace_of(name) and opt._route_supported(x), trace
    convs = ['miopen:' + n for n, m in opt.named_modules() if isinstance(m, nn.Conv2d)]
    fused.MBV2 = False
    off, trace = tc.forward_checks(opt, x, rec)
    assert trace == convs and not opt._route_supported(x), trace
    assert float((off - got).abs().max()) <= 1e-4 * float(off.abs().max())
    fused.MBV2 = True
    assert not opt._route_supported(x.bfloat16())
    assert not opt._route_supported(x.contiguous())
    with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
        assert not opt._route_supported(x)
        rec.trace.clear()
        opt(x)
    assert rec.trace == convs, rec.trace
    opt16 = rec.watch(tc.optimized(module).cuda().to(torch.bfloat16).to(memory_format=CL))
    with torch.no_grad():
        rec.trace.clear()
        opt16(x.bfloat16().contiguous(memory_format=CL))
    assert rec.trace == convs, rec.trace


@pytest.mark.parametrize('name', ['k16-leaky-first', 'k16-leaky-plain'])
def test_leaky_unit_route_selection(rec, name):
    first = MODULES[name][1][2]
    module, x, _, _, _ = _reference(name, 0)
    opt = rec.watch(tc.optimized(module).cuda().to(memory_format=CL))
    got, trace = tc.forward_checks(opt, x, rec)
    assert trace == UNIT_NEW[first], trace
    fused.UNIT_LEAKY = False                                       # today's route, launch for launch, even with the pick forced
    off, trace = tc.forward_checks(opt, x, rec)
    assert trace == UNIT_OLD[first], trace
    assert float((off - got).abs().max()) <= 1e-4 * float(off.abs().max()) and bool((off < 0).any())
    fused.UNIT_LEAKY = True
    opt16 = rec.watch(tc.optimized(module).cuda().to(torch.bfloat16).to(memory_format=CL))
    _, trace = tc.forward_checks(opt16, x.bfloat16().contiguous(memory_format=CL), rec)
    assert trace == UNIT_OLD[first], trace
    with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
        rec.trace.clear()
        opt(x)
    assert 'unit' not in rec.trace, rec.trace


def test_leaky_network_with_the_switch_off_launches_what_it_launches_today(rec):
    """A LeakyReLU shufflenetv2k16 with cocokp heads on [2, 3, 65, 97], every ``pick`` forced to the project's kernel: with
    ``UNIT_LEAKY`` off the unit GEMM runs for the two heads alone (1392 input channels), every unit is stencil + torch's 1x1
    convolutions + the interleave pass and ``conv5`` is torch's; with it on, 3 first units x 3 + 13 units x 2 + conv5 + 2 heads = 38."""
    from openpifpaf_amd import headmeta
    net = tc.randomize_(network.Shell(network.ShuffleNetV2K('shufflenetv2k16', leaky_relu=True),
                                      [network.CompositeField4(m, 1392) for m in headmeta.cocokp_metas()]), 3)
    opt = rec.watch(network.optimize_for_inference_(net).cuda().to(memory_format=CL))
    x = torch.randn((2, 3, 65, 97), generator=tc.gen(9)).cuda().contiguous(memory_format=CL)
    with torch.no_grad():
        fused.UNIT_LEAKY = False
        rec.trace.clear()
        off = opt(x)
        trace = list(rec.trace)
        assert trace.count('unit') == 2 and trace.count('interleave') == 16 and trace.count('dwconv') == 19, trace
        assert 'miopen:base_net.conv5.0' in trace and sum(t.startswith('miopen:base_net.stage') for t in trace) == 3 * 3 + 13 * 2
        fused.UNIT_LEAKY = True
        rec.trace.clear()
        on = opt(x)
        trace = list(rec.trace)
        assert trace.count('unit') == 38 and trace.count('interleave') == 0 and trace.count('dwconv') == 19, trace
        assert [t for t in trace if t.startswith('miopen:')] == ['miopen:base_net.input_block.0'], trace
    for u, v in zip(off, on):
        assert float((u - v).abs().max()) <= 1e-4 * float(u.abs().max())


# ---- 5. whole networks ---------------------------------------------------------------------------------------------------------------

NETS = ['mobilenetv2', 'shufflenetv2x1', 'shufflenetv2x2']


def _plain_e0(net, x, ref64):
    plain = copy.deepcopy(net).cuda().to(memory_format=CL)
    saved, fused.FORCE_PICK = fused.FORCE_PICK, 'conv'                 # e0: torch's own convolutions, the heads' too
    try:
        return [tc.e0(lambda: plain(x)[i], r) for i, r in enumerate(ref64)]
    finally:
        fused.FORCE_PICK = saved


@pytest.mark.parametrize('name', NETS)
def test_whole_network(rec, name):
    """cocokp heads on [2, 3, 65, 97]: the optimized channels-last model against the double model, both head outputs; then the same
    after ``load_state_dict`` of other weights into the optimised network, against THEIR double model."""
    net, net2 = tc.randomize_(network.factory(name), 7), tc.randomize_(network.factory(name), 11)
    x = torch.randn((2, 3, 65, 97), generator=tc.gen(8)).cuda().contiguous(memory_format=CL)
    with torch.no_grad():
        ref64 = copy.deepcopy(net).double().cuda()(x.double())
        e0s = _plain_e0(net, x, ref64)
        opt = rec.watch(network.optimize_for_inference_(copy.deepcopy(net)).cuda().to(memory_format=CL))
        rec.trace.clear()
        got = opt(x)
        trace = list(rec.trace)
        again = opt(x)
    torch_convs = [t for t in trace if t.startswith('miopen:')]
    if name == 'mobilenetv2':
        blocks = [m for m in opt.base_net.backbone if isinstance(m, network._MBV2Block)]
        assert len(blocks) == 17 and trace.count('dwconv') == 17 and trace.count('unit') == 17 + 16 + 1, trace
        assert torch_convs == ['miopen:base_net.backbone.0.0'], 'only the stem is torch\'s'
    else:
        assert trace.count('dwconv') == 19 and trace.count('unit') == 3 * 3 + 13 * 2 + 1 and 'interleave' not in trace, trace
        assert torch_convs == ['miopen:base_net.conv1.0'], 'only the stem is torch\'s'
    assert trace.count('head_x3') == 2, trace
    ok = True
    for i, (g, a, r) in enumerate(zip(got, again, ref64)):
        assert g.isfinite().all() and g.shape == r.shape
        ok &= _report('%s head %d' % (name, i), tc.errors(g, r), e0s[i])
        assert float((g - a).abs().max()) <= 1e-6 * float(g.abs().max())       # (the stem is MIOpen's: equal up to its own repeatability)
    # other weights into the optimised network: the new weights' result
    with torch.no_grad():
        other = network.optimize_for_inference_(copy.deepcopy(net2))
        opt.load_state_dict(other.state_dict(), strict=True)
        ref64 = copy.deepcopy(net2).double().cuda()(x.double())
        e0s = _plain_e0(net2, x, ref64)
        after = opt(x)
    for i, (g, b, r) in enumerate(zip(after, got, ref64)):
        assert not torch.equal(g, b)
        ok &= _report('%s head %d after load_state_dict' % (name, i), tc.errors(g, r), e0s[i])
    assert ok


@pytest.mark.parametrize('name', ['mbv2-residual', 'x1-first', 'k16-leaky-plain'])
def test_forward_after_load_state_dict(rec, name):
    """The same at the level of one block, where no MIOpen kernel runs: bit for bit the output of the module the weights came from."""
    _, x, _, _, _ = _reference(name, 0)
    opt = tc.optimized(_make(name, 0)).cuda().to(memory_format=CL)
    other = tc.optimized(_make(name, 1)).cuda().to(memory_format=CL)
    with torch.no_grad():
        before = opt(x)
        opt.load_state_dict(other.state_dict(), strict=True)
        rec.trace.clear()
        after = opt(x)
        assert rec.trace == _trace_of(name), rec.trace
        assert not torch.equal(before, after)
        assert torch.equal(after, other(x)), 'stale operand: max |delta| %.3g' % (after - other(x)).abs().max().item()


@pytest.mark.parametrize('name', ['mobilenetv2', 'shufflenetv2x1'])
def test_predictor_smoke(name, monkeypatch):
    from openpifpaf_amd.predictor import Predictor
    monkeypatch.setattr(fused, 'MBV2', True)
    rng = np.random.default_rng(3)
    frames = [rng.integers(0, 256, (48, 64, 3), dtype=np.uint8), rng.integers(0, 256, (64, 40, 3), dtype=np.uint8)]
    saved = Predictor.long_edge, Predictor.batch_size
    Predictor.long_edge, Predictor.batch_size = 65, 2
    try:
        pred = Predictor(name)
        assert type(pred.model_cpu.base_net) is {'mobilenetv2': network.MobileNetV2, 'shufflenetv2x1': network.ShuffleNetV2}[name]
        out = [p for p, _, _ in pred.numpy_images(frames)]
    finally:
        Predictor.long_edge, Predictor.batch_size = saved
    assert len(out) == 2 and all(isinstance(p, list) for p in out)
