"""MobileNetV3 on the project's kernels (real kernels, MI355X): the depthwise stencil with hardswish, the squeeze-and-excitation
kernels (``csrc/se.hip``), the unit-mode GEMM with hardswish and with a residual, the block route built from them
(``network._InvertedResidual._forward_unit``) and the two whole networks.

The error criterion is the one of ``test_gpu_unit_routes.py``: ``ref64`` the unfused module or op in ``double()``; ``e0`` the error
against ``ref64`` of the SAME unfused float32 torch module or op (the median of nine calls), not of the code under test;
``err = max |got - ref64| / max |ref64|`` and the same as an rms; required ``err <= 2 * e0`` (two independent errors of size ``e0``).
Every case prints an ``MBV3`` line (``pytest -s``); the lines of a run are kept in ``profiles/mobilenetv3/route_errors.log``.
The route is off by default (``fused.MBV3``); the ``rec`` fixture switches it on."""
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
_LAUNCHERS = {'conv1x1_unit_x3': 'unit', 'dwconv_bias_act': 'dwconv', 'se_gate': 'se_gate', 'scale_channels_': 'scale',
              'channel_interleave': 'interleave', 'bias_act_': 'bias_act', 'conv1x1_bias_act': 'gemm', 'conv1x1_bias_act_x3': 'gemm3',
              'head_conv_x3': 'head_x3', 'head_epilogue': 'head_epilogue'}


_report = functools.partial(tc.report, 'MBV3')


@pytest.fixture
def rec(monkeypatch):
    """Launch recorder; nothing may be timed; the switches at their defaults and the choice table empty, both restored after."""
    return tc.recorder(monkeypatch, _LAUNCHERS, ('X3_UNIT', 'MBV3'))


# ---- 1. depthwise + hardswish ------------------------------------------------------------------------------------------------

def _views(C, seed):
    """A dense tensor, a slice on an 8-byte boundary (channel vectors of 2) and one on a 4-byte boundary (of 1)."""
    dense = torch.randn((2, C, 9, 7), generator=tc.gen(seed)).cuda().contiguous(memory_format=CL)
    wide2 = torch.randn((2, C + 6, 9, 7), generator=tc.gen(seed + 1)).cuda().contiguous(memory_format=CL)
    wide1 = torch.randn((2, C + 5, 9, 7), generator=tc.gen(seed + 2)).cuda().contiguous(memory_format=CL)
    return {'dense': dense, 'slice2': wide2[:, 2:2 + C], 'slice1': wide1[:, 1:1 + C]}


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('k', [3, 5])
@pytest.mark.parametrize('C', [16, 72, 88, 200])
def test_depthwise_with_hardswish(C, k, stride):
    g = tc.gen(100 * C + 10 * k + stride)
    w = (torch.randn((C, 1, k, k), generator=g) * (2.0 / (k * k)) ** 0.5).cuda()
    b = (torch.randn(C, generator=g) * 0.5).cuda()
    taps = w.reshape(C, k * k).t().contiguous()
    ok = True
    for layout, x in _views(C, C + k + stride).items():
        assert fused.dwconv_supported(x, k, stride)
        ref64 = F.hardswish(F.conv2d(x.double(), w.double(), b.double(), stride, k // 2, groups=C))
        e0 = tc.e0(lambda: F.hardswish(F.conv2d(x, w, b, stride, k // 2, groups=C)), ref64)
        x0 = x.clone()
        got = fused.dwconv_bias_act(x, taps, b, k, stride, act=fused.ACT_HARDSWISH)
        assert torch.equal(x, x0) and got.is_contiguous(memory_format=CL) and got.isfinite().all()
        ok &= _report('dwconv+hardswish C %d k %d s %d %s' % (C, k, stride, layout), tc.errors(got, ref64), e0)
        # the other codes of the new entry point ARE the existing kernels
        for act, relu in ((fused.ACT_RELU, True), (fused.ACT_NONE, False)):
            assert torch.equal(fused.dwconv_bias_act(x, taps, b, k, stride, act=act), fused.dwconv_bias_act(x, taps, b, k, stride, relu=relu))
        assert torch.equal(fused.dwconv_bias_act(x, taps, b, k, stride, act=fused.ACT_RELU), F.relu(fused.dwconv_bias_act(x, taps, b, k, stride)))
    assert ok


def test_depthwise_act_code_is_checked():
    x = torch.zeros((1, 8, 4, 4), device='cuda').contiguous(memory_format=CL)
    taps, out = torch.zeros((9, 8), device='cuda'), torch.full((1, 8, 4, 4), 7.0, device='cuda').contiguous(memory_format=CL)
    vp = ctypes.c_void_p
    rc = _lib.lib().opa_dwconv_act(vp(x.data_ptr()), 8, vp(taps.data_ptr()), None, vp(out.data_ptr()), 8, 1, 4, 4, 8, 3, 1, 0, 3, None)
    torch.cuda.synchronize()
    assert rc == 1 and bool((out == 7.0).all())


# ---- 2. the pool -------------------------------------------------------------------------------------------------------------

def _se_convs(C, S, seed, w1_scale=1.0, w2_scale=1.0):
    g = tc.gen(seed)
    fc1, fc2 = nn.Conv2d(C, S, 1), nn.Conv2d(S, C, 1)
    with torch.no_grad():
        fc1.weight.copy_(torch.randn(fc1.weight.shape, generator=g) * w1_scale / C ** 0.5)
        fc1.bias.copy_(torch.randn(S, generator=g) * 0.5)
        fc2.weight.copy_(torch.randn(fc2.weight.shape, generator=g) * w2_scale / S ** 0.5)
        fc2.bias.copy_(torch.randn(C, generator=g))
    return fc1.cuda(), fc2.cuda()


def _pooled_mean(x, pitch, fc1, fc2):
    """``opa_se_pool`` + ``opa_se_gate`` on ``x`` ([B, C, H, W], channels innermost, ``pitch`` floats between pixels) -> the mean [B, C]."""
    B, C, H, W = x.shape
    lib, vp = _lib.lib(), ctypes.c_void_p
    nbytes = lib.opa_se_workspace_bytes(B, H * W, C)
    assert nbytes == B * ((H * W + 511) // 512) * C * 8
    ws = torch.full((nbytes // 8,), float('nan'), dtype=torch.float64, device='cuda')
    gate, mean = torch.empty((B, C), device='cuda'), torch.full((B, C), float('nan'), device='cuda')
    assert lib.opa_se_pool(vp(x.data_ptr()), pitch, B, H * W, C, vp(ws.data_ptr()), nbytes, None) == 0
    assert lib.opa_se_gate(vp(ws.data_ptr()), nbytes, B, H * W, C, fc1.out_channels, vp(fc1.weight.data_ptr()), vp(fc1.bias.data_ptr()),
                           vp(fc2.weight.data_ptr()), vp(fc2.bias.data_ptr()), vp(gate.data_ptr()), vp(mean.data_ptr()), None) == 0
    assert ws.isfinite().all() and gate.isfinite().all()
    return mean


POOL_SHAPES = [(3, 72, 1, 1), (3, 72, 5, 5), (3, 72, 41, 41), (3, 960, 1, 1), (3, 960, 5, 5), (3, 960, 41, 41), (2, 72, 161, 161)]


@pytest.mark.parametrize('pitch', ['dense', 'strided'])
@pytest.mark.parametrize('shape', POOL_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_pool(shape, pitch):
    """The mean over the pixels (``se_gate``'s ``mean_out``) against the float64 mean; (2, 72, 161, 161) is the shape whose 25 921
    pixels are split over 51 workgroups per image.  The extra 2^-24 is one rounding of the result: torch's mean may be exact."""
    B, C, H, W = shape
    extra = 8 if pitch == 'strided' else 0
    wide = F.hardswish(torch.randn((B, C + extra, H, W), generator=tc.gen(H + C)) * 2.0).cuda().contiguous(memory_format=CL)
    x = wide[:, 4:4 + C] if extra else wide
    fc1, fc2 = _se_convs(C, 8, 1)
    x0 = x.clone()
    means = [_pooled_mean(x, C + extra, fc1, fc2) for _ in range(2)]
    if H * W > 1 or not extra:         # (a 1 x 1 slice: its pitch is the batch stride, which only the C entry points take)
        assert fused._pixel_stride(x) == C + extra and fused.se_gate_supported(x, fc1, fc2)
        mean = torch.full((B, C), float('nan'), device='cuda')
        fused.se_gate(x, fc1, fc2, mean_out=mean)
        assert torch.equal(mean, means[0])
    assert torch.equal(means[0], means[1]) and torch.equal(x, x0) and means[0].isfinite().all()
    ref64 = x.double().mean((2, 3))
    e0 = tc.e0(lambda: x.mean((2, 3)), ref64)
    one = 2.0 ** -24
    assert _report('pool %s %s' % ('x'.join(map(str, shape)), pitch), tc.errors(means[0], ref64), e0, extra=(one, one))


# ---- 3. gate and apply -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('C,S', [(72, 24), (960, 240)])
def test_gate_and_apply(C, S):
    B = 3
    se = network._SqueezeExcitation(C, S)
    fc1, fc2 = _se_convs(C, S, C + S, w1_scale=2.0, w2_scale=4.0)
    se.fc1, se.fc2 = fc1, fc2
    se = se.cuda()
    x = (F.hardswish(torch.randn((B, C, 5, 5), generator=tc.gen(C)) * 2.0) * 3.0).cuda().contiguous(memory_format=CL)

    def gate_of(module, t):
        return module.scale_activation(module.fc2(module.activation(module.fc1(module.avgpool(t))))).flatten(1)
    with torch.no_grad():
        ref64 = gate_of(copy.deepcopy(se).double(), x.double())
        e0 = tc.e0(lambda: gate_of(se, x), ref64)
        # all three pieces of the hardsigmoid occur (told by its argument: 6 * (1 / 6) need not be 1 to the last bit)
        m64 = copy.deepcopy(se).double()
        z = m64.fc2(m64.activation(m64.fc1(m64.avgpool(x.double())))).flatten(1)
        assert bool((z < -3.5).any()) and bool((z > 3.5).any()) and bool(((z > -2.5) & (z < 2.5)).any())
        assert bool((ref64[z < -3.5] == 0).all()) and bool((ref64[z > 3.5] > 0.999999).all())
        assert fused.se_gate_supported(x, se.fc1, se.fc2)
        got = fused.se_gate(x, se.fc1, se.fc2)
        assert tuple(got.shape) == (B, C) and torch.equal(got, fused.se_gate(x, se.fc1, se.fc2))
        assert _report('gate %d-%d-%d' % (C, S, C), tc.errors(got, ref64), e0)
        # the apply is one multiplication: bit for bit, dense and on a slice
        assert fused.scale_channels_supported(x, got)
        want = x * got[:, :, None, None]
        y = x.clone(memory_format=torch.preserve_format)
        assert fused.scale_channels_(y, got) is y and torch.equal(y, want)
        wide = torch.zeros((B, C + 8, 5, 5), device='cuda').contiguous(memory_format=CL)
        wide[:, 4:4 + C] = x
        fused.scale_channels_(wide[:, 4:4 + C], got)
        assert torch.equal(wide[:, 4:4 + C], want) and not wide[:, :4].any() and not wide[:, 4 + C:].any()


# ---- 4. the unit GEMM with hardswish and with a residual -----------------------------------------------------------------------

@pytest.mark.parametrize('K,N', [(16, 64), (72, 40), (672, 112), (960, 160)])
def test_unit_gemm_with_hardswish_and_with_residual(K, N):
    conv = tc.randomize_(nn.Conv2d(K, N, 1), K + N).cuda()
    x = torch.randn((2, K, 13, 11), generator=tc.gen(K)).cuda().contiguous(memory_format=CL)
    res = torch.randn((2, N, 13, 11), generator=tc.gen(N)).cuda().contiguous(memory_format=CL)
    wide = torch.randn((2, N + 6, 13, 11), generator=tc.gen(N + 1)).cuda().contiguous(memory_format=CL)
    ok = True
    with torch.no_grad():
        conv64 = copy.deepcopy(conv).double()
        lin64 = conv64(x.double())
        assert fused.unit_conv_x3_supported(conv, x)
        got = fused.conv1x1_unit_x3(conv, x, act=fused.ACT_HARDSWISH)
        ref64 = F.hardswish(lin64)
        ok &= _report('unit+hardswish K %d N %d' % (K, N), tc.errors(got, ref64), tc.e0(lambda: F.hardswish(conv(x)), ref64))
        for layout, r in (('dense', res), ('slice', wide[:, 2:2 + N])):
            assert fused.unit_conv_x3_supported(conv, x, residual=r)
            r0 = r.clone()
            got = fused.conv1x1_unit_x3(conv, x, residual=r, act=fused.ACT_NONE)
            assert torch.equal(r, r0) and got.is_contiguous(memory_format=CL)
            ref64 = lin64 + r.double()
            ok &= _report('unit+residual K %d N %d %s' % (K, N, layout), tc.errors(got, ref64), tc.e0(lambda: conv(x) + r, ref64))
        # the activation behind the residual, and the codes that are the existing kernels
        got = fused.conv1x1_unit_x3(conv, x, residual=res, act=fused.ACT_HARDSWISH)
        ref64 = F.hardswish(lin64 + res.double())
        ok &= _report('unit+residual+hardswish K %d N %d' % (K, N), tc.errors(got, ref64), tc.e0(lambda: F.hardswish(conv(x) + res), ref64))
        assert torch.equal(fused.conv1x1_unit_x3(conv, x, residual=res, act=fused.ACT_RELU),
                           F.relu(fused.conv1x1_unit_x3(conv, x, residual=res, act=fused.ACT_NONE)))
    assert ok        # (act= and relu= are one call of one entry point; the C twins: test_unit_gemm_entry_points_are_one_kernel)


SENTINEL = 12345.5


@pytest.mark.parametrize('partner', [False, True], ids=['alone', 'partner'])
@pytest.mark.parametrize('act', [0, 1])
@pytest.mark.parametrize('N,terms', [(40, 6), (128, 6), (40, 9)])
def test_unit_gemm_entry_points_are_one_kernel(N, terms, act, partner, monkeypatch):
    """``opa_gemm_unit_bias_act_f32x3(relu=a)`` against ``opa_gemm_unit_act_f32x3(residual NULL, act=a)``, raw, each into its own
    sentinel-filled output: bit for bit.  K = 72 (a K tail), M = 286 (two full 128-row tiles and a tail); N = 40: the 64-wide tile
    with an N tail, N = 128: the 128-wide tile.  The launcher calls the second one only."""
    K, shape = 72, (2, 13, 11)
    conv = tc.randomize_(nn.Conv2d(K, N, 1), K + N).cuda()
    x = torch.randn((2, K, 13, 11), generator=tc.gen(K)).cuda().contiguous(memory_format=CL)
    third = torch.randn((2, N, 13, 11), generator=tc.gen(N)).cuda().contiguous(memory_format=CL) if partner else None
    w3, bp = fused._unit_weight_of(conv)
    outs = [torch.full((2, 2 * N if partner else N, 13, 11), SENTINEL, device='cuda').contiguous(memory_format=CL) for _ in range(2)]
    lib, vp = _lib.lib(), ctypes.c_void_p
    head = (vp(x.data_ptr()), K, vp(w3.data_ptr()), vp(bp.data_ptr()), vp(third.data_ptr()) if partner else None, N if partner else 0)
    tail = (shape[0] * shape[1] * shape[2], N, K, act, terms, None)
    assert lib.opa_gemm_unit_bias_act_f32x3(*head, vp(outs[0].data_ptr()), *tail) == 0
    assert lib.opa_gemm_unit_act_f32x3(*head, None, 0, vp(outs[1].data_ptr()), *tail) == 0
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and outs[0].isfinite().all() and not bool((outs[0] == SENTINEL).any())
    assert bool((outs[0][:, 1::2] if partner else outs[0]).lt(0).any()) == (act == 0)      # (the product's channels: the odd ones next to a partner)
    monkeypatch.setattr(fused, 'X3_TERMS', terms)
    assert torch.equal(fused.conv1x1_unit_x3(conv, x, relu=bool(act), partner=third), outs[1])
    assert torch.equal(fused.conv1x1_unit_x3(conv, x, act=act, partner=third), outs[1])


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['float32', 'bfloat16'])
@pytest.mark.parametrize('act', [0, 1])
@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('k', [3, 5])
def test_depthwise_entry_points_are_one_kernel(k, stride, act, dtype):
    """``opa_dwconv_bias_act(relu=a)`` against ``opa_dwconv_act(act=a)``, raw, with a bias, each into its own sentinel-filled
    output: bit for bit.  The launcher calls the second one only."""
    C, g = 8, tc.gen(10 * k + stride)
    x = torch.randn((2, C, 7, 5), generator=g).to(dtype).cuda().contiguous(memory_format=CL)
    taps = (torch.randn((k * k, C), generator=g) * (2.0 / (k * k)) ** 0.5).to(dtype).cuda()
    b = (torch.randn(C, generator=g) * 0.5).to(dtype).cuda()
    ho, wo = (7 + 2 * (k // 2) - k) // stride + 1, (5 + 2 * (k // 2) - k) // stride + 1
    outs = [torch.full((2, C, ho, wo), SENTINEL, dtype=dtype, device='cuda').contiguous(memory_format=CL) for _ in range(2)]
    sentinel = outs[0].flatten()[0].clone()
    lib, vp = _lib.lib(), ctypes.c_void_p
    for fn, out in ((lib.opa_dwconv_bias_act, outs[0]), (lib.opa_dwconv_act, outs[1])):
        assert fn(vp(x.data_ptr()), C, vp(taps.data_ptr()), vp(b.data_ptr()), vp(out.data_ptr()), C, 2, 7, 5, C, k, stride,
                  fused._DTYPES[dtype], act, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and outs[0].isfinite().all() and not bool((outs[0] == sentinel).any())
    assert bool((outs[0] < 0).any()) == (act == 0)
    assert torch.equal(fused.dwconv_bias_act(x, taps, b, k, stride, relu=bool(act)), outs[1])
    assert torch.equal(fused.dwconv_bias_act(x, taps, b, k, stride, act=act), outs[1])


def test_residual_with_partner_is_refused():
    conv = tc.randomize_(nn.Conv2d(72, 40, 1), 0).cuda()
    x = torch.randn((2, 72, 13, 11), device='cuda').contiguous(memory_format=CL)
    third = torch.randn((2, 40, 13, 11), device='cuda').contiguous(memory_format=CL)
    assert not fused.unit_conv_x3_supported(conv, x, partner=third, residual=third)
    w3, bp = fused._unit_weight_of(conv)
    out = torch.full((2, 80, 13, 11), 7.0, device='cuda').contiguous(memory_format=CL)
    vp = ctypes.c_void_p
    rc = _lib.lib().opa_gemm_unit_act_f32x3(vp(x.data_ptr()), 72, vp(w3.data_ptr()), vp(bp.data_ptr()), vp(third.data_ptr()), 40,
                                            vp(third.data_ptr()), 40, vp(out.data_ptr()), 2 * 13 * 11, 40, 72, 0, 6, None)
    torch.cuda.synchronize()
    assert rc == 1 and 'residual' in _lib.lib().opa_last_error().decode()          # OPA_ERR_INVALID_ARGUMENT
    assert bool((out == 7.0).all()), 'something was launched'
    rc = _lib.lib().opa_gemm_unit_act_f32x3(vp(x.data_ptr()), 72, vp(w3.data_ptr()), vp(bp.data_ptr()), None, 0,
                                            vp(third.data_ptr()), 40, vp(out.data_ptr()), 2 * 13 * 11, 40, 72, 3, 6, None)
    assert rc == 1


# ---- 5. block routes -----------------------------------------------------------------------------------------------------------

# in, kernel, expanded, out, SE, hardswish, stride
BLOCKS = {'large1': (16, 3, 16, 16, False, False, 1), 'large4': (24, 5, 72, 40, True, False, 2), 'large7': (40, 3, 240, 80, False, True, 2),
          'large12': (112, 3, 672, 112, True, True, 1), 'small1': (16, 3, 16, 16, True, False, 2)}


def _trace_of(spec):
    return (['unit'] if spec[2] != spec[0] else []) + ['dwconv'] + (['se_gate', 'scale'] if spec[4] else []) + ['unit']


def _make(spec, seed):
    return tc.randomize_(network._MBV3Block(*spec), seed)


@functools.lru_cache(maxsize=None)
def _reference(spec, seed):
    """-> (the unfused block on the CPU, x, ref64, e0)."""
    module = _make(spec, seed)
    x = torch.randn((2, spec[0], 13, 11), generator=tc.gen(1000 + seed)).cuda().contiguous(memory_format=CL)
    with torch.no_grad():
        ref64 = copy.deepcopy(module).double().cuda()(x.double())
        plain = copy.deepcopy(module).cuda().to(memory_format=CL)
        e0 = tc.e0(lambda: plain(x), ref64)
    assert e0[0] > 0 and ref64.isfinite().all()
    return module, x, ref64, e0


@pytest.mark.parametrize('block', list(BLOCKS))
def test_block_route(rec, block):
    spec = BLOCKS[block]
    ok = True
    for seed in SEEDS:
        module, x, ref64, e0 = _reference(spec, seed)
        opt = rec.watch(tc.optimized(module).cuda().to(memory_format=CL))
        got, trace = tc.forward_checks(opt, x, rec)
        assert trace == _trace_of(spec), trace
        assert fused.choices() == {}, 'the route made a choice-table entry'
        assert got.is_contiguous(memory_format=CL) and got.shape == ref64.shape
        ok &= _report('block %s | %s | seed %d' % (block, ' '.join(trace), seed), tc.errors(got, ref64), e0)
        # switched off: torch's forward, convolution for convolution
        fused.MBV3 = False
        off, trace = tc.forward_checks(opt, x, rec)
        convs = [name for name, m in opt.named_modules() if isinstance(m, nn.Conv2d)]
        assert trace == ['miopen:' + name for name in convs], trace
        assert float((off - got).abs().max()) <= 1e-4 * float(off.abs().max())
        fused.MBV3 = True
    assert ok


def test_block_route_declines(rec):
    """bfloat16, autocast and a tensor that is not channels-last take the torch forward."""
    spec = BLOCKS['large12']
    module, x, _, _ = _reference(spec, 0)
    opt = rec.watch(tc.optimized(module).cuda().to(memory_format=CL))
    assert opt._route_supported(x)
    assert not opt._route_supported(x.contiguous()) and not opt._route_supported(x.bfloat16())
    with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
        assert not opt._route_supported(x)
        rec.trace.clear()
        opt(x)
    assert rec.trace and all(t.startswith('miopen:') for t in rec.trace), rec.trace


def test_block_route_declines_a_tensor_autograd_follows(rec):
    """A block without an expanding convolution hands ``x`` itself to the stencil: a tensor that autograd follows takes the torch
    forward and keeps its graph; detached and under ``no_grad`` the same block takes the route.  Stride 1: the block's input is
    also the residual operand of the projecting GEMM; stride 2: the stencil is the only kernel that reads ``x``."""
    for stride in (1, 2):
        opt = rec.watch(tc.optimized(_make((16, 3, 16, 16, False, False, stride), 0)).cuda().to(memory_format=CL))
        with torch.enable_grad():
            x = torch.randn((1, 16, 5, 5), generator=tc.gen(3)).cuda().contiguous(memory_format=CL).requires_grad_(True)
            assert not opt._route_supported(x), stride
            rec.trace.clear()
            out = opt(x)
        assert rec.trace and all(t.startswith('miopen:') for t in rec.trace), rec.trace
        assert out.grad_fn is not None
        with torch.no_grad():
            assert opt._route_supported(x.detach())
            rec.trace.clear()
            opt(x.detach())
        assert rec.trace == ['dwconv', 'unit'], rec.trace


# ---- 6. operands follow the parameters ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('block', ['large12', 'small1'])
def test_forward_after_load_state_dict(rec, block):
    spec = BLOCKS[block]
    _, x, _, _ = _reference(spec, 0)
    module1, _, _, _ = _reference(spec, 1)
    opt = tc.optimized(_make(spec, 0)).cuda().to(memory_format=CL)
    other = tc.optimized(module1).cuda().to(memory_format=CL)
    with torch.no_grad():
        before = opt(x)
        opt.load_state_dict(other.state_dict(), strict=True)
        rec.trace.clear()
        after = opt(x)
        assert rec.trace == _trace_of(spec), rec.trace
        ref64 = copy.deepcopy(module1).double().cuda()(x.double())
        plain = copy.deepcopy(module1).cuda().to(memory_format=CL)
        e0 = tc.e0(lambda: plain(x), ref64)
        assert not torch.equal(before, after)
        assert torch.equal(after, other(x)), 'stale operand: max |delta| %.3g' % (after - other(x)).abs().max().item()
    assert _report('block %s after load_state_dict' % block, tc.errors(after, ref64), e0)


# ---- 7. whole networks ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['mobilenetv3large', 'mobilenetv3small'])
def test_whole_network(rec, name):
    """cocokp heads on [2, 3, 65, 49]: the optimized channels-last model against the double model, both head outputs.  The heads'
    1x1 convolutions are pinned to the split-operand kernel (960 and 576 input channels: ``head_conv_x3``), so nothing is timed."""
    net = tc.randomize_(network.factory(name), 7)
    x = torch.randn((2, 3, 65, 49), generator=tc.gen(8)).cuda().contiguous(memory_format=CL)
    with torch.no_grad():
        ref64 = copy.deepcopy(net).double().cuda()(x.double())
        plain = copy.deepcopy(net).cuda().to(memory_format=CL)
        fused.FORCE_PICK = 'conv'                                      # e0: torch's own convolutions, the heads' too
        e0s = [tc.e0(lambda: plain(x)[i], r) for i, r in enumerate(ref64)]
        fused.FORCE_PICK = 'x3'
        opt = rec.watch(network.optimize_for_inference_(copy.deepcopy(net)).cuda().to(memory_format=CL))
        rec.trace.clear()
        got = opt(x)
        trace = list(rec.trace)
        again = opt(x)
    blocks = [m for m in opt.base_net.backbone if isinstance(m, network._MBV3Block)]
    n_se = sum(1 for m in blocks if m.se is not None)
    assert trace.count('dwconv') == len(blocks) and trace.count('se_gate') == n_se and trace.count('scale') == n_se
    assert trace.count('unit') == len(blocks) + sum(1 for m in blocks if m.expand is not None) + 1
    assert [t for t in trace if t.startswith('miopen:')] == ['miopen:base_net.backbone.0.0'], 'only the stem is torch\'s'
    ok = True
    for i, (g, a, r) in enumerate(zip(got, again, ref64)):
        assert torch.equal(g, a) and g.isfinite().all()
        ok &= _report('%s head %d' % (name, i), tc.errors(g, r), e0s[i])
    assert ok


# ---- 8. Predictor ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('on_device', [False, True], ids=['host-preprocess', 'device-preprocess'])
def test_predictor_smoke(on_device):
    from openpifpaf_amd.predictor import Predictor
    rng = np.random.default_rng(3)
    frames = [rng.integers(0, 256, (48, 64, 3), dtype=np.uint8), rng.integers(0, 256, (64, 40, 3), dtype=np.uint8)]
    saved = Predictor.long_edge, Predictor.batch_size, Predictor.device_preprocess
    Predictor.long_edge, Predictor.batch_size, Predictor.device_preprocess = 65, 2, on_device
    try:
        pred = Predictor('mobilenetv3small')
        assert isinstance(pred.model_cpu.base_net, network.MobileNetV3)
        out = [p for p, _, _ in pred.numpy_images(frames)]
    finally:
        Predictor.long_edge, Predictor.batch_size, Predictor.device_preprocess = saved
    assert len(out) == 2 and all(isinstance(p, list) for p in out)
