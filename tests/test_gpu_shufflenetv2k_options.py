"""The ShuffleNetV2K options on the GPU: the depthwise stencil with a 7 x 7 window and a dilation (``opa_dwconv_dilated_act``,
``csrc/dwconv.hip``), the unit routes built on it (``network._InvertedResidualK`` dilated, 3 x 3, 7 x 7, a ``conv5`` stage, LeakyReLU),
whole networks under each option and a ``Predictor`` with ``stage4_dilation=2``.

The kernel alone is held to the DERIVED bound of ``pointwise_common.dw_reference``, restated here with a dilation: against the float64
convolution of the operands as stored, ``gamma_n (sum |x| |w| + |b|)`` with ``n = k * k + 1`` and ``u = 2^-24`` for a float32
accumulation in any order; ReLU is 1-Lipschitz, so the bound carries over; hardswish (act 2) has slope at most 1.5 and is evaluated
in float32 with three roundings (``x * min(max(x + 3, 0), 6) / 6``, each factor within ``u`` of its exact value), so
``1.5 bound + 4 u |hardswish(ref)|``; a bfloat16 result is rounded once more, ``2^-8 (|ref| + bound)``.

Routes and networks use the criterion of ``test_gpu_resnet_variants.py`` / ``test_gpu_unit_routes.py``: ``ref64`` the unfused module
in ``double()``; ``e0`` the error against ``ref64`` of torch's OWN float32 forward of the same module, the median of nine calls,
never of the code under test; ``err = max |got - ref64| / max |ref64|`` and the same as an rms; required ``err <= K * e0`` with K = 2
(two independent errors of size ``e0``), raised to 4 or 8 only for a whole family with the per-seed lines on record.  Every case
prints a ``SHUFFLEOPT`` line (``pytest -s``); the lines of a run are kept in ``profiles/shufflenetv2k_options/route_errors.log``.
Worst err/e0 of that log (max, rms) and the K it gives, per family (``K``):
  unit      dilated, 3 x 3, 7 x 7 units and the conv5 pair, 3 seeds each      0.69, 0.68  -> 2
  leaky     the LeakyReLU unit (stencil + torch's 1x1 convolutions)           1.18, 1.01  -> 2
  declined  units whose depthwise convolution the stencil declines            1.20, 1.02  -> 2
  network   whole shufflenetv2k16 networks, every pick on its kernel side     0.83, 0.87  -> 2
The kernel's worst ``|err| / bound`` is 0.27 in float32 and 0.994 in bfloat16 (the last rounding's half unit, reached by design)."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from openpifpaf_amd import _lib, fused, headmeta, network

import pointwise_common as pc
import trunk_common as tc

pytestmark = pytest.mark.gpu

SEEDS = (0, 1, 2)
K = {'unit': 2, 'leaky': 2, 'declined': 2, 'network': 2}
CL = torch.channels_last
# every (k, stride, dilation) the entry point accepts
KSD = [(k, s, 1) for k in (3, 5, 7) for s in (1, 2)] + [(k, 1, d) for k in (3, 5, 7) for d in (2, 4)]
_LAUNCHERS = {'conv1x1_unit_x3': 'unit', 'dwconv_bias_act': 'dwconv', 'channel_interleave': 'interleave', 'bias_act_': 'bias_act',
              'conv1x1_bias_act': 'gemm', 'conv1x1_bias_act_x3': 'gemm3', 'head_conv_x3': 'head_x3', 'head_epilogue': 'head_epilogue'}
_vp = ctypes.c_void_p


def _report(family, what, err, e0):
    return tc.report('SHUFFLEOPT', '%s %s' % (family, what), err, e0, K[family], show_k=True)


@pytest.fixture
def rec(monkeypatch):
    """Launch recorder (``test_gpu_resnet_variants.py``'s recipe); nothing may be timed: ``FORCE_PICK = 'x3'``, an empty choice table."""
    return tc.recorder(monkeypatch, _LAUNCHERS, ('X3_UNIT', 'X3_HEAD'), force_pick='x3')


# ---- 1. the stencil kernel ---------------------------------------------------------------------------------------------------------

def dw_reference(x, w_taps, bias, k, s, act, dilation=1):
    """``pointwise_common.dw_reference`` with ``dilation=`` and the activation code (module docstring) -> (ref, bound), float64."""
    C = x.shape[1]
    w4 = w_taps.double().t().reshape(C, 1, k, k)
    b = None if bias is None else bias.double()
    pad = k // 2 * dilation
    ref = F.conv2d(x.double(), w4, b, stride=s, padding=pad, dilation=dilation, groups=C)
    mag = F.conv2d(x.double().abs(), w4.abs(), None if b is None else b.abs(), stride=s, padding=pad, dilation=dilation, groups=C)
    n, u = k * k + 1, 2.0 ** -24
    bound = n * u / (1 - n * u) * mag
    if act == 1:
        ref = ref.clamp_min(0)
    elif act == 2:
        ref = ref * (ref + 3).clamp(0, 6) / 6
        bound = 1.5 * bound + 4 * u * ref.abs()
    if x.dtype == torch.bfloat16:
        bound = bound + 2.0 ** -8 * (ref.abs() + bound)
    return ref, bound


def _dw_run(dtype, k, s, d, x, w, b, act, xs=None, x_off=0, os_=None, o_off=0, expect=0):
    """``opa_dwconv_dilated_act`` on the layout: the input inside a NaN-filled pixel grid, the output inside a sentinel buffer.
    -> the output [B, C, Ho, Wo] on the CPU; everything outside it was checked to hold the sentinel (``expect`` 1: a refusal, ALL
    of the buffer)."""
    B, C, H, W = x.shape
    xs, os_ = xs or C, os_ or C
    dt = pc.DTYPES[dtype]
    Ho, Wo = fused.dwconv_out_hw(H, W, k, s, d) if expect == 0 else (H, W)
    xbuf = torch.full((B * H * W * xs + 2 * pc.PAD,), float('nan'), dtype=dt, device='cuda')
    xv = xbuf.as_strided((B, C, H, W), (H * W * xs, 1, W * xs, xs), pc.PAD + x_off)
    xv.copy_(x)
    obuf = torch.full((B * Ho * Wo * os_ + 2 * pc.PAD,), pc.SENTINEL, dtype=dt, device='cuda')
    ov = obuf.as_strided((B, C, Ho, Wo), (Ho * Wo * os_, 1, Wo * os_, os_), pc.PAD + o_off)
    wg, bg = w.cuda(), (b.cuda() if b is not None else None)
    rc = _lib.lib().opa_dwconv_dilated_act(_vp(xv.data_ptr()), xs, _vp(wg.data_ptr()), _vp(bg.data_ptr()) if bg is not None else None,
                                           _vp(ov.data_ptr()), os_, B, H, W, C, k, s, d, 0 if dtype == 'float32' else 2, act, None)
    torch.cuda.synchronize()
    assert rc == expect, _lib.lib().opa_last_error()
    got = ov.cpu()
    if expect == 0:
        ov.fill_(pc.SENTINEL)
    assert (obuf == pc.SENTINEL).all(), 'written outside the output pixels'
    return got, xv


# (H, W): smaller than the dilated window (3 x 5 with K = 5, D = 2; 2 x 2 with K = 7, D = 4); widths 5 and 9, no multiples of the strip
SHAPES = [(3, 5), (2, 2), (4, 9), (13, 11)]


@pytest.mark.parametrize('dtype', ['float32', 'bfloat16'])
@pytest.mark.parametrize('k,s,d', KSD)
def test_kernel_against_float64(k, s, d, dtype):
    worst = 0.0
    for n, ((H, W), C, B) in enumerate((hw, C, B) for hw in SHAPES for C in (8, 6, 5) for B in (1, 3)):
        x, w, b = pc.dw_inputs(pc._dw(dtype, k, s, B, H, W, C), seed=n)
        assert tuple(w.shape) == (k * k, C)
        for with_bias in (True, False):
            for act in (0, 1, 2):
                bias = b if with_bias else None
                got, xv = _dw_run(dtype, k, s, d, x, w, bias, act)
                ref, bound = dw_reference(x, w, bias, k, s, act, d)
                assert got.shape == ref.shape and bool(got.isfinite().all())
                ratio = float(((got.double() - ref).abs() / bound.clamp_min(1e-300)).max())
                worst = max(worst, ratio)
                assert ratio <= 1.0, ((H, W), C, B, with_bias, act, ratio)
                # the Python entry point: the same bits, and it is the route for this combination
                assert fused.dwconv_supported(xv, k, s, d)
                py = fused.dwconv_bias_act(xv, w.cuda(), bias.cuda() if with_bias else None, k, s, act=act, dilation=d)
                assert py.is_contiguous(memory_format=CL) and torch.equal(pc.bits(py.cpu()), pc.bits(got))
        # where the older entry point accepts the call too: bit for bit its result
        if k in (3, 5) and d == 1:
            ho, wo = fused.dwconv_out_hw(H, W, k, s)
            ov = torch.empty((B, ho, wo, C), dtype=pc.DTYPES[dtype], device='cuda')
            rc = _lib.lib().opa_dwconv_act(_vp(xv.data_ptr()), C, _vp(w.cuda().data_ptr()), None, _vp(ov.data_ptr()), C, B, H, W, C, k, s,
                                           0 if dtype == 'float32' else 2, 0, None)
            torch.cuda.synchronize()
            assert rc == 0
            new, _ = _dw_run(dtype, k, s, d, x, w, None, 0)
            assert torch.equal(pc.bits(ov.permute(0, 3, 1, 2).cpu()), pc.bits(new))
    print('SHUFFLEOPT kernel k %d s %d d %d %s | worst |err| / bound %.3f' % (k, s, d, dtype, worst))


@pytest.mark.parametrize('dtype', ['float32', 'bfloat16'])
@pytest.mark.parametrize('k,s,d', KSD)
def test_kernel_on_channel_slices(k, s, d, dtype):
    """An input slice (pixel stride 16; offset 8 floats: V = 4, offset 1: V = 1) and an output slice inside a wider sentinel buffer:
    the bits of the dense call."""
    B, C, H, W = 3, 8, 5, 9
    x, w, b = pc.dw_inputs(pc._dw(dtype, k, s, B, H, W, C), seed=7)
    dense, _ = _dw_run(dtype, k, s, d, x, w, b, 1)
    ref, bound = dw_reference(x, w, b, k, s, 1, d)
    assert bool(((dense.double() - ref).abs() <= bound).all())
    for kw in (dict(xs=16, x_off=8), dict(xs=16, x_off=1), dict(os_=16, o_off=8), dict(os_=24, o_off=3), dict(xs=16, x_off=8, os_=16, o_off=8)):
        got, _ = _dw_run(dtype, k, s, d, x, w, b, 1, **kw)
        assert torch.equal(pc.bits(got), pc.bits(dense)), kw


@pytest.mark.parametrize('dtype', ['float32', 'bfloat16'])
@pytest.mark.parametrize('k,d', [(5, 2), (7, 1), (7, 4), (3, 4)])
def test_nan_and_inf_go_where_the_window_says(k, d, dtype):
    """One NaN and one Inf in the input: the non-finite outputs are exactly the positions whose dilated window covers them (a wrong
    tap offset, which random data averages away, moves them)."""
    B, C, H, W = 2, 8, 13, 11
    x, w, _ = pc.dw_inputs(pc._dw(dtype, k, 1, B, H, W, C, bias=False), seed=3)
    x = (x.float() / pc.dw_channel_scales(C).view(1, C, 1, 1).float()).to(x.dtype)
    w = w.abs() + 0.25                                            # no tap is zero: every covered output sees the value
    clean, _ = _dw_run(dtype, k, 1, d, x, w, None, 0)
    P = k // 2
    for value, (b, c, y, xx) in ((float('nan'), (1, 5, 6, 4)), (float('inf'), (0, 0, 0, 10)), (float('-inf'), (1, 7, 12, 0))):
        xp = x.clone()
        xp[b, c, y, xx] = value
        got, _ = _dw_run(dtype, k, 1, d, xp, w, None, 0)
        hit = torch.zeros_like(clean, dtype=torch.bool)
        for yo in range(H):
            for xo in range(W):
                if (y - yo) % d == 0 and abs(y - yo) <= P * d and (xx - xo) % d == 0 and abs(xx - xo) <= P * d:
                    hit[b, c, yo, xo] = True
        assert hit.any() and torch.equal(~got.isfinite(), hit), 'the value is missing from an output that reads it, or reached another'
        assert torch.equal(pc.bits(got[~hit]), pc.bits(clean[~hit]))


def test_a_refused_call_writes_nothing():
    x, w, b = pc.dw_inputs(pc._dw('float32', 5, 1, 2, 5, 9, 8), seed=1)
    for k, s, d, act in ((9, 1, 1, 0), (5, 1, 3, 0), (5, 2, 2, 0), (5, 1, 2, 3), (4, 1, 1, 0)):
        w_any = torch.zeros((81, 8))
        _dw_run('float32', k, s, d, x, w_any, b, act, expect=1)
    assert torch.cuda.current_stream().query() and float(torch.ones(1, device='cuda').sum()) == 1.0      # no sticky launch error


# ---- 2. unit routes ------------------------------------------------------------------------------------------------------------------

def _unit(inp, oup, first, seed, **kw):
    return tc.randomize_(network._InvertedResidualK(inp, oup, first, **kw), seed)


def _pair(seed, **kw):
    return tc.randomize_(nn.Sequential(network._InvertedResidualK(1392, 1392, False, **kw), network._InvertedResidualK(1392, 1392, False, **kw)), seed)


FIRST, LATER = ['dwconv', 'unit', 'unit', 'dwconv', 'unit'], ['unit', 'dwconv', 'unit']
UNITS = {
    'dilated-first': (functools.partial(_unit, 348, 696, True, stride=1, dilation=2), 348, FIRST),       # stage 4's first unit under stage4_dilation=2
    'dilated-later': (functools.partial(_unit, 696, 696, False, dilation=2), 696, LATER),
    'dilated4-later': (functools.partial(_unit, 696, 696, False, dilation=4), 696, LATER),
    'kernel3': (functools.partial(_unit, 348, 348, False, kernel_size=3), 348, LATER),
    'kernel7': (functools.partial(_unit, 348, 348, False, kernel_size=7), 348, LATER),
    'kernel7-first': (functools.partial(_unit, 24, 348, True, stride=2, kernel_size=7), 24, FIRST),
    'conv5-pair': (functools.partial(_pair, dilation=2), 1392, LATER + LATER),
}


@functools.lru_cache(maxsize=None)
def _reference(make, shape, seed):
    """-> (the unfused module on the CPU, x, ref64, e0).  ``x`` has both signs: the unit's first 1x1 convolution sees negative inputs
    and, behind the random batch norms, negative pre-activations."""
    module = make(seed)
    x = torch.randn(shape, generator=tc.gen(1000 + seed)).cuda().contiguous(memory_format=CL)
    with torch.no_grad():
        ref64 = copy.deepcopy(module).double().cuda()(x.double())
        plain = copy.deepcopy(module).cuda().to(memory_format=CL)
        e0 = tc.e0(lambda: plain(x), ref64)
    assert e0[0] > 0 and ref64.isfinite().all()
    return module, x, ref64, e0


@pytest.mark.parametrize('unit', list(UNITS))
def test_unit_route(rec, unit):
    make, channels, route = UNITS[unit]
    shape = (2, channels, 13, 11)
    ok = True
    for seed in SEEDS:
        module, x, ref64, e0 = _reference(make, shape, seed)
        opt = rec.watch(tc.optimized(module).cuda().to(memory_format=CL))
        got, trace = tc.forward_checks(opt, x, rec)
        assert trace == route, trace
        assert not [t for t in trace if t.startswith('miopen:')], trace
        assert fused.choices() == {}, 'the route made a choice-table entry'
        assert got.is_contiguous(memory_format=CL) and got.shape == ref64.shape
        ok &= _report('unit', '%s | %s | seed %d' % (unit, ' '.join(trace), seed), tc.errors(got, ref64), e0)
        fused.FORCE_PICK = 'conv'               # the other side of the pick: the stencil, torch's 1x1 convolutions, the interleave
        off, trace = tc.forward_checks(opt, x, rec)
        assert 'unit' not in trace and 'dwconv' in trace and not [t for t in trace if t.endswith('branch2.3') or t.endswith('branch1.0')], trace
        assert float((off - got).abs().max()) <= 1e-4 * float(off.abs().max())
        _report('unit', '%s | %s | seed %d' % (unit, ' '.join(trace), seed), tc.errors(off, ref64), e0)          # (printed, not judged here)
        fused.FORCE_PICK = 'x3'
    assert ok


def test_leaky_relu_unit(rec):
    """The GEMM's epilogue applies a ReLU, so a LeakyReLU unit takes the stencil + torch's 1x1 convolutions + torch's LeakyReLU; a
    ReLU in its place would be wrong by order one: the float64 ReLU unit differs from the float64 leaky unit by more than 100 x the bound."""
    ok = True
    for first, channels in ((False, 696), (True, 348)):
        make = functools.partial(_unit, channels, 696, first, stride=1, dilation=2, leaky_relu=True)
        for seed in SEEDS:
            module, x, ref64, e0 = _reference(make, (2, channels, 13, 11), seed)
            assert all(isinstance(m, nn.LeakyReLU) for m in (module.branch2[2], module.branch2[7]))
            opt = rec.watch(tc.optimized(module).cuda().to(memory_format=CL))
            assert not opt._unit_route_supported(x)
            got, trace = tc.forward_checks(opt, x, rec)
            assert trace.count('dwconv') == (2 if first else 1) and 'unit' not in trace and 'interleave' in trace, trace
            assert not [t for t in trace if t.endswith('branch2.3') or t.endswith('branch1.0')], trace
            err = tc.errors(got, ref64)
            ok &= _report('leaky', 'first %d | %s | seed %d' % (first, ' '.join(trace), seed), err, e0)
            relu = _unit(channels, 696, first, seed, stride=1, dilation=2)          # the same seed: the same parameters
            with torch.no_grad():
                wrong64 = relu.double().cuda()(x.double())
            wrong = tc.errors(wrong64, ref64)
            assert wrong[0] > 100 * K['leaky'] * e0[0] and wrong[1] > 100 * K['leaky'] * e0[1], (wrong, e0)
    assert ok


@pytest.mark.parametrize('unit', ['dilated-first', 'dilated-later', 'kernel7'])
def test_forward_after_load_state_dict(rec, unit):
    make, channels, route = UNITS[unit]
    _, x, _, _ = _reference(make, (2, channels, 13, 11), 0)
    opt = tc.optimized(make(0)).cuda().to(memory_format=CL)
    other = tc.optimized(make(1)).cuda().to(memory_format=CL)
    with torch.no_grad():
        before = opt(x)
        opt.load_state_dict(other.state_dict(), strict=True)
        rec.trace.clear()
        after = opt(x)
        assert rec.trace == route, rec.trace
        assert not torch.equal(before, after)
        assert torch.equal(after, other(x)), 'stale operand: max |delta| %.3g' % (after - other(x)).abs().max().item()


def test_unit_route_declines(rec):
    """An NCHW input, dilation 3 and kernel width 9 take torch's depthwise convolution and stay correct."""
    ok = True
    make, channels, _ = UNITS['dilated-later']
    module, x, ref64, e0 = _reference(make, (2, channels, 13, 11), 0)
    opt = rec.watch(tc.optimized(module).cuda())                              # weights and input NCHW: so is every activation
    with torch.no_grad():
        assert not fused.dwconv_supported(torch.randn((2, 348, 13, 11), device='cuda'), 5, 1, 2)
        rec.trace.clear()
        got = opt(x.contiguous())
    assert 'dwconv' not in rec.trace and 'unit' not in rec.trace and 'miopen:branch2.3' in rec.trace, rec.trace
    ok &= _report('declined', 'not channels-last | %s' % ' '.join(rec.trace), tc.errors(got, ref64), e0)
    for what, kw in (('dilation 3', dict(dilation=3)), ('kernel width 9', dict(kernel_size=9))):
        make = functools.partial(_unit, 348, 348, False, **kw)
        module, x, ref64, e0 = _reference(make, (2, 348, 13, 11), 0)
        opt = rec.watch(tc.optimized(module).cuda().to(memory_format=CL))
        dw = opt.branch2[3]
        with torch.no_grad():
            h = torch.randn((2, 174, 13, 11), device='cuda').contiguous(memory_format=CL)
            assert not fused.dwconv_supported(h, dw.kernel_size[0], 1, dw.dilation[0]) and not opt._unit_route_supported(x)
            rec.trace.clear()
            got = opt(x)
        assert 'dwconv' not in rec.trace and 'unit' not in rec.trace and 'miopen:branch2.3' in rec.trace, rec.trace
        ok &= _report('declined', '%s | %s' % (what, ' '.join(rec.trace)), tc.errors(got, ref64), e0)
    assert ok


# ---- 3. whole networks, predictor ----------------------------------------------------------------------------------------------------

def _net(seed, **options):
    base = network.ShuffleNetV2K('shufflenetv2k16', **options)
    heads = [network.CompositeField4(m, base.out_features) for m in headmeta.cocokp_metas()]
    return tc.randomize_(network.Shell(base, heads), seed)


def _whole(rec, what, net):
    """The optimized channels-last net against the double net, per head -> (launch trace, every head within the bound)."""
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
    ok = True
    for i, (g, r) in enumerate(zip(got, ref64)):
        assert g.isfinite().all() and g.shape == r.shape
        ok &= _report('network', '%s head %d' % (what, i), tc.errors(g, r), e0s[i])
    depthwise = ['miopen:' + n for n, m in opt.named_modules() if isinstance(m, nn.Conv2d) and m.groups > 1]
    assert depthwise and not [t for t in trace if t in depthwise], [t for t in trace if t in depthwise]
    return trace, ok


NETWORKS = {
    'dilation2': (dict(stage4_dilation=2), 8, 4),
    'conv5_stage_dilation2': (dict(conv5_as_stage=True, stage4_dilation=2), 8, 4),
    'kernel3': (dict(kernel_width=3), 16, 8),
    'kernel7': (dict(kernel_width=7), 16, 8),
    'conv2_stride2': (dict(input_conv2_stride=2), 32, 16),
}


@pytest.mark.parametrize('variant', list(NETWORKS))
def test_whole_network(rec, variant):
    options, stride, head_stride = NETWORKS[variant]
    net = _net(7, **options)
    assert net.base_net.stride == stride and [m.stride for m in net.head_metas] == [head_stride, head_stride]
    trace, ok = _whole(rec, 'shufflenetv2k16 ' + variant, net)
    units = 16 + (2 if options.get('conv5_as_stage') else 0)
    assert trace.count('dwconv') == units + 3, trace             # one stencil per unit, two in each stage's first
    # 3 launches per first unit, 2 per other, conv5 as one convolution, the two heads (1392 input channels: the unit mode)
    assert trace.count('unit') == 3 * 3 + 2 * (units - 3) + (0 if options.get('conv5_as_stage') else 1) + 2, trace
    assert not [t for t in trace if t.startswith('miopen:base_net.stage') or t.startswith('miopen:base_net.conv5')], trace
    assert ('miopen:base_net.input_block.3.0' in trace) == ('input_conv2_stride' in options)      # the stem stays with torch
    assert ok


@pytest.mark.parametrize('on_device', [False, True], ids=['host-preprocess', 'device-preprocess'])
def test_predictor_smoke(on_device):
    from openpifpaf_amd.predictor import Predictor
    rng = np.random.default_rng(3)
    frames = [rng.integers(0, 256, (48, 64, 3), dtype=np.uint8), rng.integers(0, 256, (64, 40, 3), dtype=np.uint8)]
    saved = Predictor.long_edge, Predictor.batch_size, Predictor.device_preprocess
    Predictor.long_edge, Predictor.batch_size, Predictor.device_preprocess = 65, 2, on_device
    network.ShuffleNetV2K.stage4_dilation = 2
    shapes = []
    try:
        pred = Predictor('shufflenetv2k16')
        base = pred.model_cpu.base_net
        assert base.stage4_dilation == 2 and base.stride == 8 and base.stage4[0].branch2[3].dilation == (2, 2)
        assert [m.stride for m in pred.model_cpu.head_metas] == [4, 4]
        hooks = [pred.model.base_net.register_forward_hook(lambda mod, args, out: shapes.append(('base', tuple(args[0].shape[2:]), tuple(out.shape[2:]))))]
        hooks += [h.register_forward_hook(lambda mod, args, out: shapes.append(('head', tuple(args[0].shape[2:]), tuple(out.shape[3:]))))
                  for h in pred.model.head_nets]
        out = [p for p, _, _ in pred.numpy_images(frames)]
        for h in hooks:
            h.remove()
    finally:
        Predictor.long_edge, Predictor.batch_size, Predictor.device_preprocess = saved
        network.ShuffleNetV2K.stage4_dilation = 1
    assert len(out) == 2 and all(isinstance(p, list) for p in out)
    # the fields have the shapes of stride 4: features of stride 8 ((n - 1) // 8 + 1), upsampled by 2 less the cropped last row
    assert {kind for kind, _, _ in shapes} == {'base', 'head'}
    for kind, (ih, iw), (oh, ow) in shapes:
        if kind == 'base':
            assert (oh, ow) == ((ih - 1) // 8 + 1, (iw - 1) // 8 + 1), (ih, iw, oh, ow)
        else:
            assert (oh, ow) == (2 * ih - 1, 2 * iw - 1), (ih, iw, oh, ow)
