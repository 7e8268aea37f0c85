"""The grouped 3x3 convolution of the ResNeXt bottlenecks on the GPU (``csrc/gconv.hip``, ``opa_gconv3x3_bias_act_f32``), the block
route built on it (``network._Bottleneck`` with ``groups > 1``), the whole resnext50 and a ``Predictor`` on it.

The error criterion is the one of ``test_gpu_mobilenetv3.py``: ``ref64`` the unfused module or op in ``double()``; ``e0`` the error
against ``ref64`` of the SAME float32 torch module or op (the median of nine calls), not of the code under test;
``err = max |got - ref64| / max |ref64|`` and the same as an rms; required ``err <= 2 * e0``.  Every case prints a ``GCONV`` line
(``pytest -s``); the lines of a run are kept in ``profiles/resnext/route_errors.log``.

Template instantiations ``gconv3x3_kernel<CG, S, P>`` and who runs them (``test_kernel[cg-groups-stride]``):
  <4, 1, 8>  4-2-1, 4-3-1, 4-32-1      <4, 2, 4>  4-2-2, 4-3-2, 4-32-2
  <8, 1, 8>  8-2-1, 8-3-1              <8, 2, 4>  8-2-2, 8-3-2
  <16, 1, 8> 16-2-1, 16-3-1            <16, 2, 4> 16-2-2, 16-3-2
  <32, 1, 8> 32-2-1, 32-3-1            <32, 2, 4> 32-2-2, 32-3-2
  <64, 1, 8> 64-2-1, 64-3-1            <64, 2, 4> 64-2-2, 64-3-2
Host-side launch branches (``pick_tile``: 16 pixel slots as SX along x by 16 / SX along y; ``_tile`` below is its model):
  stride 1 (tile widths 8, 16, 32, 64):  SX 1: (9, 7), (32, 7)   SX 2: (1, 1), (2, 5), (8, 23)   SX 4: (4, 33)   SX 8: (2, 65)
  stride 2 (tile widths 4, 8, 16):       SX 1: (32, 7)           SX 2: (1, 1), (2, 5), (9, 7)    SX 4: (8, 23), (4, 33), (2, 65)
  (``test_shapes_reach_every_launch_branch``).  One W past the tile width: (4, 33) and (2, 65) at stride 1, (2, 65) -> Wo 33 at
  stride 2.  More than one tile: (8, 23) along x, (32, 7) along y.  Channel chunks of 64: one (C <= 64), a partial one (cg 16, 32
  with 3 groups: C = 48, 96), two and three full ones (cg 64).  SX 16 never fits the LDS budget and is never launched."""
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
SHAPES = [(1, 1), (2, 5), (9, 7), (8, 23)]
WIDE_SHAPES = [(4, 33), (2, 65), (32, 7)]              # the remaining launch branches (with 2 groups only)
_LAUNCHERS = {'gconv3x3_bias_act': 'gconv', 'conv1x1_bias_act': 'gemm', 'conv1x1_bias_act_x3': 'gemm3', 'conv1x1_pair_bias_act_x3': 'pair',
              'conv3x3_bias_act_x3': 'conv3x3_x3', 'stem7x7_bias_act_x3': 'stem_x3', 'bias_act_': 'bias_act', 'head_conv_x3': 'head_x3',
              'head_epilogue': 'head_epilogue'}


_report = functools.partial(tc.report, 'GCONV')


@pytest.fixture
def rec(monkeypatch):
    """Launch recorder; nothing may be timed: ``FORCE_PICK = 'x3'``, and every float32 1x1 convolution of ``conv_bias_act`` is answered
    'gemm3' (the split-operand GEMM, which the product's table picks at the trunk's sizes) by a choice table that stays empty;
    the grouped route switched on.  Not the float32 MFMA GEMM ('gemm'): it adds its K products in one float32 chain, and with the
    K = 2048 of block ``cg64`` that chain alone is 2.3 - 2.6 e0 of the block (measured on an MI355X: err max 9.1e-7 - 9.4e-7 against
    e0 3.6e-7 - 4.0e-7; a float32 replay of the block on the CPU with everything else in float64 puts 7.6e-7 on the two GEMMs and
    1.3e-7, the float64 baseline's level, on the grouped convolution) -- an error of a kernel this file does not test."""
    monkeypatch.setenv('OPA_CONV1X1', 'gemm')                 # (bfloat16, where no split-operand kernel exists: decided without timing too)
    return tc.recorder(monkeypatch, _LAUNCHERS, ('X3_PAIR', 'X3_CONV3', 'X3_STEM', 'X3_HEAD', 'GCONV'), force_pick='x3',
                       table=tc.PinnedGemm3())


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------------

def _tile(Ho, Wo, S):
    """Model of ``pick_tile`` (csrc/gconv.hip) -> log2(SX)."""
    P = 8 if S == 1 else 4
    best, best_cost = 0, -1
    for l in range(5):
        TH, TW = 16 >> l, (1 << l) * P
        IR, IC = (TH - 1) * S + 3, (TW - 1) * S + 3
        if IR * IC * 256 > 80 * 1024:
            continue
        cost = -(-Ho // TH) * -(-Wo // TW) * IR * IC
        if best_cost < 0 or cost <= best_cost:
            best, best_cost = l, cost
    return best


def test_shapes_reach_every_launch_branch():
    for S, want in ((1, {0, 1, 2, 3}), (2, {0, 1, 2})):
        assert {_tile((H - 1) // S + 1, (W - 1) // S + 1, S) for H, W in SHAPES + WIDE_SHAPES} == want


def _conv(cg, groups, stride, seed):
    C = cg * groups
    return tc.randomize_(nn.Conv2d(C, C, 3, stride, 1, groups=groups, bias=False), seed).cuda().requires_grad_(False)   # (inference)


def _raw(x, x_pitch, wt, bias, out, out_pitch, cg, stride, relu):
    """The C entry point on views: ``x`` / ``out`` channels innermost with ``x_pitch`` / ``out_pitch`` floats between pixels."""
    B, C, H, W = x.shape
    vp = ctypes.c_void_p
    rc = _lib.lib().opa_gconv3x3_bias_act_f32(vp(x.data_ptr()), x_pitch, vp(wt.data_ptr()),
                                              vp(bias.data_ptr()) if bias is not None else None, vp(out.data_ptr()),
                                              out_pitch, B, H, W, C, cg, stride, int(relu), None)
    assert rc == 0, _lib.lib().opa_last_error()
    return out


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('cg,groups', [(4, 2), (4, 3), (4, 32), (8, 2), (8, 3), (16, 2), (16, 3), (32, 2), (32, 3), (64, 2), (64, 3)])
def test_kernel(monkeypatch, cg, groups, stride):
    """Batch 2; x is a view of images 1-2 of a 4-image tensor whose images 0 and 3 and whose 4 extra channels per pixel are NaN
    (a read outside the window or the channels poisons the result); every shape with two of (bias, ReLU) on / off, (9, 7) with all
    four; input unchanged; first call == second call, bit for bit."""
    monkeypatch.setattr(fused, 'GCONV', True)
    C = cg * groups
    conv = _conv(cg, groups, stride, 1000 * cg + 10 * groups + stride)
    bias = (torch.randn(C, generator=tc.gen(cg + groups)) * 0.5).cuda()
    wt = fused.gconv_weight_of(conv)
    combos = [(True, True), (False, False), (True, False), (False, True)]
    ok = True
    for i, (H, W) in enumerate(SHAPES + (WIDE_SHAPES if groups == 2 else [])):
        big = torch.full((4, H, W, C + 4), float('nan'), device='cuda')
        big[1:3, :, :, :C] = torch.randn((2, H, W, C), generator=tc.gen(H * W + C)).cuda()
        xv = big[1:3, :, :, :C].permute(0, 3, 1, 2)                      # [2, C, H, W], pixel stride C + 4
        x = xv.contiguous(memory_format=CL)
        assert fused.gconv3x3_supported(conv, x, bias) and not fused.gconv3x3_supported(conv, xv, bias)
        lin64 = F.conv2d(x.double(), conv.weight.double(), None, stride, 1, groups=groups)
        for with_bias, relu in (combos if (H, W) == (9, 7) else [combos[i % 4], combos[(i + 1) % 4]]):
            b = bias if with_bias else None

            def post(t, b=b, relu=relu):
                t = t if b is None else t + b.to(t.dtype).view(1, -1, 1, 1)
                return F.relu(t) if relu else t
            ref64 = post(lin64)
            e0 = tc.e0(lambda: post(conv(x)), ref64)
            x0 = x.clone()
            got = fused.gconv3x3_bias_act(conv, x, b, relu=relu)
            assert torch.equal(x, x0) and got.is_contiguous(memory_format=CL) and got.shape == ref64.shape
            assert torch.equal(got, fused.gconv3x3_bias_act(conv, x, b, relu=relu)), 'two calls differ'
            # the same through the C entry point on the strided view, into a fresh output
            out = torch.empty_like(got)
            big0 = big.clone()
            _raw(xv, C + 4, wt, b, out, C, cg, stride, relu)
            assert torch.equal(out, got) and out.isfinite().all(), 'a read outside the window or the channels'
            assert torch.equal(big.isnan(), big0.isnan()) and torch.equal(big[1:3, :, :, :C], big0[1:3, :, :, :C])
            ok &= _report('kernel cg %d groups %d s %d %dx%d bias %d relu %d' % (cg, groups, stride, H, W, with_bias, relu),
                          tc.errors(got, ref64), e0)
    assert ok


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('cg,groups', [(4, 3), (16, 3), (64, 2)])
def test_writes_stay_inside_the_channel_slice(cg, groups, stride):
    C = cg * groups
    conv = _conv(cg, groups, stride, cg)
    wt = fused.gconv_weight_of(conv)
    for H, W in ((9, 7), (8, 23)):
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        x = torch.randn((2, C, H, W), generator=tc.gen(H)).cuda().contiguous(memory_format=CL)
        wide = torch.full((3, Ho + 1, Wo, C + 8), 7.0, device='cuda')            # a guard image behind, a guard row, guard channels
        out = wide[:2, :Ho, :, 4:4 + C].permute(0, 3, 1, 2)
        # (the guard row makes the image stride differ from Ho * Wo * pitch: one image per call)
        for b in range(2):
            _raw(x[b:b + 1], C, wt, None, out[b:b + 1], C + 8, cg, stride, False)
        torch.cuda.synchronize()
        want = F.conv2d(x, conv.weight, None, stride, 1, groups=groups)
        mask = torch.zeros_like(wide, dtype=torch.bool)
        mask[:2, :Ho, :, 4:4 + C] = True
        assert bool((wide[~mask] == 7.0).all()), 'a write outside the slice'
        assert float((out - want).abs().max()) <= 1e-4 * float(want.abs().max())


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('cg,groups', [(4, 3), (32, 2)])
def test_nan_and_inf_go_where_the_window_and_the_group_say(monkeypatch, cg, groups, stride):
    monkeypatch.setattr(fused, 'GCONV', True)
    C = cg * groups
    conv = _conv(cg, groups, stride, cg + 7)
    H, W = 9, 11
    x = torch.randn((2, C, H, W), generator=tc.gen(3)).cuda().contiguous(memory_format=CL)
    clean = fused.gconv3x3_bias_act(conv, x, None, relu=False)
    for value, (b, c, y, xx) in ((float('nan'), (1, cg + 1, 4, 6)), (float('inf'), (0, 0, 0, 10))):
        xp = x.clone(memory_format=torch.preserve_format)
        xp[b, c, y, xx] = value
        got = fused.gconv3x3_bias_act(conv, xp, None, relu=False)
        hit = torch.zeros_like(clean, dtype=torch.bool)
        g = c // cg
        ys = [yo for yo in range(clean.shape[2]) if -1 <= y - yo * stride <= 1]
        xs = [xo for xo in range(clean.shape[3]) if -1 <= xx - xo * stride <= 1]
        for yo in ys:
            for xo in xs:
                hit[b, g * cg:(g + 1) * cg, yo, xo] = True
        assert hit.any() and bool((~got[hit].isfinite()).all()), 'the value is missing from an output that reads it'
        assert torch.equal(got[~hit], clean[~hit]), 'the value reached an output that does not read it'


# ---- 2. block routes -----------------------------------------------------------------------------------------------------------

# inplanes, planes, stride, downsample, groups, base width, (H, W)
BLOCKS = {'first': (64, 64, 1, True, 32, 4, (13, 11)), 'strided': (256, 128, 2, True, 32, 4, (13, 11)),
          'cg64': (2048, 512, 1, False, 32, 8, (5, 4))}


def _make(spec, seed):
    inplanes, planes, stride, ds, groups, base_width, _ = spec
    down = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride, bias=False), nn.BatchNorm2d(planes * 4)) if ds else None
    return tc.randomize_(network._Bottleneck(inplanes, planes, stride, down, groups, base_width), seed)


@functools.lru_cache(maxsize=None)
def _reference(block, seed):
    """-> (the unfused block on the CPU, x, ref64, e0)."""
    spec = BLOCKS[block]
    module = _make(spec, seed)
    x = torch.randn((2, spec[0]) + spec[6], generator=tc.gen(1000 + seed)).abs().cuda().contiguous(memory_format=CL)
    with torch.no_grad():
        ref64 = copy.deepcopy(module).double().cuda()(x.double())
        plain = copy.deepcopy(module).cuda().to(memory_format=CL)
        e0 = tc.e0(lambda: plain(x), ref64)
    assert e0[0] > 0 and ref64.isfinite().all()
    return module, x, ref64, e0


@pytest.mark.parametrize('block', list(BLOCKS))
def test_block_route(rec, block):
    ok = True
    for seed in SEEDS:
        module, x, ref64, e0 = _reference(block, seed)
        opt = rec.watch(tc.optimized(module).cuda().to(memory_format=CL))
        got, trace = tc.forward_checks(opt, x, rec)
        assert trace.count('gconv') == 1 and 'miopen:conv2' not in trace, trace
        assert trace == (['gemm3', 'gconv', 'pair'] if BLOCKS[block][3] else ['gemm3', 'gconv', 'gemm3']), trace
        assert fused.choices() == {}, 'the route made a choice-table entry'
        assert got.is_contiguous(memory_format=CL) and got.shape == ref64.shape
        ok &= _report('block %s | %s | seed %d' % (block, ' '.join(trace), seed), tc.errors(got, ref64), e0)
        fused.GCONV = False                                 # switched off: conv2 is torch's again
        off, trace = tc.forward_checks(opt, x, rec)
        assert 'gconv' not in trace and trace.count('miopen:conv2') == 1, trace
        assert float((off - got).abs().max()) <= 1e-4 * float(off.abs().max())
        fused.GCONV = True
    assert ok


def test_block_route_declines(rec):
    """bfloat16, autocast and a tensor that is not channels-last take torch's convolution."""
    module, x, _, _ = _reference('first', 0)
    opt = rec.watch(tc.optimized(module).cuda().to(memory_format=CL))
    h = torch.randn((2, 128, 13, 11), device='cuda').contiguous(memory_format=CL)
    with torch.no_grad():
        assert fused.gconv3x3_supported(opt.conv2, h, opt.fb2)
        assert not fused.gconv3x3_supported(opt.conv2, h.contiguous(), opt.fb2)
        assert not fused.gconv3x3_supported(opt.conv2, h.bfloat16(), opt.fb2)
        assert not fused.gconv3x3_supported(opt.conv2, h[:, :64], opt.fb2)
    assert not fused.gconv3x3_supported(opt.conv2, h, opt.fb2)                      # the weight asks for a gradient
    assert not fused.gconv3x3_supported(opt.conv2.requires_grad_(False), h.clone().requires_grad_(), opt.fb2)
    opt.conv2.requires_grad_(True)
    with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
        assert not fused.gconv3x3_supported(opt.conv2, h, opt.fb2)
        rec.trace.clear()
        opt(x)
    assert 'gconv' not in rec.trace and 'miopen:conv2' in rec.trace, rec.trace
    with torch.no_grad():
        rec.trace.clear()
        tc.optimized(module).cuda().bfloat16().to(memory_format=CL)(x.bfloat16())
    assert 'gconv' not in rec.trace, rec.trace


def test_forward_after_load_state_dict(rec):
    _, x, _, _ = _reference('first', 0)
    module1, _, _, _ = _reference('first', 1)
    opt = tc.optimized(_make(BLOCKS['first'], 0)).cuda().to(memory_format=CL)
    other = tc.optimized(module1).cuda().to(memory_format=CL)
    with torch.no_grad():
        before = opt(x)
        opt.load_state_dict(other.state_dict(), strict=True)
        rec.trace.clear()
        after = opt(x)
        assert rec.trace == ['gemm3', 'gconv', 'pair'], rec.trace
        assert not torch.equal(before, after)
        assert torch.equal(after, other(x)), 'stale operand: max |delta| %.3g' % (after - other(x)).abs().max().item()


# ---- 3. whole network, predictor -------------------------------------------------------------------------------------------------

def test_whole_network(rec):
    """resnext50 with the cocokp heads on [2, 3, 65, 49]: the optimized channels-last model against the double model."""
    net = tc.randomize_(network.factory('resnext50'), 7)
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
    assert trace.count('gconv') == 16, trace
    assert not [t for t in trace if t.startswith('miopen:') and t.endswith('conv2')], trace
    ok = True
    for i, (g, a, r) in enumerate(zip(got, again, ref64)):
        assert g.isfinite().all()
        if not any(t.startswith('miopen:') for t in trace):
            assert torch.equal(g, a)
        ok &= _report('resnext50 head %d' % i, tc.errors(g, r), e0s[i])
    assert ok


@pytest.mark.parametrize('on_device', [False, True], ids=['host-preprocess', 'device-preprocess'])
def test_predictor_smoke(monkeypatch, on_device):
    from openpifpaf_amd.predictor import Predictor
    monkeypatch.setattr(fused, 'GCONV', True)
    rng = np.random.default_rng(3)
    frames = [rng.integers(0, 256, (48, 64, 3), dtype=np.uint8), rng.integers(0, 256, (64, 40, 3), dtype=np.uint8)]
    saved = Predictor.long_edge, Predictor.batch_size, Predictor.device_preprocess
    Predictor.long_edge, Predictor.batch_size, Predictor.device_preprocess = 65, 2, on_device
    try:
        pred = Predictor('resnext50')
        assert isinstance(pred.model_cpu.base_net, network.Resnet) and pred.model_cpu.base_net.name == 'resnext50'
        out = [p for p, _, _ in pred.numpy_images(frames)]
    finally:
        Predictor.long_edge, Predictor.batch_size, Predictor.device_preprocess = saved
    assert len(out) == 2 and all(isinstance(p, list) for p in out)
