"""The ResNet options on the GPU: the dilated 3x3 convolution of the split-operand implicit GEMM (``opa_conv3x3_dilated_f32x3``), the
input max-pool kernel (``csrc/pool.hip``, ``opa_maxpool3x3_bias_act``), the block routes built on the former
(``network._Bottleneck`` / ``_BasicBlock`` with a dilated 3x3), whole networks with ``block5_dilation=2`` and ``pool0_stride=2``
and a ``Predictor`` on each.

The error criterion is the one of ``test_gpu_gconv.py`` / ``test_gpu_trunk_routes.py``: ``ref64`` the same op or unfused module in
``double()``; ``e0`` the error against ``ref64`` of torch's OWN float32 (bfloat16 where the case is one) op or module, the median of
nine calls, never of the code under test; ``err = max |got - ref64| / max |ref64|`` and the same as an rms; required
``err <= K * e0``, K the smallest of 2, 4, 8 that holds for every case and seed of a family, as in ``test_gpu_trunk_routes.py``.
Every case prints a ``RESNETV`` line (``pytest -s``); the lines of a run are kept in ``profiles/resnet_variants/route_errors.log``.
Worst err/e0 of that log (max, rms) and the K it gives, per family (``K``):
  kernel    the dilated kernel alone, 220 cases                    1.69, 0.94  -> 2
  block     the dilated blocks on the kernel's route, 3 seeds each 1.86, 1.07  -> 2
  declined  blocks whose dilated 3x3 the kernel declines           2.16, 1.64  -> 4  (the case above 2 is the NCHW one, which runs
            torch's convolutions and the epilogue pass and no kernel of this file)
  network   whole networks, every pick on its split-operand side   2.31, 2.23  -> 4  (above 2: resnet50 with block5_dilation=2, 2.22;
            with pool0_stride=2, 2.06; with input_conv2_stride=2, 2.31.  ``profiles/resnet_variants/default_resnet50_errors.log`` holds
            the same recipe on the DEFAULT resnet50, which runs neither kernel of this file: 1.89 - 2.35 over three seeds, and the
            dilated net with block 5 on torch's convolution: 1.73 - 2.06 against 1.80 - 2.14 on the kernel)
The pool kernel is compared with ``torch.equal``: it has no rounding of its own.

Kernel cases and what they reach (``test_dilated_kernel[d-s-terms]``): c_out 64 -> the 64-wide tile, 128 -> the 128-wide one;
c_in 128 -> two K-steps more per tap; images (1, 1) and (2, 5): smaller than the dilation, off-centre taps outside (all of them at
(1, 1)); (9, 7): M = 126, one partial tile; (8, 23): M = 368, three tiles with a tail, one of which spans both images."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from openpifpaf_amd import _lib, fused, headmeta, network

import trunk_common as tc

pytestmark = pytest.mark.gpu

SEEDS = (0, 1, 2)
K = {'kernel': 2, 'block': 2, 'declined': 4, 'network': 4}
CL = torch.channels_last
SHAPES = [(1, 1), (2, 5), (9, 7), (8, 23)]
_LAUNCHERS = {'conv3x3_dilated_bias_act_x3': 'conv3x3_d', 'maxpool3x3_bias_act_': 'pool', 'gconv3x3_bias_act': 'gconv',
              'conv1x1_bias_act': 'gemm', 'conv1x1_bias_act_x3': 'gemm3', 'conv1x1_pair_bias_act_x3': 'pair',
              'conv3x3_bias_act_x3': 'conv3x3_x3', 'stem7x7_bias_act_x3': 'stem_x3', 'bias_act_': 'bias_act', 'head_conv_x3': 'head_x3',
              'head_epilogue': 'head_epilogue'}


def _report(family, what, err, e0):
    return tc.report('RESNETV', '%s %s' % (family, what), err, e0, K[family], show_k=True)


@pytest.fixture
def rec(monkeypatch):
    """Launch recorder; nothing may be timed: ``FORCE_PICK = 'x3'``, and every float32 1x1 convolution of ``conv_bias_act`` is answered
    'gemm3' by a choice table that stays empty (``test_gpu_gconv.py``'s recipe and its reason)."""
    monkeypatch.setenv('OPA_CONV1X1', 'gemm')                 # (bfloat16: decided without timing too)
    return tc.recorder(monkeypatch, _LAUNCHERS, ('X3_PAIR', 'X3_CONV3', 'X3_STEM', 'X3_HEAD', 'GCONV'), force_pick='x3',
                       table=tc.PinnedGemm3())


# ---- 1. the dilated kernel -----------------------------------------------------------------------------------------------------

def _conv(c_in, c_out, stride, d, seed):
    return tc.randomize_(nn.Conv2d(c_in, c_out, 3, stride, d, d, bias=False), seed).cuda().requires_grad_(False)


def _poisoned(H, W, C, seed):
    """-> (x, big): ``x`` is images 1-2 of the four-image channels-last ``big`` whose images 0 and 3 are NaN."""
    big = torch.full((4, H, W, C), float('nan'), device='cuda')
    big[1:3] = torch.randn((2, H, W, C), generator=tc.gen(seed)).cuda()
    return big[1:3].permute(0, 3, 1, 2), big


@pytest.mark.parametrize('terms', [6, 9])
@pytest.mark.parametrize('d,s', [(2, 1), (3, 1), (2, 2), (1, 1), (1, 2)])
def test_dilated_kernel(monkeypatch, d, s, terms):
    monkeypatch.setattr(fused, 'X3_TERMS', terms)
    monkeypatch.setattr(fused, 'X3_CONV3', True)
    combos = [(True, True), (False, False), (True, False), (False, True)]
    ok = True
    for c_in, c_out in ((64, 64), (64, 128), (128, 64)):
        conv = _conv(c_in, c_out, s, d, 100 * d + 10 * s + c_in // 64 + c_out // 64)
        bias = (torch.randn(c_out, generator=tc.gen(c_in + c_out)) * 0.5).cuda()
        zero = torch.zeros_like(bias)
        for i, (H, W) in enumerate(SHAPES if c_in == 64 else [(9, 7)]):
            x, big = _poisoned(H, W, c_in, H * W + c_in)
            assert x.is_contiguous(memory_format=CL) and fused.conv3x3_dilated_x3_supported(conv, x, bias)
            assert H * W == 1 or not fused.conv3x3_dilated_x3_supported(conv, x.contiguous(), bias)
            assert not fused.conv3x3_dilated_x3_supported(conv, x.bfloat16(), bias)
            lin64 = F.conv2d(x.double(), conv.weight.double(), None, s, d, d)
            for with_bias, relu in (combos if (H, W) == (9, 7) and c_in == 64 else [combos[i % 4], combos[(i + 1) % 4]]):
                b = bias if with_bias else zero

                def post(t, b=b, relu=relu):
                    t = t + b.to(t.dtype).view(1, -1, 1, 1)
                    return F.relu(t) if relu else t
                ref64 = post(lin64)
                e0 = tc.e0(lambda: post(conv(x)), ref64)
                big0 = big.clone()
                got = fused.conv3x3_dilated_bias_act_x3(conv, x, b, relu=relu)
                assert got.isfinite().all(), 'a tap left its image'
                assert torch.equal(big.isnan(), big0.isnan()) and torch.equal(big[1:3], big0[1:3]), 'the input changed'
                assert got.is_contiguous(memory_format=CL) and got.shape == ref64.shape
                assert torch.equal(got, fused.conv3x3_dilated_bias_act_x3(conv, x, b, relu=relu)), 'two calls differ'
                if d == 1:                      # the undilated entry point is the d = 1 call of the same code
                    assert fused.conv3x3_x3_supported(conv, x, b)
                    assert torch.equal(got, fused.conv3x3_bias_act_x3(conv, x, b, relu=relu))
                ok &= _report('kernel', 'd %d s %d terms %d c %d->%d %dx%d bias %d relu %d' % (d, s, terms, c_in, c_out, H, W, with_bias, relu),
                              tc.errors(got, ref64), e0)
    assert ok


@pytest.mark.parametrize('s', [1, 2])
def test_nan_and_inf_go_where_the_window_says(monkeypatch, s):
    monkeypatch.setattr(fused, 'X3_TERMS', 6)
    monkeypatch.setattr(fused, 'X3_CONV3', True)
    d, C = 2, 64
    conv = _conv(C, 64, s, d, 17 + s)
    zero = torch.zeros(64, device='cuda')
    H, W = 9, 11
    x = torch.randn((2, C, H, W), generator=tc.gen(3)).cuda().contiguous(memory_format=CL)
    clean = fused.conv3x3_dilated_bias_act_x3(conv, x, zero, relu=False)
    for value, (b, c, y, xx) in ((float('nan'), (1, 5, 4, 6)), (float('inf'), (0, 0, 0, 10))):
        xp = x.clone(memory_format=torch.preserve_format)
        xp[b, c, y, xx] = value
        got = fused.conv3x3_dilated_bias_act_x3(conv, xp, zero, relu=False)
        hit = torch.zeros_like(clean, dtype=torch.bool)
        ys = [yo for yo in range(clean.shape[2]) if y - yo * s in (-d, 0, d)]
        xs = [xo for xo in range(clean.shape[3]) if xx - xo * s in (-d, 0, d)]
        for yo in ys:
            for xo in xs:
                hit[b, :, yo, xo] = True
        assert hit.any() and bool((~got[hit].isfinite()).all()), 'the value is missing from an output that reads it'
        assert torch.equal(got[~hit], clean[~hit]), 'the value reached an output that does not read it'


# ---- 2. the pool kernel ----------------------------------------------------------------------------------------------------------

def _same_with_nans(a, b):
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(nan=0.0), b.nan_to_num(nan=0.0))


@pytest.mark.parametrize('C', [8, 64])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['float32', 'bfloat16'])
def test_pool_kernel(dtype, C):
    for H, W in SHAPES:
        x = (torch.randn((2, C, H, W), generator=tc.gen(H * W + C)) * 3).to(dtype).cuda().contiguous(memory_format=CL)
        bias = torch.randn(C, generator=tc.gen(C)).to(dtype).cuda()
        assert fused.maxpool3x3_supported(x) and fused.maxpool3x3_supported(x, bias)
        assert not fused.maxpool3x3_supported(x.contiguous()) or H * W == 1 or C == 1
        assert not fused.maxpool3x3_supported(x, bias.float() if dtype == torch.bfloat16 else bias.bfloat16())
        x0 = x.clone()
        for with_epilogue in (False, True):
            if with_epilogue:
                want = F.max_pool2d(F.relu(x + bias.view(1, -1, 1, 1)), 3, 2, 1)
                got = fused.maxpool3x3_bias_act_(x, bias, relu=True)
            else:
                want = F.max_pool2d(x, 3, 2, 1)
                got = fused.maxpool3x3_bias_act_(x)
            assert got.dtype == dtype and got.shape == want.shape and got.is_contiguous(memory_format=CL)
            assert torch.equal(got, want), 'max |delta| %.3g' % (got.float() - want.float()).abs().max().item()
            assert torch.equal(x, x0), 'the input changed'
        # bias without ReLU, ReLU without bias
        assert torch.equal(fused.maxpool3x3_bias_act_(x, bias), F.max_pool2d(x + bias.view(1, -1, 1, 1), 3, 2, 1))
        assert torch.equal(fused.maxpool3x3_bias_act_(x, None, relu=True), F.max_pool2d(F.relu(x), 3, 2, 1))
        # a NaN appears in exactly the outputs whose window holds it, as in torch
        b, c, y, xx = 1, C - 3, H // 2, W - 1
        xp = x.clone(memory_format=torch.preserve_format)
        xp[b, c, y, xx] = float('nan')
        for args in ((None, False), (bias, True)):
            got = fused.maxpool3x3_bias_act_(xp, *args)
            hit = torch.zeros_like(got, dtype=torch.bool)
            for yo in range(got.shape[2]):
                for xo in range(got.shape[3]):
                    if abs(y - 2 * yo) <= 1 and abs(xx - 2 * xo) <= 1:
                        hit[b, c, yo, xo] = True
            assert hit.any() and torch.equal(got.isnan(), hit)
            t = xp if args[0] is None else F.relu(xp + bias.view(1, -1, 1, 1))
            assert _same_with_nans(got, F.max_pool2d(t, 3, 2, 1))
            assert torch.equal(got[~hit], fused.maxpool3x3_bias_act_(x, *args)[~hit])


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['float32', 'bfloat16'])
def test_pool_writes_stay_inside_its_output(dtype):
    C = 64
    for H, W in ((9, 7), (8, 23)):
        ho, wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        x = torch.randn((2, C, H, W), generator=tc.gen(H)).to(dtype).cuda().contiguous(memory_format=CL)
        wide = torch.full((4, ho, wo, C), 7.0, dtype=dtype, device='cuda')
        out = wide[1:3].permute(0, 3, 1, 2)                    # the two images in the middle
        fused.maxpool3x3_bias_act_(x, out=out)
        torch.cuda.synchronize()
        assert bool((wide[0] == 7.0).all()) and bool((wide[3] == 7.0).all()), 'a write outside the output'
        assert torch.equal(out, F.max_pool2d(x, 3, 2, 1))


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['float32', 'bfloat16'])
def test_pool_without_epilogue_keeps_the_sign_of_a_zero(dtype):
    """Windows of +0.0 and -0.0 alone: the first of equal values in torch's scan order stays, so the BITS are torch's."""
    x = torch.zeros((2, 8, 9, 7), dtype=dtype)
    x[torch.rand(x.shape, generator=tc.gen(21)) < 0.5] = -0.0
    x[0, :, :4] = -0.0                                            # whole windows of -0.0 too
    x = x.cuda().contiguous(memory_format=CL)
    got, want = fused.maxpool3x3_bias_act_(x), F.max_pool2d(x, 3, 2, 1)
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(got.contiguous().view(bits), want.contiguous().view(bits))
    assert bool(torch.signbit(got).any()) and not bool(torch.signbit(got).all())


def test_pool_entry_point_refuses_other_strides():
    x = torch.zeros((1, 8, 4, 4), device='cuda').contiguous(memory_format=CL)
    out = torch.full((1, 8, 4, 4), 7.0, device='cuda').contiguous(memory_format=CL)
    vp = ctypes.c_void_p
    for stride in (1, 3):
        assert _lib.lib().opa_maxpool3x3_bias_act(vp(x.data_ptr()), None, vp(out.data_ptr()), 0, 1, 4, 4, 8, stride, 0, None) == 1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---- 3. block routes -------------------------------------------------------------------------------------------------------------

def _bottleneck(seed, groups=1, base_width=64):
    ds = nn.Sequential(nn.Conv2d(256, 512, 1, 2, bias=False), nn.BatchNorm2d(512))
    block = network._Bottleneck(256, 128, 2, ds, groups, base_width)          # as _make_layer builds it, then dilated like block 5
    return tc.randomize_(network._dilate_(block, 2), seed)


def _basic(seed):
    return tc.randomize_(network._dilate_(network._BasicBlock(64, 64), 2), seed)


BLOCKS = {'bottleneck': (_bottleneck, (2, 256, 13, 11), ['gemm3', 'conv3x3_d', 'pair']),
          'basic': (_basic, (2, 64, 13, 11), ['conv3x3_d', 'conv3x3_d', 'bias_act'])}


@functools.lru_cache(maxsize=None)
def _reference(make, shape, seed, dtype=torch.float32):
    """-> (the unfused module on the CPU, x, ref64, e0)."""
    module = make(seed)
    x = torch.randn(shape, generator=tc.gen(1000 + seed)).abs().cuda().to(dtype).contiguous(memory_format=CL)
    with torch.no_grad():
        ref64 = copy.deepcopy(module).double().cuda()(x.double())
        plain = copy.deepcopy(module).cuda().to(dtype).to(memory_format=CL)
        e0 = tc.e0(lambda: plain(x), ref64)
    assert e0[0] > 0 and ref64.isfinite().all()
    return module, x, ref64, e0


@pytest.mark.parametrize('block', list(BLOCKS))
def test_block_route(rec, block):
    make, shape, route = BLOCKS[block]
    ok = True
    for seed in SEEDS:
        module, x, ref64, e0 = _reference(make, shape, seed)
        convs = [m for m in module.modules() if isinstance(m, nn.Conv2d)]
        assert all(m.stride == (1, 1) for m in convs) and sum(m.dilation == (2, 2) for m in convs) == (1 if block == 'bottleneck' else 2)
        opt = rec.watch(tc.optimized(module).cuda().to(memory_format=CL))
        got, trace = tc.forward_checks(opt, x, rec)
        assert trace == route, trace
        assert not [t for t in trace if t.startswith('miopen:')], trace
        assert fused.choices() == {}, 'the route made a choice-table entry'
        assert got.is_contiguous(memory_format=CL) and got.shape == ref64.shape == x.shape[:1] + (ref64.shape[1],) + x.shape[2:]
        ok &= _report('block', '%s | %s | seed %d' % (block, ' '.join(trace), seed), tc.errors(got, ref64), e0)
        fused.FORCE_PICK = 'conv'                           # the other side of every pick: torch's convolution + the epilogue pass
        off, trace = tc.forward_checks(opt, x, rec)
        assert 'conv3x3_d' not in trace and 'miopen:conv2' in trace, trace
        assert float((off - got).abs().max()) <= 1e-4 * float(off.abs().max())
        _report('block', '%s | %s | seed %d' % (block, ' '.join(trace), seed), tc.errors(off, ref64), e0)       # (printed, not judged here)
        fused.FORCE_PICK = 'x3'
    assert ok


def test_block_route_declines(rec):
    """bfloat16, a tensor that is not channels-last and a grouped dilated convolution take torch's convolution and stay correct."""
    ok = True
    make, shape, _ = BLOCKS['bottleneck']
    module, x, ref64, e0 = _reference(make, shape, 0)
    opt = rec.watch(tc.optimized(module).cuda())                              # weights and input NCHW: so is every activation
    with torch.no_grad():
        assert not fused.conv3x3_dilated_x3_supported(opt.conv2, torch.randn((2, 128, 13, 11), device='cuda'), opt.fb2)
        rec.trace.clear()
        got = opt(x.contiguous())
    assert 'conv3x3_d' not in rec.trace and 'miopen:conv2' in rec.trace, rec.trace
    ok &= _report('declined', 'not channels-last | %s' % ' '.join(rec.trace), tc.errors(got, ref64), e0)

    module, x, ref64, e0 = _reference(make, shape, 0, torch.bfloat16)
    opt = rec.watch(tc.optimized(module).cuda().bfloat16().to(memory_format=CL))
    with torch.no_grad():
        rec.trace.clear()
        got = opt(x)
    assert got.dtype == torch.bfloat16 and 'conv3x3_d' not in rec.trace and 'miopen:conv2' in rec.trace, rec.trace
    ok &= _report('declined', 'bfloat16 | %s' % ' '.join(rec.trace), tc.errors(got, ref64), e0)

    grouped = functools.partial(_bottleneck, groups=32, base_width=4)          # ResNeXt's width: 32 groups of 8 channels
    module, x, ref64, e0 = _reference(grouped, shape, 0)
    assert module.conv2.groups == 32 and module.conv2.dilation == (2, 2)
    opt = rec.watch(tc.optimized(module).cuda().to(memory_format=CL))
    with torch.no_grad():
        h = torch.randn((2, 256, 13, 11), device='cuda').contiguous(memory_format=CL)
        assert not fused.gconv3x3_supported(opt.conv2, h, opt.fb2) and not fused.conv3x3_dilated_x3_supported(opt.conv2, h, opt.fb2)
        rec.trace.clear()
        got = opt(x)
    assert 'conv3x3_d' not in rec.trace and 'gconv' not in rec.trace and 'miopen:conv2' in rec.trace, rec.trace
    ok &= _report('declined', 'grouped | %s' % ' '.join(rec.trace), tc.errors(got, ref64), e0)
    assert ok


@pytest.mark.parametrize('block', list(BLOCKS))
def test_forward_after_load_state_dict(rec, block):
    make, shape, route = BLOCKS[block]
    _, x, _, _ = _reference(make, shape, 0)
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


# ---- 4. whole networks, predictor ----------------------------------------------------------------------------------------------------

def _net(name, seed, **options):
    base = network.Resnet(name, **options)
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
        again = opt(x)
    ok = True
    for i, (g, a, r) in enumerate(zip(got, again, ref64)):
        assert g.isfinite().all() and g.shape == r.shape
        if not any(t.startswith('miopen:') for t in trace):
            assert torch.equal(g, a)
        ok &= _report('network', '%s head %d' % (what, i), tc.errors(g, r), e0s[i])
    return trace, ok


def test_whole_network_dilated(rec):
    net = _net('resnet50', 7, block5_dilation=2)
    assert net.base_net.stride == 8 and [m.stride for m in net.head_metas] == [4, 4]
    trace, ok = _whole(rec, 'resnet50 block5_dilation=2', net)
    assert trace.count('conv3x3_d') == 3 and 'pool' not in trace, trace
    assert not [t for t in trace if t.startswith('miopen:') and t.endswith('conv2')], trace
    assert ok


def test_whole_network_with_the_input_pool(rec):
    net = _net('resnet50', 9, pool0_stride=2)
    assert net.base_net.stride == 32 and [m.stride for m in net.head_metas] == [16, 16]
    trace, ok = _whole(rec, 'resnet50 pool0_stride=2', net)
    assert trace.count('pool') == 1 and 'conv3x3_d' not in trace, trace
    assert trace[:2] == ['stem_x3', 'pool'], trace              # bias + ReLU inside the stem's GEMM: the pool alone
    assert ok


def test_the_pool_takes_the_epilogue_of_a_raw_stem(rec):
    """bfloat16 (torch's raw convolution in front): the kernel applies the stem's bias + ReLU, no epilogue pass before it; equal to
    the pass followed by torch's pool, bit for bit."""
    base = tc.randomize_(network.Resnet('resnet18', pool0_stride=2), 5)
    opt = network.optimize_for_inference_(copy.deepcopy(base)).cuda().bfloat16().to(memory_format=CL)
    x = torch.randn((2, 3, 65, 49), generator=tc.gen(6)).cuda().bfloat16().contiguous(memory_format=CL)
    raws = []
    opt.input_block[0].register_forward_hook(lambda mod, args, out: raws.append(out.clone()))      # (the kernel only reads it)
    with torch.no_grad():
        rec.trace.clear()
        got = opt._input_block_fused(x)
        assert rec.trace == ['pool'] and len(raws) == 1, rec.trace
        want = F.max_pool2d(F.relu(raws[0] + opt.fb0.view(1, -1, 1, 1)), 3, 2, 1)
    assert got.dtype == torch.bfloat16 and torch.equal(got, want)


def test_the_pool_takes_the_epilogue_of_a_float32_stem_that_ran_as_torchs_convolution(rec):
    """``pick('stempool')`` on its 'conv' side: the raw convolution, then ONE pass (bias + ReLU + pool), equal to torch's three ops."""
    base = tc.randomize_(network.Resnet('resnet18', pool0_stride=2), 5)
    opt = network.optimize_for_inference_(copy.deepcopy(base)).cuda().to(memory_format=CL)
    x = torch.randn((2, 3, 65, 49), generator=tc.gen(6)).cuda().contiguous(memory_format=CL)
    raws = []
    opt.input_block[0].register_forward_hook(lambda mod, args, out: raws.append(out.clone()))
    with torch.no_grad():
        fused.FORCE_PICK = 'conv'
        rec.trace.clear()
        got = opt._input_block_fused(x)
        assert rec.trace == ['pool'] and len(raws) == 1, rec.trace
        want = F.max_pool2d(F.relu(raws[0] + opt.fb0.view(1, -1, 1, 1)), 3, 2, 1)
        assert torch.equal(got, want)
        fused.FORCE_PICK = 'x3'
        rec.trace.clear()
        other = opt._input_block_fused(x)
        assert rec.trace == ['stem_x3', 'pool'], rec.trace
    assert float((other - got).abs().max()) <= 1e-4 * float(got.abs().max())


def test_whole_network_with_the_second_input_convolution(rec):
    """``input_conv2_stride=2``: the 64 -> 64 stride-2 3x3 behind the stem runs as the implicit GEMM with its folded bias (``fb0_2``)."""
    net = _net('resnet50', 13, input_conv2_stride=2)
    assert net.base_net.stride == 32
    trace, ok = _whole(rec, 'resnet50 input_conv2_stride=2', net)
    assert trace[:2] == ['stem_x3', 'conv3x3_x3'], trace
    assert not [t for t in trace if t.startswith('miopen:base_net.input_block')], trace
    assert ok


def test_whole_network_resnet18_dilated(rec):
    net = _net('resnet18', 11, block5_dilation=2)
    trace, ok = _whole(rec, 'resnet18 block5_dilation=2', net)
    assert trace.count('conv3x3_d') == 4, trace
    assert ok


@pytest.mark.parametrize('on_device', [False, True], ids=['host-preprocess', 'device-preprocess'])
@pytest.mark.parametrize('option,value,stride', [('block5_dilation', 2, 4), ('pool0_stride', 2, 16)])
def test_predictor_smoke(option, value, stride, on_device):
    from openpifpaf_amd.predictor import Predictor
    rng = np.random.default_rng(3)
    frames = [rng.integers(0, 256, (48, 64, 3), dtype=np.uint8), rng.integers(0, 256, (64, 40, 3), dtype=np.uint8)]
    saved = Predictor.long_edge, Predictor.batch_size, Predictor.device_preprocess
    saved_option = getattr(network.Resnet, option)
    Predictor.long_edge, Predictor.batch_size, Predictor.device_preprocess = 65, 2, on_device
    setattr(network.Resnet, option, value)
    try:
        pred = Predictor('resnet50')
        assert getattr(pred.model_cpu.base_net, option) == value
        assert [m.stride for m in pred.model_cpu.head_metas] == [stride, stride]
        out = [p for p, _, _ in pred.numpy_images(frames)]
    finally:
        Predictor.long_edge, Predictor.batch_size, Predictor.device_preprocess = saved
        setattr(network.Resnet, option, saved_option)
    assert len(out) == 2 and all(isinstance(p, list) for p in out)
