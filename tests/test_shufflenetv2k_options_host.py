"""The reference's ShuffleNetV2K options (``network.ShuffleNetV2K``; reference ``network/basenetworks.py:186-400``) without a GPU:
strides, features, module structure and state-dict keys of every variant, the defaults against the network as it was before the
options, every variant against the reference's own class in float64 (``tests/golden/shufflenetv2k_options.npz``, written by
``tests/golden/make_golden_shufflenetv2k_options.py``) before and after conv + BN folding, a float64 model of the tap formula the
dilated stencil is written against, the command line, and the argument checks of ``opa_dwconv_dilated_act``."""
import argparse
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from openpifpaf_amd import fused, network
from openpifpaf_amd.predictor import Predictor

# options -> (overall stride, output H x W on [1, 3, 65, 49])
VARIANTS = {
    'default': ({}, 16, (5, 4)),
    'dilation2': (dict(stage4_dilation=2), 8, (9, 7)),
    'dilation4': (dict(stage4_dilation=4), 8, (9, 7)),
    'conv2_stride2': (dict(input_conv2_stride=2), 32, (3, 2)),
    'conv2_stride1': (dict(input_conv2_stride=1), 32, (3, 2)),              # the quirk: the convolution's stride is 2 all the same
    'kernel3': (dict(kernel_width=3), 16, (5, 4)),
    'kernel7': (dict(kernel_width=7), 16, (5, 4)),
    'conv5_stage': (dict(conv5_as_stage=True), 16, (5, 4)),
    'conv5_stage_dilation2': (dict(conv5_as_stage=True, stage4_dilation=2), 8, (9, 7)),
}
GOLDEN_VARIANTS = dict({k: v[0] for k, v in VARIANTS.items()}, leaky_relu=dict(leaky_relu=True),
                       conv2_out6=dict(input_conv2_stride=2, input_conv2_outchannels=6))
DEFAULTS = dict(input_conv2_stride=0, input_conv2_outchannels=None, stage4_dilation=1, kernel_width=5, conv5_as_stage=False,
                leaky_relu=False)
BN_KEYS = ('weight', 'bias', 'running_mean', 'running_var', 'num_batches_tracked')
NAMES = {'shufflenetv2k16': ([4, 8, 4], [24, 348, 696, 1392, 1392]), 'shufflenetv2k30': ([8, 16, 6], [32, 512, 1024, 2048, 2048])}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'shufflenetv2k_options.npz')
TINY = ([2, 2, 2], [4, 8, 16, 32, 32])


def _unit_keys(prefix, first):
    """The state-dict keys of one unit, written out from the architecture: branch1 = [dw, bn, 1x1, bn, act] in a first unit, branch2 =
    [1x1, bn, act, dw, bn, 1x1, bn, act]."""
    keys = []
    if first:
        for i in (0, 2):
            keys += ['%sbranch1.%d.weight' % (prefix, i)] + ['%sbranch1.%d.%s' % (prefix, i + 1, k) for k in BN_KEYS]
    for i in (0, 3, 5):
        keys += ['%sbranch2.%d.weight' % (prefix, i)] + ['%sbranch2.%d.%s' % (prefix, i + 1, k) for k in BN_KEYS]
    return keys


def _parent_keys(repeats):
    """The state-dict keys of ``ShuffleNetV2K(name)`` before the options existed, written out from the architecture."""
    keys = ['input_block.0.weight'] + ['input_block.1.' + k for k in BN_KEYS]
    for stage, rep in zip((2, 3, 4), repeats):
        for i in range(rep):
            keys += _unit_keys('stage%d.%d.' % (stage, i), i == 0)
    return keys + ['conv5.0.weight'] + ['conv5.1.' + k for k in BN_KEYS]


@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('name', list(NAMES))
def test_structure(name, variant):
    options, stride, hw = VARIANTS[variant]
    repeats, ch = NAMES[name]
    base = network.ShuffleNetV2K(name, **options).eval()
    assert base.stride == stride and base.out_features == ch[-1]
    with torch.no_grad():
        y = base(torch.randn(1, 3, 65, 49))
    assert tuple(y.shape) == (1, ch[-1]) + hw
    keys, plain = list(base.state_dict()), _parent_keys(repeats)
    k, d = options.get('kernel_width', 5), options.get('stage4_dilation', 1)
    stem = base.input_block[0]
    assert (stem.kernel_size, stem.stride, stem.padding, stem.out_channels) == ((3, 3), (2, 2), (1, 1), ch[0])
    if 'input_conv2_stride' in options:
        conv2 = base.input_block[3]
        assert len(base.input_block) == 4 and [type(m) for m in conv2] == [nn.Conv2d, nn.BatchNorm2d, nn.ReLU]
        assert (conv2[0].in_channels, conv2[0].out_channels, conv2[0].kernel_size, conv2[0].stride, conv2[0].padding, conv2[0].bias) == \
            (ch[0], ch[0], (3, 3), (2, 2), (1, 1), None)
        assert keys[:6] == plain[:6] and keys[6:12] == ['input_block.3.0.weight'] + ['input_block.3.1.' + kk for kk in BN_KEYS]
        assert keys[12:] == plain[6:]
    elif options.get('conv5_as_stage'):
        assert len(base.conv5) == 2 and all(isinstance(u, network._InvertedResidualK) and u.branch1 is None for u in base.conv5)
        assert keys == plain[:-6] + _unit_keys('conv5.0.', False) + _unit_keys('conv5.1.', False)
    else:
        assert keys == plain and len(base.input_block) == 3     # a dilation and a kernel width add and rename nothing
    # every depthwise convolution: stride, padding, dilation
    for stage_name, rep in zip(('stage2', 'stage3', 'stage4', 'conv5'), list(repeats) + [2]):
        stage = getattr(base, stage_name)
        if stage_name == 'conv5' and not options.get('conv5_as_stage'):
            assert [type(m) for m in stage] == [nn.Conv2d, nn.BatchNorm2d, nn.ReLU]
            continue
        dil = d if stage_name in ('stage4', 'conv5') else 1
        assert len(stage) == rep
        for i, unit in enumerate(stage):
            first = i == 0 and stage_name != 'conv5'
            assert (unit.branch1 is not None) == first
            dws = [m for m in unit.modules() if isinstance(m, nn.Conv2d) and m.groups > 1]
            assert len(dws) == (2 if first else 1)
            for m in dws:
                s = 2 if first and dil == 1 else 1
                assert (m.kernel_size, m.stride, m.dilation, m.padding) == ((k, k), (s, s), (dil, dil), ((k - 1) // 2 * dil,) * 2)
                assert m.groups == m.in_channels == m.out_channels
            for m in unit.modules():
                if isinstance(m, nn.Conv2d) and m.groups == 1:
                    assert (m.kernel_size, m.stride, m.dilation, m.padding) == ((1, 1), (1, 1), (1, 1), (0, 0))


def test_second_input_convolution_width_and_x5():
    base = network.ShuffleNetV2K('shufflenetv2k16', input_conv2_stride=2, input_conv2_outchannels=40)
    assert base.input_block[3][0].out_channels == 40 and base.stage2[0].branch1[0].in_channels == 40 and base.stride == 32
    x5 = network.ShuffleNetV2K('shufflenetv2kx5')
    assert x5.out_features == 2560 and [len(s) for s in (x5.stage2, x5.stage3, x5.stage4)] == [6, 13, 6]
    assert x5.input_block[0].out_channels == 42 and x5.stage2[0].branch2[5].out_channels == 320
    assert network.factory('shufflenetv2kx5').base_net.out_features == 2560
    # a first-in-stage conv5 if and only if the widths differ
    odd = network.ShuffleNetV2K('odd', conv5_as_stage=True, config=([2, 2, 2], [4, 8, 16, 32, 64]))
    assert odd.conv5[0].branch1 is not None and odd.conv5[1].branch1 is None and odd.out_features == 64
    assert odd.conv5[0].branch1[0].stride == (1, 1)
    with torch.no_grad():
        assert tuple(odd.eval()(torch.randn(1, 3, 33, 33)).shape) == (1, 64, 3, 3)


def test_leaky_relu_is_everywhere_a_relu_was():
    plain, leaky = network.ShuffleNetV2K('shufflenetv2k16'), network.ShuffleNetV2K('shufflenetv2k16', leaky_relu=True, conv5_as_stage=False)
    a, b = list(plain.modules()), list(leaky.modules())
    assert len(a) == len(b) and any(isinstance(m, nn.ReLU) for m in a)
    for m, n in zip(a, b):
        if isinstance(m, nn.ReLU):
            assert isinstance(n, nn.LeakyReLU) and n.negative_slope == 0.01 and n.inplace
        else:
            assert type(m) is type(n)
    assert list(plain.state_dict()) == list(leaky.state_dict())


def test_defaults_are_the_network_as_it_was():
    assert {k: getattr(network.ShuffleNetV2K, k) for k in DEFAULTS} == DEFAULTS
    for name, (repeats, ch) in NAMES.items():
        assert list(network.ShuffleNetV2K(name).state_dict()) == _parent_keys(repeats)
    torch.manual_seed(11)
    a = network.ShuffleNetV2K('shufflenetv2k16').eval()
    torch.manual_seed(11)
    spelled = dict(DEFAULTS)                                      # (None: "the class attribute", itself None)
    b = network.ShuffleNetV2K('shufflenetv2k16', **spelled).eval()
    assert list(a.state_dict()) == _parent_keys([4, 8, 4]) == list(b.state_dict())
    assert [type(m) for m in a.input_block] == [nn.Conv2d, nn.BatchNorm2d, nn.ReLU] and a.stride == 16 and a.out_features == 1392
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka
    x = torch.randn((1, 3, 33, 33), generator=torch.Generator().manual_seed(12))
    with torch.no_grad():
        assert torch.equal(a(x), b(x))
    # the factory's seeded network too: the same weights whether or not the keywords are spelled out
    net = network.factory('shufflenetv2k16', seed=3).base_net
    torch.manual_seed(3)
    again = network.ShuffleNetV2K('shufflenetv2k16', **spelled)
    assert torch.equal(net.conv5[0].weight, again.conv5[0].weight) and torch.equal(net.stage4[3].branch2[3].weight, again.stage4[3].branch2[3].weight)
    # ... and the seeded first weights are those of the architecture written out by hand, module by module in the old order
    torch.manual_seed(3)
    stem = nn.Conv2d(3, 24, 3, 2, 1, bias=False)
    assert torch.equal(net.input_block[0].weight, stem.weight)


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def _golden_net(golden, variant):
    net = network.ShuffleNetV2K('tiny', config=TINY, **dict(DEFAULTS, **GOLDEN_VARIANTS[variant])).double().eval()
    keys, sizes, flat = [str(k) for k in golden[variant + '/keys']], golden[variant + '/sizes'], golden[variant + '/w']
    state = net.state_dict()
    assert keys == [k for k in state if not k.endswith('num_batches_tracked')], 'the key names differ from the reference\'s'
    assert int(sizes.sum()) == len(flat)
    at = 0
    for key, size in zip(keys, sizes):
        assert state[key].numel() == size, key
        state[key] = torch.from_numpy(flat[at:at + size].astype(np.float64)).reshape(state[key].shape)
        at += int(size)
    net.load_state_dict(state, strict=True)
    return net


@pytest.mark.parametrize('variant', list(GOLDEN_VARIANTS))
def test_against_the_reference_class(golden, variant):
    """The in-tree float64 network with the reference's weights against the reference's float64 output: ``max |delta| <= 1e-9 max
    |ref|`` (six orders of magnitude above double rounding; any structural mistake moves the output by order one), and the same
    after ``optimize_for_inference_`` on the CPU (folding only)."""
    assert golden['x'].dtype == np.float32 and all(golden[k].dtype.kind in 'fiU' for k in golden.files)
    net = _golden_net(golden, variant)
    x = torch.from_numpy(golden['x']).double()
    ref = torch.from_numpy(golden[variant + '/out'])
    assert ref.dtype == torch.float64
    with torch.no_grad():
        got = net(x)
        opt = network.optimize_for_inference_(copy.deepcopy(net))
        assert not any(isinstance(m, nn.BatchNorm2d) for m in opt.modules()) and opt.fused and opt.stage4[0].fused
        folded = opt(x)
    scale = float(ref.abs().max())
    assert got.shape == ref.shape and scale > 1
    for what, t in (('unfused', got), ('folded', folded)):
        delta = float((t - ref).abs().max())
        print('SHUFFLEOPT golden %s %s max |delta| %.3e of max |ref| %.3e' % (variant, what, delta, scale))
        assert delta <= 1e-9 * scale, (what, delta, scale)


def test_the_golden_variants_differ_from_the_default(golden):
    """No variant's reference output is the default's with the variant's weights: the options change what is computed.  (A golden
    that every network passes would show nothing.)"""
    for variant, options in GOLDEN_VARIANTS.items():
        if variant == 'default' or 'kernel_width' in options or 'conv5_as_stage' in options or 'input_conv2_stride' in options:
            continue                                    # (other weights' shapes: the default network cannot even load them)
        net = _golden_net(golden, variant)
        plain = network.ShuffleNetV2K('tiny', config=TINY, **DEFAULTS).double().eval()
        plain.load_state_dict(net.state_dict())
        with torch.no_grad():
            out = plain(torch.from_numpy(golden['x']).double())
        ref = torch.from_numpy(golden[variant + '/out'])
        assert out.shape != ref.shape or float((out - ref).abs().max()) > 1e-3 * float(ref.abs().max()), variant


def _tap_model(x, w_taps, K, D):
    """The stencil's formula, stride 1: tap (ky, kx) of output (y, x) reads input (y - P D + ky D, x - P D + kx D), P = K / 2, zeros
    outside; ``w_taps`` ``[K * K, C]`` as ``fused.depthwise_taps`` orders it."""
    B, C, H, W = x.shape
    P = K // 2
    out = torch.zeros_like(x)
    for ky in range(K):
        for kx in range(K):
            for y in range(H):
                yy = y - P * D + ky * D
                if not 0 <= yy < H:
                    continue
                for xo in range(W):
                    xx = xo - P * D + kx * D
                    if 0 <= xx < W:
                        out[:, :, y, xo] += x[:, :, yy, xx] * w_taps[ky * K + kx]
    return out


@pytest.mark.parametrize('hw', [(6, 7), (2, 2), (3, 5), (1, 1)])
@pytest.mark.parametrize('D', [1, 2, 4])
@pytest.mark.parametrize('K', [3, 5, 7])
def test_tap_formula_is_the_dilated_depthwise_convolution(K, D, hw):
    g = torch.Generator().manual_seed(10 * K + D)
    C = 3
    weight = torch.randn((C, 1, K, K), generator=g, dtype=torch.float64)
    x = torch.randn((2, C) + hw, generator=g, dtype=torch.float64)
    want = F.conv2d(x, weight, None, stride=1, padding=K // 2 * D, dilation=D, groups=C)
    taps = fused.depthwise_taps(weight)
    assert tuple(taps.shape) == (K * K, C)
    got = _tap_model(x, taps, K, D)
    assert got.shape == want.shape == x.shape and float((got - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1e-30)
    assert fused.dwconv_out_hw(hw[0], hw[1], K, 1, D) == hw
    for s in (1, 2):                                    # the undilated sizes are torch's
        assert fused.dwconv_out_hw(hw[0], hw[1], K, s) == tuple(F.conv2d(x, weight, None, s, K // 2, 1, C).shape[2:])


def test_folding_and_cpu_declines():
    net = network.ShuffleNetV2K('tiny', config=TINY, stage4_dilation=2, kernel_width=7)
    opt = network.optimize_for_inference_(net.eval())
    dw = opt.stage4[0].branch2[3]
    assert tuple(dw.w_taps.shape) == (49, 16) and dw.dilation == (2, 2)
    h = torch.randn(1, 16, 5, 5).contiguous(memory_format=torch.channels_last)
    assert not fused.dwconv_supported(h, 7, 1, 2) and not fused.dwconv_supported(h, 5, 1)          # the CPU declines
    assert not network._InvertedResidualK._dw_ok(dw, h)
    leaky = network.optimize_for_inference_(network.ShuffleNetV2K('tiny', config=TINY, leaky_relu=True).eval())
    x = torch.randn(1, 16, 5, 5)
    assert opt.stage3[1]._unit_route_supported(x) in (True, False)         # (decided by the library's presence)
    assert leaky.stage3[1]._unit_route_supported(x) is False and leaky.stage3[0]._unit_route_supported(torch.randn(1, 8, 5, 5)) is False


def test_cli_sets_the_class_attributes():
    parser = argparse.ArgumentParser()
    Predictor.cli(parser)
    flags = {k: 'shufflenetv2k_' + ('kernel' if k == 'kernel_width' else k) for k in DEFAULTS}
    saved = {k: getattr(network.ShuffleNetV2K, k) for k in DEFAULTS}
    try:
        args = parser.parse_args([])
        assert {k: getattr(args, flags[k]) for k in DEFAULTS} == DEFAULTS
        args = parser.parse_args(['--shufflenetv2k-stage4-dilation', '2', '--shufflenetv2k-kernel', '3', '--shufflenetv2k-conv5-as-stage'])
        Predictor.configure(args)
        assert {k: getattr(network.ShuffleNetV2K, k) for k in DEFAULTS} == dict(DEFAULTS, stage4_dilation=2, kernel_width=3, conv5_as_stage=True)
        base = network.factory('shufflenetv2k16').base_net
        assert base.stride == 8 and base.stage4[1].branch2[3].dilation == (2, 2) and base.stage4[1].branch2[3].kernel_size == (3, 3)
        assert isinstance(base.conv5[0], network._InvertedResidualK)
        args = parser.parse_args(['--shufflenetv2k-input-conv2-stride', '2', '--shufflenetv2k-input-conv2-outchannels', '32',
                                  '--shufflenetv2k-leaky-relu'])
        Predictor.configure(args)
        assert {k: getattr(network.ShuffleNetV2K, k) for k in DEFAULTS} == dict(DEFAULTS, input_conv2_stride=2, input_conv2_outchannels=32,
                                                                              leaky_relu=True)
        base = network.factory('shufflenetv2k16').base_net
        assert base.stride == 32 and base.input_block[3][0].out_channels == 32 and isinstance(base.conv5[2], nn.LeakyReLU)
        # a ResNet flag next to them, as before
        Predictor.configure(parser.parse_args(['--resnet-block5-dilation', '2']))
        assert network.Resnet.block5_dilation == 2
        Predictor.configure(parser.parse_args([]))
        assert {k: getattr(network.ShuffleNetV2K, k) for k in DEFAULTS} == DEFAULTS and network.Resnet.block5_dilation == 1
        assert not [a.dest for a in parser._actions if 'instance_norm' in a.dest or 'group_norm' in a.dest]
    finally:
        for k, v in saved.items():
            setattr(network.ShuffleNetV2K, k, v)
        network.Resnet.block5_dilation = 1


def test_entry_point_checks_its_arguments():
    """Bad arguments are refused on the host, before anything is launched (so this needs no GPU): never dereferenced pointers."""
    from openpifpaf_amd import _lib
    lib, fake = _lib.lib(), 4096
    INVALID = 1
    name = b'opa_dwconv_dilated_act: '

    def call(x=fake, xs=8, w=fake, bias=fake, out=fake, os_=8, batch=2, h=9, wd=7, c=8, k=5, stride=1, dilation=2, dtype=0, act=1):
        return lib.opa_dwconv_dilated_act(x, xs, w, bias, out, os_, batch, h, wd, c, k, stride, dilation, dtype, act, None)
    bad_arguments = ([dict(k=k) for k in (1, 2, 4, 6, 9)] + [dict(dilation=d) for d in (0, -1, 3, 8)] +
                     [dict(stride=2, dilation=2), dict(stride=2, dilation=4), dict(stride=3, dilation=1), dict(stride=0, dilation=1),
                      dict(dtype=1), dict(dtype=3), dict(x=None), dict(w=None), dict(out=None), dict(xs=7), dict(os_=7),
                      dict(batch=0), dict(h=0), dict(wd=0), dict(c=0)])
    for bad in bad_arguments:
        assert call(**bad) == INVALID, bad
        assert lib.opa_last_error() == name + b'bad arguments', (bad, lib.opa_last_error())
    for act in (-1, 3):
        assert call(act=act) == INVALID
        assert lib.opa_last_error() == name + b'act must be 0 (none), 1 (ReLU) or 2 (hardswish)'
    assert call(act=3, k=4) == INVALID and b'act must be' in lib.opa_last_error()        # the neighbours' order: the act first
    # batch * output rows: a dilated call keeps its rows, a strided one halves them
    for kw in (dict(batch=1, h=65536), dict(batch=2, h=32768, k=7, dilation=4), dict(batch=65536, h=1, k=3),
               dict(batch=1, h=131071, stride=2, dilation=1), dict(batch=1, h=65536, k=7, dilation=1)):
        assert call(**kw) == INVALID, kw
        assert lib.opa_last_error() == name + b'batch * output rows must not exceed 65535', kw
    # the neighbours keep their accepted set and their texts
    for symbol in ('opa_dwconv_act', 'opa_dwconv_bias_act'):
        assert getattr(lib, symbol)(fake, 8, fake, None, fake, 8, 2, 9, 7, 8, 7, 1, 0, 1, None) == INVALID
        assert lib.opa_last_error() == symbol.encode() + b': bad arguments'
