"""MobileNetV2 (``network.MobileNetV2``) and ShuffleNetV2 x1 / x2 (``network.ShuffleNetV2``) without a GPU: the architectures restated
with torchvision's module trees (reference ``network/basenetworks.py:407-430`` and ``:36-69``), parameter counts, key names and shapes
of the state dicts (no checkpoint can be loaded offline), conv + BN folding in float64, the LeakyReLU unit's switch and the command
line."""
import argparse
import copy

import pytest
import torch
from torch import nn

from openpifpaf_amd import fused, network
from openpifpaf_amd.predictor import Predictor

import trunk_common as tc

# name -> (class, stride, out_features, parameters of the base network, output rows x columns on 65 x 97)
# the parameter counts: torchvision's totals 3 504 872 / 2 278 604 / 7 393 996 minus their classifiers 1 281 000 / 1 025 000 / 2 049 000
NETS = {'mobilenetv2': (network.MobileNetV2, 32, 1280, 2223872, (3, 4)),
        'shufflenetv2x1': (network.ShuffleNetV2, 16, 1024, 1253604, (5, 7)),
        'shufflenetv2x2': (network.ShuffleNetV2, 16, 2048, 5344996, (5, 7))}
OWN_KEYS = ('weight', 'bias', 'running_mean', 'running_var', 'num_batches_tracked')


@pytest.mark.parametrize('name', list(NETS))
def test_structure_and_output_shape(name):
    cls, stride, out_features, n_params, hw = NETS[name]
    assert 3504872 - 1281000 == NETS['mobilenetv2'][3] and 2278604 - 1025000 == NETS['shufflenetv2x1'][3]
    assert 7393996 - 2049000 == NETS['shufflenetv2x2'][3]
    base = network.factory(name).base_net
    assert type(base) is cls and base.name == name and base.stride == stride and base.out_features == out_features
    assert sum(p.numel() for p in base.parameters()) == n_params
    with torch.no_grad():
        y = base(torch.randn(1, 3, 65, 97))
    assert tuple(y.shape) == (1, out_features) + hw
    assert (-(-65 // stride), -(-97 // stride)) == hw


def test_mobilenetv2_layers():
    base = network.factory('mobilenetv2').base_net
    backbone = base.backbone
    assert len(backbone) == 19 and all(isinstance(m, network._MBV2Block) for m in list(backbone)[1:18])
    stem, last = backbone[0], backbone[18]
    assert stem[0].stride == (2, 2) and stem[0].kernel_size == (3, 3) and stem[0].padding == (1, 1) and stem[0].bias is None
    assert (stem[0].in_channels, stem[0].out_channels, last[0].in_channels, last[0].out_channels) == (3, 32, 320, 1280)
    assert isinstance(stem[2], nn.ReLU6) and isinstance(last[2], nn.ReLU6) and last[0].kernel_size == (1, 1)
    # (t, c, n, s) of the paper's table, block by block: output channels, depthwise stride, whether there is an expanding convolution
    want = [(16, 1, False)] + [(24, 2, True), (24, 1, True)] + [(32, 2, True)] + [(32, 1, True)] * 2 + [(64, 2, True)] + [(64, 1, True)] * 3 \
        + [(96, 1, True)] * 3 + [(160, 2, True)] + [(160, 1, True)] * 2 + [(320, 1, True)]
    assert [(m.project.out_channels, m.depthwise.stride[0], m.expand is not None) for m in list(backbone)[1:18]] == want
    assert [i for i, m in enumerate(backbone) if isinstance(m, network._MBV2Block) and m.use_res_connect] == [3, 5, 6, 8, 9, 10, 12, 13, 15, 16]
    for m in list(backbone)[1:18]:
        assert len(m.conv) == (4 if m.expand is not None else 3) and isinstance(m.conv[-2], nn.Conv2d) and isinstance(m.conv[-1], nn.BatchNorm2d)
        assert m.depthwise.groups == m.depthwise.in_channels == m.project.in_channels and m.depthwise.kernel_size == (3, 3)
        assert m.expand is None or m.expand.out_channels == 6 * m.expand.in_channels
        assert sum(isinstance(a, nn.ReLU6) for a in m.modules()) == (2 if m.expand is not None else 1)
    bns = [m for m in base.modules() if isinstance(m, nn.BatchNorm2d)]
    assert len(bns) == 52 and all(m.eps == 1e-3 and m.momentum == 0.01 for m in bns)         # (as ``_conv_bn_act`` sets MobileNetV3's)
    assert all(m.bias is None for m in base.modules() if isinstance(m, nn.Conv2d))


@pytest.mark.parametrize('name', ['shufflenetv2x1', 'shufflenetv2x2'])
def test_shufflenetv2_layers(name):
    base = network.factory(name).base_net
    widths = {'shufflenetv2x1': (24, 116, 232, 464), 'shufflenetv2x2': (24, 244, 488, 976)}[name]
    assert isinstance(base.conv1[0], nn.Conv2d) and isinstance(base.conv1[1], nn.BatchNorm2d) and isinstance(base.conv1[2], nn.ReLU)
    assert (base.conv1[0].out_channels, base.conv1[0].kernel_size, base.conv1[0].stride, base.conv1[0].padding) == (24, (3, 3), (2, 2), (1, 1))
    assert [len(s) for s in (base.stage2, base.stage3, base.stage4)] == [4, 8, 4]
    inp = widths[0]
    for stage, width in zip((base.stage2, base.stage3, base.stage4), widths[1:]):
        for i, unit in enumerate(stage):
            assert isinstance(unit, network._InvertedResidualK) and not unit.leaky_relu and (unit.branch1 is not None) == (i == 0)
            dw = unit.branch2[3]
            assert dw.kernel_size == (3, 3) and dw.padding == (1, 1) and dw.dilation == (1, 1) and dw.stride == ((2, 2) if i == 0 else (1, 1))
            assert dw.groups == width // 2 and unit.branch2[0].in_channels == (inp if i == 0 else width // 2)
            assert unit.branch2[5].out_channels == width // 2 and isinstance(unit.branch2[7], nn.ReLU)
            if i == 0:
                assert unit.branch1[0].groups == inp and unit.branch1[0].kernel_size == (3, 3) and unit.branch1[2].out_channels == width // 2
        inp = width
    assert (base.conv5[0].in_channels, base.conv5[0].out_channels, base.conv5[0].kernel_size) == (widths[3], base.out_features, (1, 1))
    assert isinstance(base.conv5[2], nn.ReLU) and not hasattr(base, 'maxpool')


def test_state_dict_keys_and_shapes():
    """torchvision's names below ``base_net``: what a reference checkpoint holds (names and shapes only), written out by hand."""
    want = {
        'mobilenetv2': {
            'backbone.0.0.weight': (32, 3, 3, 3), 'backbone.0.1.weight': (32,), 'backbone.0.1.running_mean': (32,),
            'backbone.1.conv.0.0.weight': (32, 1, 3, 3), 'backbone.1.conv.0.1.bias': (32,), 'backbone.1.conv.1.weight': (16, 32, 1, 1),
            'backbone.1.conv.2.running_var': (16,), 'backbone.2.conv.0.0.weight': (96, 16, 1, 1), 'backbone.2.conv.0.1.weight': (96,),
            'backbone.2.conv.1.0.weight': (96, 1, 3, 3), 'backbone.2.conv.1.1.running_mean': (96,), 'backbone.2.conv.2.weight': (24, 96, 1, 1),
            'backbone.2.conv.3.weight': (24,), 'backbone.2.conv.3.num_batches_tracked': (), 'backbone.3.conv.0.0.weight': (144, 24, 1, 1),
            'backbone.7.conv.2.weight': (64, 192, 1, 1), 'backbone.11.conv.1.0.weight': (384, 1, 3, 3), 'backbone.14.conv.2.weight': (160, 576, 1, 1),
            'backbone.17.conv.0.0.weight': (960, 160, 1, 1), 'backbone.17.conv.2.weight': (320, 960, 1, 1), 'backbone.17.conv.3.bias': (320,),
            'backbone.18.0.weight': (1280, 320, 1, 1), 'backbone.18.1.weight': (1280,), 'backbone.18.1.running_var': (1280,)},
        'shufflenetv2x1': {
            'conv1.0.weight': (24, 3, 3, 3), 'conv1.1.running_mean': (24,), 'stage2.0.branch1.0.weight': (24, 1, 3, 3),
            'stage2.0.branch1.1.weight': (24,), 'stage2.0.branch1.2.weight': (58, 24, 1, 1), 'stage2.0.branch1.3.bias': (58,),
            'stage2.0.branch2.0.weight': (58, 24, 1, 1), 'stage2.0.branch2.1.running_var': (58,), 'stage2.0.branch2.3.weight': (58, 1, 3, 3),
            'stage2.0.branch2.4.weight': (58,), 'stage2.0.branch2.5.weight': (58, 58, 1, 1), 'stage2.0.branch2.6.num_batches_tracked': (),
            'stage2.3.branch2.0.weight': (58, 58, 1, 1), 'stage3.0.branch1.0.weight': (116, 1, 3, 3), 'stage3.0.branch2.0.weight': (116, 116, 1, 1),
            'stage3.7.branch2.5.weight': (116, 116, 1, 1), 'stage4.0.branch1.2.weight': (232, 232, 1, 1), 'stage4.3.branch2.3.weight': (232, 1, 3, 3),
            'conv5.0.weight': (1024, 464, 1, 1), 'conv5.1.weight': (1024,), 'conv5.1.bias': (1024,)},
        'shufflenetv2x2': {
            'conv1.0.weight': (24, 3, 3, 3), 'stage2.0.branch1.2.weight': (122, 24, 1, 1), 'stage2.0.branch2.0.weight': (122, 24, 1, 1),
            'stage2.1.branch2.3.weight': (122, 1, 3, 3), 'stage3.0.branch1.0.weight': (244, 1, 3, 3), 'stage3.7.branch2.5.weight': (244, 244, 1, 1),
            'stage4.0.branch2.0.weight': (488, 488, 1, 1), 'stage4.3.branch2.5.weight': (488, 488, 1, 1), 'conv5.0.weight': (2048, 976, 1, 1),
            'conv5.1.bias': (2048,)}}
    counts = {'mobilenetv2': 52 + 52 * 5, 'shufflenetv2x1': 56 + 56 * 5, 'shufflenetv2x2': 56 + 56 * 5}      # convolutions + 5 per batch norm
    for name, keys in want.items():
        sd = network.factory(name).state_dict()
        for key, shape in keys.items():
            assert tuple(sd['base_net.' + key].shape) == shape, (name, key)
        base_keys = [k for k in sd if k.startswith('base_net.')]
        assert len(base_keys) == counts[name], (name, len(base_keys))
        # nothing but torchvision's parameters and buffers: no key of our own in an unoptimized network
        assert all(k.split('.')[-1] in OWN_KEYS for k in base_keys)
        # a unit that is not first in its stage has no branch1 (torchvision: an empty Sequential, no keys either)
        assert not any('.branch1.' in k and not k.split('.')[2] == '0' for k in base_keys if k.startswith('base_net.stage'))


@pytest.mark.parametrize('name', list(NETS))
def test_optimized_state_dict(name):
    """After ``optimize_for_inference_``: no derived operand (``_opa*``) among the keys, and a strict load of another optimised
    network's state dict."""
    opt = network.optimize_for_inference_(tc.randomize_(network.factory(name), 1))
    other = network.optimize_for_inference_(tc.randomize_(network.factory(name), 2))
    x = torch.randn((1, 3, 33, 33), generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        before = opt(x)                                            # (a forward first: whatever it caches must stay out of the keys)
        assert not any('_opa' in k for k in opt.state_dict())
        result = opt.load_state_dict(other.state_dict(), strict=True)
        assert not result.missing_keys and not result.unexpected_keys
        after, want = opt(x), other(x)
    for b, a, w in zip(before, after, want):
        assert torch.equal(a, w) and not torch.equal(a, b)


@pytest.mark.parametrize('name', list(NETS))
def test_folding_on_the_cpu_in_float64(name, monkeypatch):
    """The optimised network equals the unoptimised one to 1e-10 of the output's size in float64, with random batch-norm statistics,
    whatever the switches say (on the CPU every route declines)."""
    net = tc.randomize_(network.factory(name), 3).double()
    x = torch.randn((2, 3, 33, 33), generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    with torch.no_grad():
        ref = net(x)
        for on in (True, False):
            monkeypatch.setattr(fused, 'MBV2', on)
            monkeypatch.setattr(fused, 'UNIT_LEAKY', on)
            opt = network.optimize_for_inference_(copy.deepcopy(net))
            assert not any(isinstance(m, nn.BatchNorm2d) for m in opt.modules())
            assert all(m.fused for m in opt.modules()
                       if isinstance(m, (network._MBV2Block, network.MobileNetV2, network._InvertedResidualK, network.ShuffleNetV2)))
            for r, g in zip(ref, opt(x)):
                assert float((r - g).abs().max()) <= 1e-10 * float(r.abs().max())
    assert all(float(r.abs().max()) > 0 and r.isfinite().all() for r in ref)


def test_leaky_units_fold_in_float64(monkeypatch):
    net = tc.randomize_(network.Shell(network.ShuffleNetV2K('shufflenetv2k16', leaky_relu=True, config=([2, 2, 2], [24, 32, 64, 128, 128])), []), 5)
    net = net.double()
    x = torch.randn((2, 3, 33, 33), generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    with torch.no_grad():
        ref = net.base_net(x)
        for on in (True, False):
            monkeypatch.setattr(fused, 'UNIT_LEAKY', on)
            got = network.optimize_for_inference_(copy.deepcopy(net)).base_net(x)
            assert float((ref - got).abs().max()) <= 1e-10 * float(ref.abs().max())
    assert bool((ref < 0).any())


def test_routes_decline_on_the_cpu_and_when_switched_off(monkeypatch):
    block = network.optimize_for_inference_(tc.randomize_(network._MBV2Block(32, 32, 1, 6), 0))
    x = torch.randn(1, 32, 5, 5).contiguous(memory_format=torch.channels_last)
    monkeypatch.setattr(fused, 'MBV2', True)
    assert block.fused and block.use_res_connect and not block._route_supported(x)
    assert block.expand is block.conv[0][0] and block.depthwise is block.conv[1][0] and block.project is block.conv[2]
    bare = network._MBV2Block(32, 16, 1, 1)
    assert bare.expand is None and bare.depthwise is bare.conv[0][0] and bare.project is bare.conv[1] and not bare.use_res_connect
    with pytest.raises(AssertionError):
        bare.enable_fused_()                                          # batch norms not folded
    # a LeakyReLU unit asks the switch before anything else
    unit = network.optimize_for_inference_(tc.randomize_(network._InvertedResidualK(32, 32, False, leaky_relu=True), 0))
    seen = []
    monkeypatch.setattr(fused, 'unit_conv_supported', lambda *a, **k: seen.append(1) or False)
    monkeypatch.setattr(fused, 'UNIT_LEAKY', False)
    assert not unit._unit_route_supported(x) and not seen
    monkeypatch.setattr(fused, 'UNIT_LEAKY', True)
    monkeypatch.setattr(network._InvertedResidualK, '_dw_ok', staticmethod(lambda m, t: True))
    monkeypatch.setattr(fused, '_unit_conv_ok', lambda mode, conv: True)
    assert not unit._unit_route_supported(x) and seen                # (past the switch: the operands decide)


def test_cli_offers_the_names_and_no_new_flags():
    parser = argparse.ArgumentParser()
    Predictor.cli(parser)
    for name in NETS:
        assert parser.parse_args(['--basenet', name]).basenet == name
    assert set(NETS) <= set(network.BASE_FACTORIES)
    flags = [s for a in parser._actions for s in a.option_strings]
    assert not any('mobilenetv2' in s or 'shufflenetv2-' in s or 'shufflenetv2x' in s for s in flags), flags
