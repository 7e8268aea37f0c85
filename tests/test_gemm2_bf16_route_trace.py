"""Which launches of ``opa_gemm2_bias_act_bf16`` a ResNet cast to bfloat16 makes with ``fused.PAIR_BF16`` on, with every argument (an
address as null / ptr, every scalar as its value), and that no downsampling ``nn.Conv2d`` is called any more -- traced on the CPU with
the technique of ``test_resnet_route_trace.py`` (a recorder in place of ``fused._launch``, tensors that say they are on the GPU, the
library reported as built, a forward hook on every ``nn.Conv2d`` that records ``miopen:<module name>``).  No GPU is touched and nothing
is timed.  What is expected is written here: resnet18, resnet50, resnet50 with ``block5_dilation=2`` and resnext50 at input
``[1, 3, 33, 25]`` -- the stem leaves 17 x 13 pixels, the stages 17 x 13, 9 x 7, 5 x 4 and 3 x 2 (block 5 dilated: 5 x 4)."""
import copy

import pytest
import torch
from torch import nn

from openpifpaf_amd import _lib, fused, network, winograd

import trunk_common as tc

CL = torch.channels_last
SYMBOL = 'opa_gemm2_bias_act_bf16'
NETWORKS = {'resnet18': ('resnet18', {}), 'resnet50': ('resnet50', {}), 'resnet50-dilated': ('resnet50', {'block5_dilation': 2}),
            'resnext50': ('resnext50', {})}
# (h_in, w_in) of the input of the first block of each stage
HW = ((17, 13), (17, 13), (9, 7), (5, 4))


def _launch(k1, k2, hw, stride, a_bias, n, bias=True, relu=1):
    """a1, k1, a2, k2, batch, h_in, w_in, stride, a_bias, wcat, bias, out, n, relu"""
    return '%s(%s, %d, ptr, %d, 1, %d, %d, %d, %s, ptr, %s, ptr, %d, %d)' % (
        SYMBOL, 'ptr' if k1 else 'null', k1, k2, hw[0], hw[1], stride, 'ptr' if a_bias else 'null', 'ptr' if bias else 'null', n, relu)


def expected(net_name, conv3_bf16):
    """The launches of the symbol in forward order.  ``a_bias`` (conv2's owed bias + ReLU) is handed over where conv2 went to MIOpen:
    with ``CONV3_BF16`` off, and in a ResNeXt, whose grouped 3x3 has no bf16 kernel."""
    if net_name == 'resnet18':                     # BasicBlocks: the strided 1x1 alone, stages 2 - 4; no first source, bias or ReLU
        return [_launch(0, 64, HW[1], 2, False, 128, bias=False, relu=0), _launch(0, 128, HW[2], 2, False, 256, bias=False, relu=0),
                _launch(0, 256, HW[3], 2, False, 512, bias=False, relu=0)]
    widths = (128, 256, 512, 1024) if net_name == 'resnext50' else (64, 128, 256, 512)      # conv3's input channels
    inputs = (64, 256, 512, 1024)                                                          # the block's
    strides = (1, 2, 2, 1 if net_name == 'resnet50-dilated' else 2)
    a_bias = net_name == 'resnext50' or not conv3_bf16
    return [_launch(widths[i], inputs[i], HW[i], strides[i], a_bias, 256 << i) for i in range(4)]


class _OnDevice(torch.Tensor):
    is_cuda = True


@pytest.fixture
def traced(monkeypatch):
    """-> (trace, {network name: the optimized bfloat16 network with a hook on every convolution}, the input)"""
    trace = []
    monkeypatch.setattr(fused, '_launch', lambda symbol, *args: trace.append('%s(%s)' % (symbol, ', '.join(map(str, args)))))
    monkeypatch.setattr(fused, '_ptr', lambda t: 'null' if t is None else 'ptr')
    empty = fused._empty_nhwc
    monkeypatch.setattr(fused, '_empty_nhwc', lambda *a, **kw: empty(*a, **kw).zero_().as_subclass(_OnDevice))
    monkeypatch.setattr(_lib, 'available', lambda: True)

    class Stream:
        cuda_stream = 0x7F00DEAD0040
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda *a: Stream())
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: False)
    for name, value in (('X3_TERMS', 6), ('_CHOICE', {}), ('FORCE_PICK', 'conv'), ('GCONV', False), ('STEM7_BF16', False)):
        monkeypatch.setattr(fused, name, value)
    monkeypatch.setattr(winograd, '_mode', winograd.get_mode())
    nets = {}
    for net_name, (config, options) in NETWORKS.items():
        torch.manual_seed(5)
        net = network.optimize_for_inference_(copy.deepcopy(tc.randomize_(network.Resnet(config, **options), 5))).to(torch.bfloat16)
        for name, m in net.named_modules():
            if isinstance(m, nn.Conv2d):
                m.register_forward_hook(lambda mod, args, out, name=name: trace.append('miopen:' + name))
        nets[net_name] = net
    x = torch.randn((1, 3, 33, 25), generator=tc.gen(7)).to(torch.bfloat16).contiguous(memory_format=CL).as_subclass(_OnDevice)
    return trace, nets, x


def _forward(trace, net, x):
    del trace[:]
    with torch.no_grad():
        net(x)
    return list(trace)


@pytest.mark.parametrize('conv3_bf16', [False, True])
@pytest.mark.parametrize('net_name', sorted(NETWORKS))
def test_the_downsampling_convolutions_go_to_the_kernel_with_these_arguments(traced, monkeypatch, net_name, conv3_bf16):
    trace, nets, x = traced
    monkeypatch.setattr(fused, 'CONV3_BF16', conv3_bf16)
    monkeypatch.setattr(fused, 'PAIR_BF16', True)
    on = _forward(trace, nets[net_name], x)
    got = [launch for launch in on if launch.startswith(SYMBOL + '(')]
    assert got == expected(net_name, conv3_bf16), (got, expected(net_name, conv3_bf16))
    assert len(got) == (3 if net_name == 'resnet18' else 4)
    assert not [launch for launch in on if launch.startswith('miopen:') and launch.endswith('downsample.0')], on
    if net_name == 'resnet50-dilated':
        assert got[-1].split(', ')[7] == '1' and got[-2].split(', ')[7] == '2'              # block 5: stride 1
    if net_name == 'resnext50':
        assert all(launch.split(', ')[8] == 'ptr' for launch in got)                       # a_bias, whatever CONV3_BF16 says
    # the switch off: the symbol never appears, every downsampling convolution is MIOpen's, and nothing else differs from the trace above
    monkeypatch.setattr(fused, 'PAIR_BF16', False)
    off = _forward(trace, nets[net_name], x)
    assert not [launch for launch in off if launch.startswith(SYMBOL)]
    assert len([launch for launch in off if launch.startswith('miopen:') and launch.endswith('downsample.0')]) == len(got)
    if net_name == 'resnet18':                     # the identity is computed where it was: one launch for one MIOpen call, in place
        assert [launch if not launch.endswith('downsample.0') else SYMBOL for launch in off] == \
               [launch if not launch.startswith(SYMBOL) else SYMBOL for launch in on]
    else:                                          # a Bottleneck: MIOpen's downsampling and conv3 (+ its epilogue pass) became the one launch
        assert len(off) > len(on)
        assert len([launch for launch in on if launch.endswith('.0.conv3')]) == 0 < len([launch for launch in off if launch.endswith('.0.conv3')])


def test_a_float32_network_runs_the_calls_it_ran(traced, monkeypatch):
    """float32 with the switch on: the trace is the trace with the switch off."""
    trace, nets, x = traced
    net = nets['resnet50'].to(torch.float32)
    x32 = x.float().contiguous(memory_format=CL).as_subclass(_OnDevice)
    monkeypatch.setattr(fused, 'PAIR_BF16', False)
    off = _forward(trace, net, x32)
    monkeypatch.setattr(fused, 'PAIR_BF16', True)
    assert _forward(trace, net, x32) == off and not [launch for launch in off if launch.startswith(SYMBOL)]
