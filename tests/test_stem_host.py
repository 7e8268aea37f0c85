"""The host side of the RGB stem route (``fused.stem_*``, ``network._stem_route``), without a GPU: the output size, the derived weight
operand and its cache, everything ``stem_conv3x3_supported`` declines, the switch's default, and the five families' optimized
networks on the CPU, where the route is never taken."""
import copy
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from openpifpaf_amd import fused, network

import trunk_common as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ['shufflenetv2k16', 'shufflenetv2x1', 'mobilenetv2', 'mobilenetv3small', 'squeezenet']


def _stem(channels=32, stride=2, bias=True, **kwargs):
    kwargs = dict(dict(kernel_size=3, stride=stride, padding=1, bias=bias), **kwargs)
    return tc.randomize_(nn.Conv2d(kwargs.pop('in_channels', 3), channels, **kwargs), channels)


def test_out_hw_is_the_convolutions():
    for s in (1, 2):
        for h in range(1, 10):
            for w in range(1, 10):
                want = F.conv2d(torch.zeros(1, 3, h, w), torch.zeros(1, 3, 3, 3), stride=s, padding=1).shape[2:]
                assert fused.stem_conv_out_hw(h, w, s) == tuple(want), (h, w, s)


@pytest.mark.parametrize('channels', fused.STEM_CHANNELS)
def test_weight_operand_is_tap_major(channels):
    conv = _stem(channels)
    w = fused.stem_weight_of(conv)
    assert w.shape == (27, channels) and w.dtype == torch.float32 and w.is_contiguous()
    for ky in range(3):
        for kx in range(3):
            for ci in range(3):
                assert torch.equal(w[(ky * 3 + kx) * 3 + ci], conv.weight[:, ci, ky, kx].detach())


def test_weight_operand_follows_the_weight():
    conv, other = _stem(24), _stem(24, stride=1)
    w = fused.stem_weight_of(conv)
    assert fused.stem_weight_of(conv) is w
    conv.load_state_dict(other.state_dict())
    w2 = fused.stem_weight_of(conv)                          # (the kept tensor, overwritten in place: a HIP graph may hold its address)
    assert w2 is w and torch.equal(w2[5], other.weight[:, 2, 0, 1].detach()) and fused.stem_weight_of(conv) is w2
    old = w2.clone()
    with torch.no_grad():
        conv.weight.mul_(2.0)
    w3 = fused.stem_weight_of(conv)
    assert w3 is w2 and torch.equal(w3, old * 2.0) and fused.stem_weight_of(conv) is w3
    assert [k for k in conv.state_dict()] == ['weight', 'bias']


class _OnDevice(torch.Tensor):
    is_cuda = True


def _x(channels=3, dtype=torch.float32):
    return torch.zeros((2, channels, 9, 7), dtype=dtype).contiguous(memory_format=torch.channels_last).as_subclass(_OnDevice)


def test_supported_declines(monkeypatch):
    """Every reason on its own.  A CPU tensor that says it is on the GPU stands in for one (``test_launch_marshalling.py`` does the
    same), so that each case is declined for the reason it names and not for the device; the first case is the device."""
    from openpifpaf_amd import _lib
    monkeypatch.setattr(_lib, 'available', lambda: True)
    with torch.no_grad():
        assert fused.stem_conv3x3_supported(_stem(), _x()), 'the base case is not accepted: the cases below would show nothing'
        assert fused.stem_conv3x3_supported(_stem(16, 1, bias=False), _x().contiguous().as_subclass(_OnDevice))
        assert not fused.stem_conv3x3_supported(_stem(), torch.zeros(2, 3, 9, 7))                       # a CPU tensor
        assert not fused.stem_conv3x3_supported(_stem().bfloat16(), _x(dtype=torch.bfloat16))
        assert not fused.stem_conv3x3_supported(_stem(), _x(dtype=torch.bfloat16))
        assert not fused.stem_conv3x3_supported(_stem().bfloat16(), _x())
        with monkeypatch.context() as m:                                                                # autocast
            m.setattr(torch, 'is_autocast_enabled', lambda *a: True)
            assert not fused.stem_conv3x3_supported(_stem(), _x())
        assert not fused.stem_conv3x3_supported(_stem(), _x().requires_grad_())
        assert not fused.stem_conv3x3_supported(_stem(in_channels=4), _x(4))
        assert not fused.stem_conv3x3_supported(_stem(), _x(4))
        assert not fused.stem_conv3x3_supported(_stem(kernel_size=5, padding=2), _x())
        assert not fused.stem_conv3x3_supported(_stem(padding=0), _x())
        assert not fused.stem_conv3x3_supported(_stem(dilation=2, padding=2), _x())
        assert not fused.stem_conv3x3_supported(_stem(dilation=2), _x())
        assert not fused.stem_conv3x3_supported(_stem(in_channels=3, groups=3, channels=24), _x())
        assert not fused.stem_conv3x3_supported(_stem(40), _x())
        assert not fused.stem_conv3x3_supported(_stem(stride=3), _x())
        assert not fused.stem_conv3x3_supported(_stem(stride=(2, 1)), _x())
        assert not fused.stem_conv3x3_supported(_stem(padding_mode='reflect'), _x())
        assert not fused.stem_conv3x3_supported(_stem(), _x()[0])                                      # three dimensions
        assert not fused.stem_conv3x3_supported(_stem(), torch.zeros(2, 3, 0, 7).as_subclass(_OnDevice))                      # no pixel
        assert not fused.stem_conv3x3_supported(_stem(), torch.zeros(1, 1, 9, 7).expand(2, 3, 9, 7).as_subclass(_OnDevice))   # a stride of 0
        monkeypatch.setattr(fused, 'STEM_DECLINED', frozenset({32}))
        assert not fused.stem_conv3x3_supported(_stem(), _x()) and fused.stem_conv3x3_supported(_stem(24), _x())
        monkeypatch.setattr(fused, 'STEM_DECLINED', frozenset())
        monkeypatch.setattr(_lib, 'available', lambda: False)
        assert not fused.stem_conv3x3_supported(_stem(), _x())
    # parameters that autograd follows, with gradients enabled
    monkeypatch.setattr(_lib, 'available', lambda: True)
    assert not fused.stem_conv3x3_supported(_stem(), _x())
    frozen = _stem().requires_grad_(False)
    assert fused.stem_conv3x3_supported(frozen, _x())


def test_the_switch_is_read_once_and_ships_off():
    code = 'from openpifpaf_amd import fused; print(int(fused.STEM))'
    for env, want in (({}, '0'), ({'OPA_STEM': '1'}, '1'), ({'OPA_STEM': '0'}, '0')):
        clean = {k: v for k, v in os.environ.items() if k != 'OPA_STEM'}
        proc = subprocess.run([sys.executable, '-c', code], env=dict(clean, **env), cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert proc.returncode == 0 and proc.stdout.split('\n')[-2] == want, (env, proc.stdout[-500:], proc.stderr[-500:])
    if 'OPA_STEM' not in os.environ:
        assert fused.STEM is False


def test_the_activations_map_to_their_codes():
    assert network._stem_act(nn.ReLU(inplace=True)) == (fused.ACT_RELU, 0.0) == (1, 0.0)
    assert network._stem_act(nn.Hardswish()) == (fused.ACT_HARDSWISH, 0.0) == (2, 0.0)
    assert network._stem_act(nn.LeakyReLU(0.2)) == (fused.ACT_LEAKY_RELU, 0.2) == (3, 0.2)
    assert network._stem_act(nn.LeakyReLU()) == (3, 0.01)
    assert network._stem_act(nn.ReLU6()) == (fused.ACT_RELU6, 6.0) == (4, 6.0)
    assert network._stem_act(nn.Sigmoid()) is None and network._stem_act(nn.Identity()) is None


@pytest.mark.parametrize('name', FAMILIES + ['shufflenetv2k16-leaky'])
def test_optimized_network_on_the_cpu_gives_the_unfused_result(name, monkeypatch):
    """With the switch ON: on the CPU the route is not taken, and the optimized float32 network computes what the unfused one does.
    The two differ by the folding of the batch norms alone -- a few float32 roundings per layer, which the later layers carry on:
    1e-4 of the output's size, the bound every route test here puts on "the same network, rounded differently"; a stem applied
    without its bias or with the wrong activation moves the output by order one."""
    monkeypatch.setattr(fused, 'STEM', True)
    base = network.ShuffleNetV2K('shufflenetv2k16', leaky_relu=True) if name.endswith('-leaky') else network.BASE_FACTORIES[name]()
    base = tc.randomize_(base, 5)
    x = torch.randn((1, 3, 33, 49), generator=tc.gen(6))

    def no_launch(*args, **kwargs):
        raise AssertionError('the stem kernel was launched on the CPU')
    monkeypatch.setattr(fused, 'stem_conv3x3_bias_act', no_launch)
    with torch.no_grad():
        want = base(x)
        opt = network.optimize_for_inference_(copy.deepcopy(base))
        assert opt.fused
        got = opt(x)
        got_cl = opt(x.contiguous(memory_format=torch.channels_last))
    assert got.shape == want.shape and want.isfinite().all()
    scale = float(want.abs().max())
    assert float((got - want).abs().max()) <= 1e-4 * scale and float((got_cl - want).abs().max()) <= 1e-4 * scale
