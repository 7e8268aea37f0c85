"""Host side of the bf16 3x3 implicit-GEMM route (``fused.CONV3_BF16``, ``fused.conv3x3_bias_act_bf16``, csrc/conv3x3_bf16.hip): the
derived operands, what ``conv3x3_bf16_supported`` declines, and which launches a bfloat16 ``_Bottleneck`` and ``_BasicBlock`` make
with the switch off and on -- traced on the CPU with a recorder in place of ``fused._launch`` and tensors that say they are on the
GPU.  No GPU is touched."""
import os
import subprocess
import sys

import pytest
import torch
from torch import nn

from openpifpaf_amd import _lib, fused, network

import trunk_common as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CL = torch.channels_last
BF16 = torch.bfloat16
SYMBOL = 'opa_conv3x3_act_bf16'


class _OnDevice(torch.Tensor):
    is_cuda = True


def _t(channels=64, dtype=BF16, hw=(9, 7), batch=2):
    return torch.zeros((batch, channels) + hw, dtype=dtype).contiguous(memory_format=CL).as_subclass(_OnDevice)


def _conv(c=64, n=128, stride=1, dilation=1, padding=None, dtype=BF16, **kw):
    padding = dilation if padding is None else padding
    return nn.Conv2d(c, n, 3, stride, padding, dilation=dilation, bias=False, **kw).to(dtype).requires_grad_(False)


def _bias(n=128, dtype=BF16):
    return torch.zeros(n, dtype=dtype)


# ---- the derived operands -----------------------------------------------------------------------------------------------------------

def test_the_weight_is_tap_major_and_the_bias_upcast():
    torch.manual_seed(1)
    conv, bias = _conv(), torch.randn(128).to(BF16)
    w9, b32 = fused.conv3x3_bf16_weight_of(conv, bias)
    assert w9.dtype == BF16 and tuple(w9.shape) == (128, 9, 64) and w9.is_contiguous()
    assert torch.equal(w9.view(128, 3, 3, 64), conv.weight.permute(0, 2, 3, 1))
    for ky in range(3):
        for kx in range(3):
            assert torch.equal(w9[:, 3 * ky + kx], conv.weight[:, :, ky, kx])
    assert b32.dtype == torch.float32 and torch.equal(b32, bias.float()) and b32.is_contiguous()    # (bf16 -> float32 is exact)
    again = fused.conv3x3_bf16_weight_of(conv, bias)
    assert again[0] is w9 and again[1] is b32                                              # kept on the module
    assert fused.conv3x3_bf16_weight_of(_conv())[1] is None                                # no bias: none handed over


def test_the_operands_are_derived_again_when_the_parameters_change():
    torch.manual_seed(2)
    block = network.optimize_for_inference_(tc.basic_block(64, 64, 1, False, 3)).to(BF16)
    conv, bias = block.conv1, block.fb1
    w9, b32 = fused.conv3x3_bf16_weight_of(conv, bias)
    w9_0, b32_0 = w9.clone(), b32.clone()
    state = {k: torch.randn_like(v) for k, v in block.state_dict().items()}
    block.load_state_dict(state)                                                          # (in place: the version counters move)
    w9b, b32b = fused.conv3x3_bf16_weight_of(conv, bias)
    # (the same pointers, no new version: the KEPT tensors are overwritten in place -- an address a HIP graph holds sees the new weights)
    assert w9b is w9 and torch.equal(w9b.view(64, 3, 3, 64), state['conv1.weight'].permute(0, 2, 3, 1)) and not torch.equal(w9b, w9_0)
    assert b32b is b32 and torch.equal(b32b, state['fb1'].float()) and not torch.equal(b32b, b32_0)
    w9_1 = w9b.clone()
    with torch.no_grad():                                                                 # an in-place update of the weight alone
        conv.weight.mul_(2.0)
    w9c, b32c = fused.conv3x3_bf16_weight_of(conv, bias)
    assert w9c is w9b and torch.equal(w9c, w9_1 * 2) and torch.equal(b32c, state['fb1'].float())
    with torch.no_grad():                                                                 # ... and of the folded bias alone
        bias.add_(1.0)
    assert torch.equal(fused.conv3x3_bf16_weight_of(conv, bias)[1], bias.float())
    conv.weight = nn.Parameter(torch.ones_like(conv.weight), requires_grad=False)         # a weight REPLACED
    assert bool((fused.conv3x3_bf16_weight_of(conv, bias)[0] == 1).all())


# ---- conv3x3_bf16_supported ------------------------------------------------------------------------------------------------------------

def test_supported_declines(monkeypatch):
    """Every reason on its own; the base cases first, so that the declines below show something."""
    monkeypatch.setattr(fused, 'CONV3_BF16', True)
    monkeypatch.setattr(_lib, 'available', lambda: True)
    ok = fused.conv3x3_bf16_supported
    conv, x, bias = _conv(), _t(), _bias()
    with torch.no_grad():
        assert ok(conv, x, bias) and ok(conv, x, None) and ok(conv, x, bias.float())
        assert ok(conv, x, bias, _t(128)) and ok(_conv(stride=2), x, bias, _t(128, hw=(5, 4)))
        assert ok(_conv(dilation=2), x, bias) and ok(_conv(dilation=4), x, bias, _t(128))
        assert ok(_conv(128, 192), _t(128), _bias(192))
        # the switch, the device, the dtypes, autocast
        with monkeypatch.context() as m:
            m.setattr(fused, 'CONV3_BF16', False)
            assert not ok(conv, x, bias)
        with monkeypatch.context() as m:
            m.setattr(_lib, 'available', lambda: False)
            assert not ok(conv, x, bias)
        assert not ok(conv, torch.zeros(2, 64, 9, 7, dtype=BF16).contiguous(memory_format=CL), bias)          # a CPU tensor
        assert not ok(_conv(dtype=torch.float32), _t(dtype=torch.float32), bias.float())                       # float32
        assert not ok(_conv(dtype=torch.float32), x, bias)                                                     # autocast's pairing
        assert not ok(conv, _t(dtype=torch.float32), bias) and not ok(conv, _t(dtype=torch.float16), bias)
        with monkeypatch.context() as m:
            m.setattr(torch, 'is_autocast_enabled', lambda *a: True)
            assert not ok(conv, x, bias)
        # NCHW, a channel slice (not dense), other channels, no pixels
        assert not ok(conv, torch.zeros(2, 64, 9, 7, dtype=BF16).as_subclass(_OnDevice), bias)
        assert not ok(conv, _t(128)[:, :64], bias) and not ok(conv, _t(128), bias)
        assert not ok(conv, _t(hw=(0, 7)), bias)
        # another convolution: groups, a bias of its own, 1x1, 5x5, padding != dilation, a stride of 3, a dilation of 3, stride 2 dilated
        assert not ok(_conv(groups=2), x, bias)
        own = nn.Conv2d(64, 128, 3, 1, 1).to(BF16).requires_grad_(False)
        assert own.bias is not None and not ok(own, x, bias)
        assert not ok(nn.Conv2d(64, 128, 1, bias=False).to(BF16).requires_grad_(False), x, bias)
        assert not ok(nn.Conv2d(64, 128, 5, 1, 2, bias=False).to(BF16).requires_grad_(False), x, bias)
        assert not ok(_conv(padding=0), x, bias) and not ok(_conv(dilation=2, padding=1), x, bias) and not ok(_conv(padding=2), x, bias)
        assert not ok(_conv(stride=3), x, bias) and not ok(_conv(dilation=3), x, bias) and not ok(_conv(stride=2, dilation=2), x, bias)
        assert not ok(nn.Conv2d(64, 128, 3, (1, 2), 1, bias=False).to(BF16).requires_grad_(False), x, bias)
        # channel counts that are no multiples of 64
        assert not ok(_conv(32, 128), _t(32), bias) and not ok(_conv(64, 96), x, _bias(96)) and not ok(_conv(72, 128), _t(72), bias)
        # the folded bias: another length, another dtype
        assert not ok(conv, x, _bias(64)) and not ok(conv, x, _bias(dtype=torch.float16))
        # the residual: float32, other pixels, other channels, NCHW, not dense
        assert not ok(conv, x, bias, _t(128, dtype=torch.float32)) and not ok(conv, x, bias, _t(128, hw=(9, 8)))
        assert not ok(conv, x, bias, _t(64)) and not ok(conv, x, bias, torch.zeros(2, 128, 9, 7, dtype=BF16).as_subclass(_OnDevice))
        assert not ok(conv, x, bias, _t(256)[:, :128]) and not ok(_conv(stride=2), x, bias, _t(128))
    # grad enabled and something that autograd follows
    assert ok(conv, x, bias)
    assert not ok(conv, _t().requires_grad_(), bias) and not ok(conv, x, bias, _t(128).requires_grad_())
    assert not ok(_conv().requires_grad_(True), x, bias)


# ---- the routes -------------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def trace(monkeypatch):
    """A recorder in place of ``fused._launch`` (nothing runs: the outputs hold zeros), outputs that say they are on the GPU like their
    inputs, the library reported as built; ``fused.conv_bias_act`` and ``fused.bias_act_`` recorded on their way.
    -> {'launches': [symbols], 'conv_bias_act': [(conv, a_bias)], 'bias_act_': count}"""
    seen = {'launches': [], 'conv_bias_act': [], 'bias_act_': 0}
    monkeypatch.setattr(fused, '_launch', lambda symbol, *args: seen['launches'].append(symbol))
    empty = fused._empty_nhwc
    monkeypatch.setattr(fused, '_empty_nhwc', lambda *a, **kw: empty(*a, **kw).zero_().as_subclass(_OnDevice))
    monkeypatch.setattr(_lib, 'available', lambda: True)
    conv_bias_act, bias_act_ = fused.conv_bias_act, fused.bias_act_

    def traced_conv_bias_act(conv, x, bias, residual=None, relu=True, a_bias=None):
        seen['conv_bias_act'].append((conv, a_bias))
        return conv_bias_act(conv, x, bias, residual, relu, a_bias)

    def traced_bias_act_(*args, **kw):
        seen['bias_act_'] += 1
        return bias_act_(*args, **kw)
    monkeypatch.setattr(fused, 'conv_bias_act', traced_conv_bias_act)
    monkeypatch.setattr(fused, 'bias_act_', traced_bias_act_)
    return seen


def _optimized_bf16(block):
    return network.optimize_for_inference_(block).to(BF16).requires_grad_(False)


def _reset(trace):
    del trace['launches'][:], trace['conv_bias_act'][:]
    trace['bias_act_'] = 0


@pytest.mark.parametrize('stride,downsample,dilation', [(1, False, 1), (2, True, 1), (1, True, 2)])
def test_a_bfloat16_bottleneck_takes_the_kernel_for_conv2_and_the_plain_gemm_behind_it(trace, monkeypatch, stride, downsample, dilation):
    block = tc.bottleneck(256, 64, stride, downsample, 4)
    if dilation != 1:
        network._dilate_(block, dilation)
    block = _optimized_bf16(block)
    x = _t(256, hw=(9, 7))
    for on in (True, False):
        monkeypatch.setattr(fused, 'CONV3_BF16', on)
        _reset(trace)
        with torch.no_grad():
            out = block(x)
        assert tuple(out.shape) == (2, 256) + ((5, 4) if stride == 2 else (9, 7)) and out.dtype == BF16
        assert trace['launches'].count(SYMBOL) == (1 if on else 0), (on, trace['launches'])
        (conv1, a_bias1), (conv3, a_bias3) = trace['conv_bias_act']
        assert conv1 is block.conv1 and a_bias1 is None and conv3 is block.conv3
        # on: conv2's bias + ReLU are the kernel's, conv3 is the plain GEMM; off: conv2's raw output and its epilogue left to conv3's operand
        assert (a_bias3 is None) if on else (a_bias3 is block.fb2), on
        assert 'opa_gemm_pro_bias_act_bf16' not in trace['launches'] or not on


@pytest.mark.parametrize('stride,downsample,dilation', [(1, False, 1), (2, True, 1), (1, False, 2)])
def test_a_bfloat16_basic_block_makes_two_launches_and_no_epilogue_pass(trace, monkeypatch, stride, downsample, dilation):
    block = tc.basic_block(64, 128 if downsample else 64, stride, downsample, 5)
    if dilation != 1:
        network._dilate_(block, dilation)
    block = _optimized_bf16(block)
    x = _t(64, hw=(9, 7))
    for on in (True, False):
        monkeypatch.setattr(fused, 'CONV3_BF16', on)
        _reset(trace)
        with torch.no_grad():
            out = block(x)
        assert tuple(out.shape) == (2, 128 if downsample else 64) + ((5, 4) if stride == 2 else (9, 7)) and out.dtype == BF16
        assert trace['launches'].count(SYMBOL) == (2 if on else 0), (on, trace['launches'])
        assert trace['bias_act_'] == (0 if on else 2), (on, trace['bias_act_'])
        if on:
            assert trace['launches'] == [SYMBOL, SYMBOL]


def test_float32_autocast_and_grouped_blocks_stay_where_they_are(trace, monkeypatch):
    monkeypatch.setattr(fused, 'CONV3_BF16', True)
    monkeypatch.setattr(fused, 'FORCE_PICK', 'conv')                                      # (float32: nothing is timed without a device)
    basic, bottle = tc.basic_block(64, 64, 2, True, 6), tc.bottleneck(256, 64, 2, True, 6)
    with torch.no_grad():
        network.optimize_for_inference_(basic)(_t(64, dtype=torch.float32))
        network.optimize_for_inference_(bottle)(_t(256, dtype=torch.float32))
    assert SYMBOL not in trace['launches']
    grouped = tc.randomize_(network._Bottleneck(256, 64, 1, None, groups=32, base_width=4), 6)       # ResNeXt's
    with torch.no_grad():
        _optimized_bf16(grouped)(_t(256))
    assert SYMBOL not in trace['launches']
    monkeypatch.setattr(torch, 'is_autocast_enabled', lambda *a: True)
    with torch.no_grad():
        _optimized_bf16(tc.basic_block(64, 64, 1, False, 6))(_t(64))
    assert SYMBOL not in trace['launches']


def test_the_switch_is_read_once_and_ships_off():
    code = 'from openpifpaf_amd import fused; print(int(fused.CONV3_BF16))'
    for env, want in (({}, '0'), ({'OPA_CONV3_BF16': '1'}, '1'), ({'OPA_CONV3_BF16': '0'}, '0')):
        clean = {k: v for k, v in os.environ.items() if k != 'OPA_CONV3_BF16'}
        proc = subprocess.run([sys.executable, '-c', code], env=dict(clean, **env), cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert proc.returncode == 0 and proc.stdout.split('\n')[-2] == want, (env, proc.stdout[-500:], proc.stderr[-500:])


def test_the_header_the_binding_and_the_library_agree():
    with open(os.path.join(ROOT, 'include', 'openpifpaf_amd.h')) as f:
        header = f.read()
    assert SYMBOL + '(' in header and SYMBOL in _lib.SYMBOLS and hasattr(_lib.lib(), SYMBOL)
    declaration = header.split('int ' + SYMBOL + '(')[1].split(');')[0]
    assert len(declaration.split(',')) == 14                                             # 13 arguments and the stream
    assert len(_lib.SYMBOLS[SYMBOL][1]) == 14
    assert '#define OPA_ABI_VERSION 9' in header.replace('  ', ' ')
