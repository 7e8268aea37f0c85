"""Host side of the bf16 grouped 3x3 implicit-GEMM route (``fused.GCONV_BF16``, ``fused.gconv3x3_bias_act_bf16``,
csrc/gconv3x3_bf16.hip): the packed block-diagonal weight against ``F.conv2d(..., groups=)`` in float64, its cache, what
``gconv3x3_bf16_supported`` declines, and which launches a bfloat16 ResNeXt ``_Bottleneck`` makes with the switch off and on -- traced
on the CPU with a recorder in place of ``fused._launch`` and tensors that say they are on the GPU.  No GPU is touched."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from openpifpaf_amd import _lib, fused, network

import trunk_common as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CL = torch.channels_last
BF16 = torch.bfloat16
SYMBOL = 'opa_gconv3x3_act_bf16'


class _OnDevice(torch.Tensor):
    is_cuda = True


def _t(channels=128, dtype=BF16, hw=(9, 7), batch=2):
    return torch.zeros((batch, channels) + hw, dtype=dtype).contiguous(memory_format=CL).as_subclass(_OnDevice)


def _conv(c=128, cg=4, stride=1, dilation=1, padding=None, dtype=BF16, n=None):
    padding = dilation if padding is None else padding
    return nn.Conv2d(c, n or c, 3, stride, padding, dilation=dilation, groups=c // cg, bias=False).to(dtype).requires_grad_(False)


def _bias(n=128, dtype=BF16):
    return torch.zeros(n, dtype=dtype)


# ---- the derived operands -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('c,cg', [(64, 4), (128, 8), (192, 16), (128, 32), (192, 64)])
def test_the_packed_weight_multiplied_out_is_the_grouped_convolution(c, cg):
    """Per 64-channel chunk, the 9 taps of the packed weight against the chunk's own channel slice -- in float64 -- are
    ``F.conv2d(..., groups=)``; every off-group entry is exactly zero, every in-group one the weight's own."""
    torch.manual_seed(c + cg)
    conv, bias = _conv(c, cg), torch.randn(c).to(BF16)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape))
    w9, b32 = fused.gconv3x3_bf16_weight_of(conv, bias)
    assert w9.dtype == BF16 and tuple(w9.shape) == (c, 9, 64) and w9.is_contiguous()
    assert b32.dtype == torch.float32 and torch.equal(b32, bias.float()) and b32.is_contiguous()    # (bf16 -> float32 is exact)
    co, j = torch.arange(c)[:, None], torch.arange(64)[None, :]
    own = (j // cg) == ((co % 64) // cg)                                                          # [c, 64]
    assert bool((w9.permute(1, 0, 2)[:, ~own] == 0).all())                                        # exactly zero off the group
    assert int(own.sum()) == c * cg and torch.equal(w9.permute(0, 2, 1)[own].reshape(c, cg, 3, 3), conv.weight)
    x = torch.randn(2, c, 6, 5, dtype=torch.float64)
    want = F.conv2d(x, conv.weight.double(), None, 1, 1, 1, c // cg)
    xp = F.pad(x, (1, 1, 1, 1))
    got = torch.zeros_like(want)
    for n0 in range(0, c, 64):
        for ky in range(3):
            for kx in range(3):
                window = xp[:, n0:n0 + 64, ky:ky + 6, kx:kx + 5]                                  # [B, 64, h, w]: the chunk's own slice
                got[:, n0:n0 + 64] += torch.einsum('bjhw,oj->bohw', window, w9[n0:n0 + 64, 3 * ky + kx].double())
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
    again = fused.gconv3x3_bf16_weight_of(conv, bias)
    assert again[0] is w9 and again[1] is b32                                              # kept on the module
    assert fused.gconv3x3_bf16_weight_of(_conv(c, cg))[1] is None                          # no bias: none handed over
    assert '_opa_w_gconv_bf16' not in conv.state_dict() and len(conv.state_dict()) == 1


def _grouped_block(seed, stride=1, downsample=False, inplanes=256):
    ds = None
    if downsample:
        ds = nn.Sequential(nn.Conv2d(inplanes, 256, 1, stride, bias=False), nn.BatchNorm2d(256))
    return tc.randomize_(network._Bottleneck(inplanes, 64, stride, ds, groups=32, base_width=4), seed)   # ResNeXt 32x4d, layer 1


def _optimized_bf16(block):
    return network.optimize_for_inference_(block).to(BF16).requires_grad_(False)


def test_the_operands_are_derived_again_when_the_parameters_change():
    block = _optimized_bf16(_grouped_block(2))
    conv, bias = block.conv2, block.fb2
    assert conv.groups == 32 and conv.in_channels == 128

    def unpacked(w9):
        co, j = torch.arange(128)[:, None], torch.arange(64)[None, :]
        return w9.permute(0, 2, 1)[(j // 4) == ((co % 64) // 4)].reshape(128, 4, 3, 3)
    w9, b32 = fused.gconv3x3_bf16_weight_of(conv, bias)
    w9_0, b32_0 = w9.clone(), b32.clone()
    torch.manual_seed(3)
    state = {k: torch.randn_like(v) for k, v in block.state_dict().items()}
    block.load_state_dict(state)                                                          # (in place: the version counters move)
    w9b, b32b = fused.gconv3x3_bf16_weight_of(conv, bias)
    # (the pointers stayed: the KEPT tensors are overwritten in place -- an address a HIP graph holds sees the new weights)
    assert w9b is w9 and torch.equal(unpacked(w9b), state['conv2.weight']) and not torch.equal(w9b, w9_0)
    assert b32b is b32 and torch.equal(b32b, state['fb2'].float()) and not torch.equal(b32b, b32_0)
    w9_1 = w9b.clone()
    with torch.no_grad():                                                                 # an in-place update of the weight alone
        conv.weight.mul_(2.0)
    w9c, b32c = fused.gconv3x3_bf16_weight_of(conv, bias)
    assert w9c is w9b and torch.equal(w9c, w9_1 * 2) and torch.equal(b32c, state['fb2'].float())
    with torch.no_grad():                                                                 # ... and of the folded bias alone
        bias.add_(1.0)
    assert torch.equal(fused.gconv3x3_bf16_weight_of(conv, bias)[1], bias.float())
    conv.weight = nn.Parameter(torch.ones_like(conv.weight), requires_grad=False)         # a weight REPLACED
    w9d = fused.gconv3x3_bf16_weight_of(conv, bias)[0]
    assert bool((unpacked(w9d) == 1).all()) and int((w9d != 0).sum()) == 128 * 9 * 4
    conv.to(torch.float32)                                                                # ... and converted
    assert fused.gconv3x3_bf16_weight_of(conv, bias)[0].dtype == torch.float32


# ---- gconv3x3_bf16_supported -----------------------------------------------------------------------------------------------------------

def test_supported_declines(monkeypatch):
    """Every reason on its own; the base cases first, so that the declines below show something."""
    monkeypatch.setattr(fused, 'GCONV_BF16', True)
    monkeypatch.setattr(_lib, 'available', lambda: True)
    ok = fused.gconv3x3_bf16_supported
    conv, x, bias = _conv(), _t(), _bias()
    with torch.no_grad():
        assert ok(conv, x, bias) and ok(conv, x, None) and ok(conv, x, bias.float())
        assert ok(_conv(stride=2), x, bias) and ok(_conv(dilation=2), x, bias) and ok(_conv(dilation=4), x, bias)
        for cg in (8, 16, 32, 64):
            assert ok(_conv(cg=cg), x, bias), cg
        assert ok(_conv(192, 64), _t(192), _bias(192)) and ok(_conv(64, 4), _t(64), _bias(64))
        # the switch, the library, the device, the dtypes, autocast
        with monkeypatch.context() as m:
            m.setattr(fused, 'GCONV_BF16', False)
            assert not ok(conv, x, bias)
        with monkeypatch.context() as m:
            m.setattr(_lib, 'available', lambda: False)
            assert not ok(conv, x, bias)
        assert not ok(conv, torch.zeros(2, 128, 9, 7, dtype=BF16).contiguous(memory_format=CL), bias)         # a CPU tensor
        assert not ok(_conv(dtype=torch.float32), _t(dtype=torch.float32), bias.float())                       # float32
        assert not ok(_conv(dtype=torch.float32), x, bias)                                                     # autocast's pairing
        assert not ok(conv, _t(dtype=torch.float32), bias) and not ok(conv, _t(dtype=torch.float16), bias)
        with monkeypatch.context() as m:
            m.setattr(torch, 'is_autocast_enabled', lambda *a: True)
            assert not ok(conv, x, bias)
        # NCHW, a channel slice (not dense), other channels, no pixels
        assert not ok(conv, torch.zeros(2, 128, 9, 7, dtype=BF16).as_subclass(_OnDevice), bias)
        assert not ok(conv, _t(256)[:, :128], bias) and not ok(conv, _t(256), bias)
        assert not ok(conv, _t(hw=(0, 7)), bias)
        # groups: none (the dense route's), one per channel pair, widths that do not divide 64
        assert not ok(nn.Conv2d(128, 128, 3, 1, 1, bias=False).to(BF16).requires_grad_(False), x, bias)
        assert not ok(_conv(cg=2), x, bias) and not ok(_conv(cg=1), x, bias)
        assert not ok(_conv(192, 12), _t(192), _bias(192)) and not ok(_conv(192, 24), _t(192), _bias(192))
        assert not ok(_conv(384, 128), _t(384), _bias(384))
        # channels: no multiple of 64, more output than input channels
        assert not ok(_conv(96, 4), _t(96), _bias(96)) and not ok(_conv(32, 4), _t(32), _bias(32))
        assert not ok(_conv(128, 4, n=256), x, _bias(256))
        # another convolution: a bias of its own, 1x1, 5x5, padding != dilation, a stride of 3, a dilation of 3, stride 2 dilated
        own = nn.Conv2d(128, 128, 3, 1, 1, groups=32).to(BF16).requires_grad_(False)
        assert own.bias is not None and not ok(own, x, bias)
        assert not ok(nn.Conv2d(128, 128, 1, groups=32, bias=False).to(BF16).requires_grad_(False), x, bias)
        assert not ok(nn.Conv2d(128, 128, 5, 1, 2, groups=32, bias=False).to(BF16).requires_grad_(False), x, bias)
        assert not ok(_conv(padding=0), x, bias) and not ok(_conv(dilation=2, padding=1), x, bias) and not ok(_conv(padding=2), x, bias)
        assert not ok(_conv(stride=3), x, bias) and not ok(_conv(dilation=3), x, bias) and not ok(_conv(stride=2, dilation=2), x, bias)
        assert not ok(nn.Conv2d(128, 128, 3, (1, 2), 1, groups=32, bias=False).to(BF16).requires_grad_(False), x, bias)
        # the folded bias: another length, another dtype
        assert not ok(conv, x, _bias(64)) and not ok(conv, x, _bias(dtype=torch.float16))
        # a layer the timing declined
        with monkeypatch.context() as m:
            m.setattr(fused, 'GCONV_BF16_DECLINED', frozenset({(128, 4, 1)}))
            assert not ok(conv, x, bias) and ok(_conv(stride=2), x, bias) and ok(_conv(cg=8), x, bias)
    assert fused.GCONV_BF16_DECLINED == frozenset()
    # no residual operand: the predicate takes none
    with pytest.raises(TypeError):
        ok(conv, x, bias, _t())
    # grad enabled and something that autograd follows
    assert ok(conv, x, bias)
    assert not ok(conv, _t().requires_grad_(), bias) and not ok(_conv().requires_grad_(True), x, bias)
    assert not ok(conv, x, _bias(dtype=torch.float32).requires_grad_())


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


def _reset(trace):
    del trace['launches'][:], trace['conv_bias_act'][:]
    trace['bias_act_'] = 0


def test_the_route_row_is_the_last_one_and_competes_with_nothing():
    names = [row[0] for row in network._CONV3_ROUTES]
    assert names[-1] == 'gconv-bf16' and names.count('gconv-bf16') == 1 and names[:-1] == ['wino', 'x3', 'x3-dilated', 'gconv', 'bf16']
    _, _, _, adds_residual, pick_key = network._CONV3_ROUTES[-1]
    assert adds_residual is False and pick_key is None


@pytest.mark.parametrize('stride,downsample,dilation', [(1, False, 1), (2, True, 1), (1, True, 2), (1, False, 4)])
def test_a_bfloat16_resnext_bottleneck_takes_the_kernel_for_conv2_and_the_plain_gemm_behind_it(trace, monkeypatch, stride, downsample, dilation):
    block = _grouped_block(4, stride, downsample)
    if dilation != 1:
        network._dilate_(block, dilation)
    block = _optimized_bf16(block)
    x = _t(256, hw=(9, 7))
    for on in (True, False):
        monkeypatch.setattr(fused, 'GCONV_BF16', on)
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


def test_the_route_is_reached_only_for_grouped_bfloat16_operands_with_the_switch_on(trace, monkeypatch):
    monkeypatch.setattr(fused, 'FORCE_PICK', 'conv')                                      # (float32: nothing is timed without a device)
    calls = []
    run = fused.gconv3x3_bias_act_bf16
    monkeypatch.setattr(fused, 'gconv3x3_bias_act_bf16', lambda *a, **kw: calls.append(a[0]) or run(*a, **kw))
    with torch.no_grad():
        # the switch off: every other bf16 switch on changes nothing for the grouped convolution
        monkeypatch.setattr(fused, 'CONV3_BF16', True)
        _optimized_bf16(_grouped_block(6))(_t(256))
        assert not calls and SYMBOL not in trace['launches']
        monkeypatch.setattr(fused, 'GCONV_BF16', True)
        # float32 grouped, bfloat16 dense (the dense row's), autocast: not this row
        network.optimize_for_inference_(_grouped_block(6))(_t(256, dtype=torch.float32))
        _optimized_bf16(tc.bottleneck(256, 64, 1, False, 6))(_t(256))
        _optimized_bf16(tc.basic_block(64, 64, 1, False, 6))(_t(64))
        assert not calls and SYMBOL not in trace['launches']
        assert trace['launches'].count('opa_conv3x3_act_bf16') == 3
        with monkeypatch.context() as m:
            m.setattr(torch, 'is_autocast_enabled', lambda *a: True)
            _optimized_bf16(_grouped_block(6))(_t(256))
        assert not calls and SYMBOL not in trace['launches']
        # grouped, bfloat16, the switch on
        block = _optimized_bf16(_grouped_block(6))
        block(_t(256))
        assert calls == [block.conv2] and trace['launches'].count(SYMBOL) == 1
        # ... and not where the dense row is skipped by name only
        out, owed = network._conv3x3(block.conv2, _t(128), block.fb2, skip=('gconv-bf16',), defer=True)
        assert owed is block.fb2 and len(calls) == 1


def test_the_switch_is_read_once_and_ships_off():
    code = 'from openpifpaf_amd import fused; print(int(fused.GCONV_BF16))'
    for env, want in (({}, '0'), ({'OPA_GCONV_BF16': '1'}, '1'), ({'OPA_GCONV_BF16': '0'}, '0')):
        clean = {k: v for k, v in os.environ.items() if k != 'OPA_GCONV_BF16'}
        proc = subprocess.run([sys.executable, '-c', code], env=dict(clean, **env), cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert proc.returncode == 0 and proc.stdout.split('\n')[-2] == want, (env, proc.stdout[-500:], proc.stderr[-500:])


def test_the_header_the_binding_and_the_library_agree():
    with open(os.path.join(ROOT, 'include', 'openpifpaf_amd.h')) as f:
        header = f.read()
    assert SYMBOL + '(' in header and SYMBOL in _lib.SYMBOLS and hasattr(_lib.lib(), SYMBOL)
    declaration = header.split('int ' + SYMBOL + '(')[1].split(');')[0]
    assert len(declaration.split(',')) == 13                                             # 12 arguments and the stream
    assert len(_lib.SYMBOLS[SYMBOL][1]) == 13
    assert '32-ALIGNED CHANNEL BLOCK' in header.split('int ' + SYMBOL + '(')[0][-3000:]  # the contract for non-finite values
