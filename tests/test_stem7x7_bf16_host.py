"""Host side of the bf16 7x7 stem route (``fused.STEM7_BF16``, ``fused.stem7x7_bias_act_bf16``, csrc/stem7x7_bf16.hip): the derived
operands, what ``stem7x7_bf16_supported`` declines, what is handed to the C ABI for an NCHW, a channels-last and a cropped image, and
which launches a bfloat16 ``Resnet('resnet18')`` makes with the switch off and on -- traced on the CPU with a recorder in place of
``fused._launch`` and tensors that say they are on the GPU.  No GPU is touched."""
import os
import subprocess
import sys

import pytest
import torch
from torch import nn

from openpifpaf_amd import _lib, fused, network

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CL = torch.channels_last
BF16 = torch.bfloat16
SYMBOL = 'opa_stem7x7_act_bf16'


class _OnDevice(torch.Tensor):
    is_cuda = True


def _x(layout='cl', dtype=BF16, channels=3, hw=(9, 7), batch=2):
    """A ``[batch, channels, *hw]`` image that says it is on the GPU: 'cl' channels-last, 'nchw', or 'crop' -- a view of a larger
    channels-last image."""
    h, w = hw
    if layout == 'crop':
        big = torch.zeros((batch, channels, h + 5, w + 4), dtype=dtype).contiguous(memory_format=CL)
        return big[:, :, 2:2 + h, 1:1 + w].as_subclass(_OnDevice)
    x = torch.zeros((batch, channels) + hw, dtype=dtype)
    return (x.contiguous(memory_format=CL) if layout == 'cl' else x).as_subclass(_OnDevice)


def _conv(n=64, stride=2, k=7, padding=3, c=3, dtype=BF16, bias=False, **kw):
    return nn.Conv2d(c, n, k, stride, padding, bias=bias, **kw).to(dtype).requires_grad_(False)


def _bias(n=64, dtype=BF16):
    return torch.zeros(n, dtype=dtype)


# ---- the derived operands -----------------------------------------------------------------------------------------------------------

def test_the_weight_is_in_the_plans_k_order_with_zero_columns_and_the_bias_upcast():
    torch.manual_seed(1)
    conv, bias = _conv(), torch.randn(64).to(BF16)
    wk, b32 = fused.stem7x7_bf16_weight_of(conv, bias)
    assert wk.dtype == BF16 and tuple(wk.shape) == (64, 192) and wk.is_contiguous() and fused.STEM7_BF16_K == 192
    assert bool((conv.weight != 0).all())
    for k in range(192):                                                                   # element by element, from the definition
        ky, kx, ci = k // 24, k % 24 // 3, k % 3
        if ky < 7 and kx < 7:
            assert torch.equal(wk[:, k], conv.weight[:, ci, ky, kx]), k
        else:
            assert bool((wk[:, k] == 0).all()), k
    assert int((wk != 0).sum()) == 64 * 147
    assert b32.dtype == torch.float32 and torch.equal(b32, bias.float()) and b32.is_contiguous()    # (bf16 -> float32 is exact)
    again = fused.stem7x7_bf16_weight_of(conv, bias)
    assert again[0] is wk and again[1] is b32                                              # kept on the module
    assert fused.stem7x7_bf16_weight_of(_conv())[1] is None                                # no bias: none handed over


def test_the_operands_are_derived_again_when_the_parameters_change():
    torch.manual_seed(2)
    net = network.optimize_for_inference_(network.Resnet('resnet18').eval()).to(BF16).requires_grad_(False)
    conv, bias = net.input_block[0], net.fb0
    wk, b32 = fused.stem7x7_bf16_weight_of(conv, bias)
    wk_0, b32_0 = wk.clone(), b32.clone()
    state = {k: torch.randn_like(v) for k, v in net.state_dict().items()}
    net.load_state_dict(state)                                                            # (in place: the version counters move)
    wkb, b32b = fused.stem7x7_bf16_weight_of(conv, bias)
    # (the pointers stayed: the KEPT tensors are overwritten in place -- an address a HIP graph holds sees the new weights)
    assert wkb is wk and not torch.equal(wkb, wk_0)
    assert torch.equal(wkb.view(64, 8, 8, 3)[:, :7, :7], state['input_block.0.weight'].permute(0, 2, 3, 1))
    assert b32b is b32 and torch.equal(b32b, state['fb0'].float()) and not torch.equal(b32b, b32_0)
    wk_1 = wkb.clone()
    with torch.no_grad():                                                                 # an in-place update of the weight alone
        conv.weight.mul_(2.0)
    wkc, b32c = fused.stem7x7_bf16_weight_of(conv, bias)
    assert wkc is wkb and torch.equal(wkc, wk_1 * 2) and torch.equal(b32c, state['fb0'].float())
    with torch.no_grad():                                                                 # ... and of the folded bias alone
        bias.add_(1.0)
    assert torch.equal(fused.stem7x7_bf16_weight_of(conv, bias)[1], bias.float())
    conv.weight = nn.Parameter(torch.ones_like(conv.weight), requires_grad=False)         # a weight REPLACED
    assert int((fused.stem7x7_bf16_weight_of(conv, bias)[0] == 1).sum()) == 64 * 147


# ---- stem7x7_bf16_supported -----------------------------------------------------------------------------------------------------------

def test_supported_declines(monkeypatch):
    """Every reason on its own; the base cases first, so that the declines below show something."""
    monkeypatch.setattr(fused, 'STEM7_BF16', True)
    monkeypatch.setattr(_lib, 'available', lambda: True)
    ok = fused.stem7x7_bf16_supported
    conv, x, bias = _conv(), _x(), _bias()
    with torch.no_grad():
        assert ok(conv, x, bias) and ok(conv, x, None) and ok(conv, x, bias.float())
        assert ok(conv, _x('nchw'), bias) and ok(conv, _x('crop'), bias) and ok(_conv(stride=1), x, bias) and ok(_conv(128), x, _bias(128))
        with monkeypatch.context() as m:                                                  # the switch off
            m.setattr(fused, 'STEM7_BF16', False)
            assert not ok(conv, x, bias)
        with monkeypatch.context() as m:
            m.setattr(_lib, 'available', lambda: False)
            assert not ok(conv, x, bias)
        assert not ok(conv, torch.zeros(2, 3, 9, 7, dtype=BF16), bias)                    # a CPU tensor
        assert not ok(_conv(dtype=torch.float32), _x(dtype=torch.float32), bias.float())  # float32
        assert not ok(conv, _x(dtype=torch.float32), bias) and not ok(conv, _x(dtype=torch.float16), bias)
        assert not ok(_conv(dtype=torch.float32), x, bias)                                # autocast's pairing
        with monkeypatch.context() as m:                                                  # autocast
            m.setattr(torch, 'is_autocast_enabled', lambda *a: True)
            assert not ok(conv, x, bias)
        assert not ok(_conv(c=4), _x(channels=4), bias)                                   # 4 channels
        assert not ok(conv, _x(channels=4), bias)
        assert not ok(_conv(k=3, padding=1), x, bias)                                     # a 3x3 kernel
        assert not ok(_conv(k=5, padding=2), x, bias)
        assert not ok(_conv(stride=3), x, bias)                                           # stride 3
        assert not ok(nn.Conv2d(3, 64, 7, (1, 2), 3, bias=False).to(BF16).requires_grad_(False), x, bias)
        assert not ok(_conv(padding=2), x, bias)                                          # padding 2
        assert not ok(_conv(dilation=2), x, bias)
        own = _conv(bias=True)                                                            # a convolution with a bias
        assert own.bias is not None and not ok(own, x, bias)
        assert not ok(_conv(32), x, _bias(32)) and not ok(_conv(96), x, _bias(96))        # c_out 32
        assert not ok(conv, x, _bias(128)) and not ok(conv, x, _bias(dtype=torch.float16))  # the folded bias: another length, another dtype
        assert not ok(conv, _x(hw=(0, 7)), bias) and not ok(conv, _x(batch=0), bias)      # no pixels
        assert not ok(conv, _x('nchw').expand(2, 3, 9, 7)[:, :, :, :].as_strided((2, 3, 9, 7), (0, 63, 7, 1)).as_subclass(_OnDevice), bias)   # a stride of 0
        assert not ok(conv, torch.zeros(2, 9, 7, 3, dtype=BF16).permute(0, 3, 1, 2)[0].as_subclass(_OnDevice), bias)   # 3 dimensions
    # grad enabled and something that autograd follows
    assert ok(conv, x, bias)
    assert not ok(conv, _x(dtype=torch.float32).requires_grad_().to(BF16).as_subclass(_OnDevice), bias)                # requires_grad
    assert not ok(_conv().requires_grad_(True), x, bias) and not ok(conv, x, _bias().requires_grad_())


# ---- what is handed to the C ABI ------------------------------------------------------------------------------------------------------

@pytest.fixture
def trace(monkeypatch):
    """A recorder in place of ``fused._launch`` (nothing runs: the outputs hold zeros), outputs that say they are on the GPU like their
    inputs, the library reported as built, nothing timed (``FORCE_PICK``).  -> [(symbol, arguments)]"""
    seen = []
    monkeypatch.setattr(fused, '_launch', lambda symbol, *args: seen.append((symbol, args)))
    empty = fused._empty_nhwc
    monkeypatch.setattr(fused, '_empty_nhwc', lambda *a, **kw: empty(*a, **kw).zero_().as_subclass(_OnDevice))
    monkeypatch.setattr(_lib, 'available', lambda: True)
    monkeypatch.setattr(fused, 'FORCE_PICK', 'conv')
    monkeypatch.setattr(fused, 'STEM7_BF16', True)
    return seen


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('layout,strides', [('nchw', (3 * 9 * 7, 9 * 7, 7, 1)), ('cl', (9 * 7 * 3, 1, 7 * 3, 3)), ('crop', (14 * 11 * 3, 1, 11 * 3, 3))])
def test_the_call_argument_by_argument(trace, layout, strides, relu, stride):
    conv, x, bias = _conv(128, stride=stride), _x(layout), torch.ones(128, dtype=BF16)
    assert tuple(x.stride()) == strides                                                   # (in elements, as torch counts them)
    with torch.no_grad():
        out = fused.stem7x7_bias_act_bf16(conv, x, bias, relu=relu)
    wk, b32 = fused.stem7x7_bf16_weight_of(conv, bias)
    ho, wo = ((9, 7) if stride == 1 else (5, 4))
    assert tuple(out.shape) == (2, 128, ho, wo) and out.dtype == BF16 and out.is_contiguous(memory_format=CL)
    (symbol, args), = trace
    assert symbol == SYMBOL and len(args) + 1 == len(_lib.SYMBOLS[SYMBOL][1])             # (+ the stream, which _launch appends)
    assert args == (x.data_ptr(),) + strides + (wk.data_ptr(), b32.data_ptr(), out.data_ptr(), 2, 9, 7, 128, stride, int(relu))
    if layout == 'crop':                                                                  # the view's first element, not the larger image's
        assert args[0] == x.untyped_storage().data_ptr() + 2 * (2 * 11 * 3 + 1 * 3)
    del trace[:]
    with torch.no_grad():
        fused.stem7x7_bias_act_bf16(conv, x, None)
    assert trace[0][1][6] is None and trace[0][1][13] == 1                                # no bias: a null pointer; relu defaults to on


# ---- the routes -------------------------------------------------------------------------------------------------------------------------

def _resnet18(dtype=BF16, **options):
    torch.manual_seed(3)
    net = network.optimize_for_inference_(network.Resnet('resnet18', **options).eval())
    return net.to(dtype).requires_grad_(False)


def _stem_launches(trace, net, x, on):
    fused.STEM7_BF16 = on
    del trace[:]
    with torch.no_grad():
        out = net._input_block_fused(x)
    return out, list(trace)


@pytest.mark.parametrize('options,hw', [({}, (5, 4)), ({'pool0_stride': 2}, (3, 2)), ({'input_conv_stride': 1}, (9, 7)),
                                        ({'input_conv_stride': 1, 'pool0_stride': 2}, (5, 4))])
@pytest.mark.parametrize('layout', ['cl', 'nchw', 'crop'])
def test_a_bfloat16_resnet_stem_is_one_launch(trace, options, hw, layout):
    net, x = _resnet18(**options), _x(layout)
    pool = bool(options.get('pool0_stride'))
    out, on = _stem_launches(trace, net, x, True)
    assert tuple(out.shape) == (2, 64) + hw and out.dtype == BF16
    symbols = [s for s, _ in on]
    assert symbols == ([SYMBOL, 'opa_maxpool3x3_bias_act'] if pool else [SYMBOL])         # no opa_bias_act for the stem
    assert on[0][1][12] == options.get('input_conv_stride', 2) and on[0][1][13] == 1      # its stride; the ReLU inside
    assert on[0][1][6] == fused.stem7x7_bf16_weight_of(net.input_block[0], net.fb0)[1].data_ptr()    # the folded bias, upcast
    if pool:                                                                              # the pool of what the kernel wrote: no bias, no ReLU
        args = on[1][1]
        assert args[1] is None and args[-1] == 0 and args[4:8] == ((2, 9, 7, 64) if 'input_conv_stride' in options else (2, 5, 4, 64))
    # the switch off: the launches are what they were -- torch's convolution, then the epilogue pass or the pool with the bias
    out_off, off = _stem_launches(trace, net, x, False)
    assert tuple(out_off.shape) == tuple(out.shape) and SYMBOL not in [s for s, _ in off]
    if layout != 'cl':                                                                    # (torch's output follows the input's layout; the passes theirs)
        return
    if pool:
        (symbol, args), = off
        assert symbol == 'opa_maxpool3x3_bias_act' and args[1] == net.fb0.data_ptr() and args[-1] == 1
    else:
        (symbol, args), = off
        assert symbol == 'opa_bias_act' and args[1] == net.fb0.data_ptr()


def test_the_whole_bfloat16_network_launches_the_stem_once(trace):
    net, x = _resnet18(), _x(hw=(33, 17))
    launches = {}
    for on in (True, False):
        fused.STEM7_BF16 = on
        del trace[:]
        with torch.no_grad():
            net(x)
        launches[on] = [s for s, _ in trace]
    assert launches[True][0] == SYMBOL and launches[True].count(SYMBOL) == 1
    assert launches[False][0] == 'opa_bias_act' and SYMBOL not in launches[False]
    assert launches[True][1:] == launches[False][1:] and len(launches[True]) > 1          # nothing behind the stem moved


def test_a_float32_network_never_takes_the_route(trace):
    for options in ({}, {'pool0_stride': 2}, {'input_conv_stride': 1}):
        net = _resnet18(torch.float32, **options)
        _, launches = _stem_launches(trace, net, _x(dtype=torch.float32), True)
        assert SYMBOL not in [s for s, _ in launches]
    net = _resnet18()                                                                     # bfloat16 weights under autocast: declined too
    with pytest.MonkeyPatch.context() as m:
        m.setattr(torch, 'is_autocast_enabled', lambda *a: True)
        _, launches = _stem_launches(trace, net, _x(), True)
    assert SYMBOL not in [s for s, _ in launches]


def test_the_switch_is_read_once_and_ships_off():
    code = 'from openpifpaf_amd import fused; print(int(fused.STEM7_BF16))'
    for env, want in (({}, '0'), ({'OPA_STEM7_BF16': '1'}, '1'), ({'OPA_STEM7_BF16': '0'}, '0')):
        clean = {k: v for k, v in os.environ.items() if k != 'OPA_STEM7_BF16'}
        proc = subprocess.run([sys.executable, '-c', code], env=dict(clean, **env), cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert proc.returncode == 0 and proc.stdout.split('\n')[-2] == want, (env, proc.stdout[-500:], proc.stderr[-500:])


def test_the_header_the_binding_and_the_library_agree():
    with open(os.path.join(ROOT, 'include', 'openpifpaf_amd.h')) as f:
        header = f.read()
    assert SYMBOL + '(' in header and SYMBOL in _lib.SYMBOLS and hasattr(_lib.lib(), SYMBOL)
    declaration = header.split('int ' + SYMBOL + '(')[1].split(');')[0]
    assert len(declaration.split(',')) == 15                                             # 14 arguments and the stream
    assert len(_lib.SYMBOLS[SYMBOL][1]) == 15
    assert '#define OPA_ABI_VERSION 9' in header.replace('  ', ' ')
