"""Host side of the bf16 two-source GEMM route (``fused.PAIR_BF16``, ``fused.conv1x1_pair_bias_act_bf16``,
``fused.conv1x1_strided_bf16``, csrc/gemm2_bf16.hip): the derived operands, and what ``pair_bf16_supported`` and
``conv1x1_strided_bf16_supported`` decline -- every clause flipped alone -- on the CPU with tensors that say they are on the GPU.
No GPU is touched."""
import os
import subprocess
import sys

import torch
from torch import nn

from openpifpaf_amd import _lib, fused, network

import trunk_common as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CL = torch.channels_last
BF16 = torch.bfloat16
SYMBOL = 'opa_gemm2_bias_act_bf16'
K1, K2, N = 64, 128, 256


class _OnDevice(torch.Tensor):
    is_cuda = True


def _t(channels, hw=(9, 7), dtype=BF16, batch=2):
    return torch.zeros((batch, channels) + hw, dtype=dtype).contiguous(memory_format=CL).as_subclass(_OnDevice)


def _conv(c, n=N, stride=1, dtype=BF16, k=1, padding=0, **kw):
    return nn.Conv2d(c, n, k, stride, padding, bias=False, **kw).to(dtype).requires_grad_(False)


def _bias(n=N, dtype=BF16):
    return torch.zeros(n, dtype=dtype)


# ---- the derived operands -----------------------------------------------------------------------------------------------------------

def test_the_weight_is_both_weights_side_by_side_and_the_bias_upcast():
    torch.manual_seed(1)
    conv, dconv, bias = _conv(K1), _conv(K2, stride=2), torch.randn(N).to(BF16)
    wcat, b32 = fused.pair_bf16_weight_of(conv, dconv, bias)
    assert wcat.dtype == BF16 and tuple(wcat.shape) == (N, K1 + K2) and wcat.is_contiguous()
    assert torch.equal(wcat, torch.cat((conv.weight.reshape(N, K1), dconv.weight.reshape(N, K2)), dim=1))
    assert torch.equal(wcat[:, :K1], conv.weight[:, :, 0, 0]) and torch.equal(wcat[:, K1:], dconv.weight[:, :, 0, 0])
    assert b32.dtype == torch.float32 and torch.equal(b32, bias.float()) and b32.is_contiguous()    # (bf16 -> float32 is exact)
    again = fused.pair_bf16_weight_of(conv, dconv, bias)
    assert again[0] is wcat and again[1] is b32                                            # kept on the module
    assert fused.pair_bf16_weight_of(conv, dconv, None)[1] is None                         # no bias: none handed over
    # without ``conv``: the downsampling weight alone
    wd, none = fused.pair_bf16_weight_of(None, dconv, None)
    assert none is None and tuple(wd.shape) == (N, K2) and wd.is_contiguous() and torch.equal(wd, dconv.weight.reshape(N, K2))


def test_the_operands_are_derived_again_when_the_parameters_change():
    torch.manual_seed(2)
    block = network.optimize_for_inference_(tc.bottleneck(128, 64, 2, True, 3)).to(BF16)
    conv, dconv, bias = block.conv3, block.downsample[0], block.fb3
    k1, k2, n = conv.in_channels, dconv.in_channels, conv.out_channels

    def cat(w, wd):
        return torch.cat((w.reshape(n, k1), wd.reshape(n, k2)), dim=1)
    wcat, b32 = fused.pair_bf16_weight_of(conv, dconv, bias)
    wcat_0, b32_0 = wcat.clone(), b32.clone()
    state = {k: torch.randn_like(v) for k, v in block.state_dict().items()}
    block.load_state_dict(state)                                                          # (in place: the version counters move)
    wcat_b, b32_b = fused.pair_bf16_weight_of(conv, dconv, bias)
    # (the pointers stayed: the KEPT tensors are overwritten in place -- an address a HIP graph holds sees the new weights)
    assert wcat_b is wcat and not torch.equal(wcat_b, wcat_0)
    assert torch.equal(wcat_b, cat(state['conv3.weight'], state['downsample.0.weight']))
    assert b32_b is b32 and torch.equal(b32_b, state['fb3'].float()) and not torch.equal(b32_b, b32_0)
    wcat_1 = wcat_b.clone()
    with torch.no_grad():                                                                 # an in-place update of conv3's weight alone
        conv.weight.mul_(2.0)
    wcat_c, b32_c = fused.pair_bf16_weight_of(conv, dconv, bias)
    assert wcat_c is wcat_b and torch.equal(wcat_c[:, :k1], wcat_1[:, :k1] * 2) and torch.equal(wcat_c[:, k1:], wcat_1[:, k1:])
    assert torch.equal(b32_c, state['fb3'].float())
    wcat_2 = wcat_c.clone()
    with torch.no_grad():                                                                 # ... of the downsampling weight alone
        dconv.weight.mul_(0.5)
    wcat_d = fused.pair_bf16_weight_of(conv, dconv, bias)[0]
    assert torch.equal(wcat_d[:, k1:], wcat_2[:, k1:] * 0.5) and torch.equal(wcat_d[:, :k1], wcat_2[:, :k1])
    with torch.no_grad():                                                                 # ... and of the folded bias alone
        bias.add_(1.0)
    assert torch.equal(fused.pair_bf16_weight_of(conv, dconv, bias)[1], bias.float())
    dconv.weight = nn.Parameter(torch.ones_like(dconv.weight), requires_grad=False)       # a weight REPLACED
    assert bool((fused.pair_bf16_weight_of(conv, dconv, bias)[0][:, k1:] == 1).all())
    # the k1 == 0 form follows its weight too
    wd = fused.pair_bf16_weight_of(None, dconv, None)[0].clone()                           # (a dense weight is handed over where it lies)
    with torch.no_grad():
        dconv.weight.mul_(3.0)
    assert torch.equal(fused.pair_bf16_weight_of(None, dconv, None)[0], wd * 3)


# ---- the predicates -----------------------------------------------------------------------------------------------------------------

def test_pair_supported_declines(monkeypatch):
    """Every clause on its own; the base cases first, so that the declines below show something."""
    monkeypatch.setattr(fused, 'PAIR_BF16', True)
    monkeypatch.setattr(_lib, 'available', lambda: True)
    ok = fused.pair_bf16_supported
    conv, dconv, d1 = _conv(K1), _conv(K2, stride=2), _conv(K2)
    h, x, bias, a_bias = _t(K1, (5, 4)), _t(K2), _bias(), _bias(K1)
    with torch.no_grad():
        assert ok(conv, dconv, h, x, bias) and ok(conv, dconv, h, x, None) and ok(conv, dconv, h, x, bias.float())
        assert ok(conv, dconv, h, x, bias, a_bias) and ok(conv, d1, _t(K1), x, bias, a_bias)
        assert ok(_conv(128, 192), _conv(192, 192, 2), _t(128, (5, 4)), _t(192), _bias(192))
        # the switch, the library, the declined keys
        with monkeypatch.context() as m:
            m.setattr(fused, 'PAIR_BF16', False)
            assert not ok(conv, dconv, h, x, bias)
        with monkeypatch.context() as m:
            m.setattr(_lib, 'available', lambda: False)
            assert not ok(conv, dconv, h, x, bias)
        with monkeypatch.context() as m:
            m.setattr(fused, 'PAIR_BF16_DECLINED', frozenset({(K1, K2, N, 2)}))
            assert not ok(conv, dconv, h, x, bias) and ok(conv, d1, _t(K1), x, bias)
        # the device, the dtypes, autocast
        assert not ok(conv, dconv, h, torch.zeros(2, K2, 9, 7, dtype=BF16).contiguous(memory_format=CL), bias)     # a CPU tensor
        assert not ok(conv, dconv, torch.zeros(2, K1, 5, 4, dtype=BF16).contiguous(memory_format=CL), x, bias)
        f32 = torch.float32
        assert not ok(_conv(K1, dtype=f32), _conv(K2, stride=2, dtype=f32), _t(K1, (5, 4), f32), _t(K2, dtype=f32), bias.float())   # float32
        assert not ok(_conv(K1, dtype=f32), dconv, h, x, bias) and not ok(conv, _conv(K2, stride=2, dtype=f32), h, x, bias)  # autocast's pairing
        assert not ok(conv, dconv, _t(K1, (5, 4), f32), x, bias) and not ok(conv, dconv, h, _t(K2, dtype=torch.float16), bias)
        with monkeypatch.context() as m:
            m.setattr(torch, 'is_autocast_enabled', lambda *a: True)
            assert not ok(conv, dconv, h, x, bias)
        # NCHW, a channel slice (not dense), other channels, no pixels, another batch
        assert not ok(conv, dconv, h, torch.zeros(2, K2, 9, 7, dtype=BF16).as_subclass(_OnDevice), bias)
        assert not ok(conv, dconv, torch.zeros(2, K1, 5, 4, dtype=BF16).as_subclass(_OnDevice), x, bias)
        assert not ok(conv, dconv, h, _t(K2 + 64)[:, :K2], bias) and not ok(conv, dconv, _t(K1 + 64, (5, 4))[:, :K1], x, bias)
        assert not ok(conv, dconv, h, _t(K2 + 64), bias) and not ok(conv, dconv, _t(K1 + 64, (5, 4)), x, bias)
        assert not ok(conv, dconv, _t(K1, (0, 4)), _t(K2, (0, 7)), bias)
        assert not ok(conv, dconv, _t(K1, (5, 4), batch=3), x, bias)
        # h's pixels are not x's at the stride
        assert not ok(conv, dconv, _t(K1), x, bias) and not ok(conv, d1, h, x, bias) and not ok(conv, dconv, _t(K1, (5, 3)), x, bias)
        # other convolutions: 3x3, groups, padding, a bias of their own, a strided conv, stride 3, a stride that is not square, other outputs
        assert not ok(_conv(K1, k=3, padding=1), dconv, h, x, bias) and not ok(conv, _conv(K2, stride=2, k=3, padding=1), h, x, bias)
        assert not ok(_conv(K1, groups=2), dconv, h, x, bias) and not ok(conv, _conv(K2, stride=2, groups=2), h, x, bias)
        assert not ok(_conv(K1, padding=1), dconv, _t(K1, (3, 2)), x, bias)
        own = nn.Conv2d(K1, N, 1).to(BF16).requires_grad_(False)
        own_d = nn.Conv2d(K2, N, 1, 2).to(BF16).requires_grad_(False)
        assert not ok(own, dconv, h, x, bias) and not ok(conv, own_d, h, x, bias)
        assert not ok(_conv(K1, stride=2), dconv, h, x, bias)
        assert not ok(conv, _conv(K2, stride=3), _t(K1, (3, 3)), x, bias)
        assert not ok(conv, _conv(K2, stride=(2, 1)), _t(K1, (5, 7)), x, bias)
        assert not ok(conv, _conv(K2, 128, 2), h, x, bias)
        # channel counts that are no multiples of 64
        assert not ok(_conv(32), dconv, _t(32, (5, 4)), x, bias) and not ok(conv, _conv(96, stride=2), h, _t(96), bias)
        assert not ok(_conv(K1, 96), _conv(K2, 96, 2), h, x, _bias(96))
        # the folded bias: another length, another dtype
        assert not ok(conv, dconv, h, x, _bias(64)) and not ok(conv, dconv, h, x, _bias(dtype=torch.float16))
        # a_bias: float32, another length, not contiguous, off a 16-byte boundary
        assert not ok(conv, dconv, h, x, bias, a_bias.float()) and not ok(conv, dconv, h, x, bias, _bias(K1 + 64))
        assert not ok(conv, dconv, h, x, bias, _bias(2 * K1)[::2]) and not ok(conv, dconv, h, x, bias, _bias(K1 + 8)[1:K1 + 1])
        # an operand off a 16-byte boundary
        shifted = torch.zeros(2 * 9 * 7 * K2 + 8, dtype=BF16)[1:-7].view(2, 9, 7, K2).permute(0, 3, 1, 2).as_subclass(_OnDevice)
        assert shifted.is_contiguous(memory_format=CL) and shifted.data_ptr() % 16 != 0 and not ok(conv, dconv, h, shifted, bias)
    # grad enabled and something that autograd follows
    assert ok(conv, dconv, h, x, bias, a_bias)
    assert not ok(conv, dconv, h, _t(K2).requires_grad_(), bias) and not ok(conv, dconv, _t(K1, (5, 4)).requires_grad_(), x, bias)
    assert not ok(_conv(K1).requires_grad_(True), dconv, h, x, bias) and not ok(conv, _conv(K2, stride=2).requires_grad_(True), h, x, bias)
    assert not ok(conv, dconv, h, x, _bias().requires_grad_()) and not ok(conv, dconv, h, x, bias, _bias(K1).requires_grad_())


class _Sized:
    """Stands in for a tensor too large to allocate: a dense channels-last bfloat16 tensor on the GPU of this shape."""
    is_cuda, dtype, requires_grad, device = True, BF16, False, torch.device('cpu')

    def __init__(self, *shape):
        self.shape = torch.Size(shape)

    def dim(self):
        return 4

    def is_contiguous(self, memory_format=None):
        return True

    def data_ptr(self):
        return 4096

    def numel(self):
        return self.shape.numel()


def test_the_size_limits(monkeypatch):
    monkeypatch.setattr(fused, 'PAIR_BF16', True)
    monkeypatch.setattr(_lib, 'available', lambda: True)
    with torch.no_grad():
        conv, dconv = _conv(64, 256), _conv(64, 256)
        assert fused.pair_bf16_supported(conv, dconv, _Sized(2 ** 8, 64, 2 ** 7, 2 ** 6), _Sized(2 ** 8, 64, 2 ** 7, 2 ** 6), None)
        assert fused.conv1x1_strided_bf16_supported(dconv, _Sized(2 ** 8, 64, 2 ** 7, 2 ** 6))
        # x of 2^31 elements
        wide = _conv(256, 64)
        assert not fused.pair_bf16_supported(_conv(64, 64), wide, _Sized(2 ** 8, 64, 2 ** 8, 2 ** 7), _Sized(2 ** 8, 256, 2 ** 8, 2 ** 7), None)
        assert not fused.conv1x1_strided_bf16_supported(wide, _Sized(2 ** 8, 256, 2 ** 8, 2 ** 7))
        # h of 2^31 elements where x and the output have 2^29
        assert not fused.pair_bf16_supported(_conv(256, 64), _conv(64, 64), _Sized(2 ** 8, 256, 2 ** 8, 2 ** 7),
                                             _Sized(2 ** 8, 64, 2 ** 8, 2 ** 7), None)
        # the output of 2^31 elements where x and h have 2^29
        assert not fused.pair_bf16_supported(conv, dconv, _Sized(2 ** 8, 64, 2 ** 8, 2 ** 7), _Sized(2 ** 8, 64, 2 ** 8, 2 ** 7), None)
        assert not fused.conv1x1_strided_bf16_supported(dconv, _Sized(2 ** 8, 64, 2 ** 8, 2 ** 7))


def test_strided_supported_declines(monkeypatch):
    monkeypatch.setattr(fused, 'PAIR_BF16', True)
    monkeypatch.setattr(_lib, 'available', lambda: True)
    ok = fused.conv1x1_strided_bf16_supported
    dconv, x = _conv(K2, stride=2), _t(K2)
    with torch.no_grad():
        assert ok(dconv, x) and ok(_conv(K2), x) and ok(_conv(64, 128, 2), _t(64))
        with monkeypatch.context() as m:
            m.setattr(fused, 'PAIR_BF16', False)
            assert not ok(dconv, x)
        with monkeypatch.context() as m:
            m.setattr(_lib, 'available', lambda: False)
            assert not ok(dconv, x)
        with monkeypatch.context() as m:
            m.setattr(fused, 'PAIR_BF16_DECLINED', frozenset({(0, K2, N, 2)}))
            assert not ok(dconv, x) and ok(_conv(K2), x)
        with monkeypatch.context() as m:
            m.setattr(torch, 'is_autocast_enabled', lambda *a: True)
            assert not ok(dconv, x)
        assert not ok(dconv, torch.zeros(2, K2, 9, 7, dtype=BF16).contiguous(memory_format=CL))                    # a CPU tensor
        assert not ok(_conv(K2, stride=2, dtype=torch.float32), _t(K2, dtype=torch.float32)) and not ok(_conv(K2, stride=2, dtype=torch.float32), x)
        assert not ok(dconv, _t(K2, dtype=torch.float16))
        assert not ok(dconv, torch.zeros(2, K2, 9, 7, dtype=BF16).as_subclass(_OnDevice))                          # NCHW
        assert not ok(dconv, _t(K2 + 64)[:, :K2]) and not ok(dconv, _t(K2 + 64)) and not ok(dconv, _t(K2, (0, 7)))
        assert not ok(_conv(K2, stride=2, k=3, padding=1), x) and not ok(_conv(K2, stride=2, groups=2), x) and not ok(_conv(K2, padding=1), x)
        assert not ok(nn.Conv2d(K2, N, 1, 2).to(BF16).requires_grad_(False), x)
        assert not ok(_conv(K2, stride=3), x) and not ok(_conv(K2, stride=(2, 1)), x)
        assert not ok(_conv(96, stride=2), _t(96)) and not ok(_conv(K2, 96, 2), x)
    assert ok(dconv, x)
    assert not ok(dconv, _t(K2).requires_grad_()) and not ok(_conv(K2, stride=2).requires_grad_(True), x)


# ---- the switch, the header, the binding ---------------------------------------------------------------------------------------------

def test_the_switch_is_read_once_and_ships_off():
    code = 'from openpifpaf_amd import fused; print(int(fused.PAIR_BF16), len(fused.PAIR_BF16_DECLINED))'
    for env, want in (({}, '0'), ({'OPA_PAIR_BF16': '1'}, '1'), ({'OPA_PAIR_BF16': '0'}, '0')):
        clean = {k: v for k, v in os.environ.items() if k != 'OPA_PAIR_BF16'}
        proc = subprocess.run([sys.executable, '-c', code], env=dict(clean, **env), cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert proc.returncode == 0 and proc.stdout.split('\n')[-2].split()[0] == want, (env, proc.stdout[-500:], proc.stderr[-500:])
    assert isinstance(fused.PAIR_BF16_DECLINED, frozenset)
    assert all(len(key) == 4 for key in fused.PAIR_BF16_DECLINED)                          # (k1, k2, n, stride)


def test_the_header_the_binding_and_the_library_agree():
    with open(os.path.join(ROOT, 'include', 'openpifpaf_amd.h')) as f:
        header = f.read()
    assert SYMBOL + '(' in header and SYMBOL in _lib.SYMBOLS and hasattr(_lib.lib(), SYMBOL)
    declaration = header.split('int ' + SYMBOL + '(')[1].split(');')[0]
    assert len(declaration.split(',')) == 15                                             # 14 arguments and the stream
    assert len(_lib.SYMBOLS[SYMBOL][1]) == 15
    assert '#define OPA_ABI_VERSION 9' in header.replace('  ', ' ')
