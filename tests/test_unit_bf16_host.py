"""Host side of the bf16 unit-mode GEMM route (``fused.UNIT_BF16``, ``fused.conv1x1_unit_bf16``, csrc/gemm_unit_bf16.hip): the derived
operands, what ``unit_conv_bf16_supported`` declines, and which launches a ShuffleNetV2K cast to bfloat16 makes with the switch off and
on -- traced on the CPU with a recorder in place of ``fused._launch`` and tensors that say they are on the GPU.  No GPU is touched."""
import copy
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
SYMBOL = 'opa_gemm_unit_actp_bf16'
TINY = ([2, 1, 1], [24, 116, 64, 256, 24])


class _OnDevice(torch.Tensor):
    is_cuda = True


def _t(channels=24, dtype=BF16, hw=(9, 7)):
    return torch.zeros((2, channels) + hw, dtype=dtype).contiguous(memory_format=CL).as_subclass(_OnDevice)


def _conv(k=24, n=40, bias=True, dtype=BF16):
    return nn.Conv2d(k, n, 1, bias=bias).to(dtype).requires_grad_(False)


# ---- the derived operands -----------------------------------------------------------------------------------------------------------

def test_the_weight_is_padded_and_the_bias_upcast():
    torch.manual_seed(1)
    conv = _conv(174, 58)
    wp, bp = fused._unit_weight_bf16_of(conv)
    assert wp.dtype == BF16 and tuple(wp.shape) == (64, 192) and wp.is_contiguous() and bp.dtype == torch.float32 and tuple(bp.shape) == (64,)
    assert torch.equal(wp[:58, :174], conv.weight.view(58, 174)) and not wp[58:].any() and not wp[:, 174:].any()
    assert torch.equal(bp[:58], conv.bias.float()) and not bp[58:].any()                 # (bf16 -> float32 is exact)
    assert fused._unit_weight_bf16_of(conv)[0] is wp                                       # kept on the module
    wq, bq = fused._unit_weight_bf16_of(_conv(64, 128, bias=False))
    assert tuple(wq.shape) == (128, 64) and tuple(bq.shape) == (128,) and not bq.any()     # multiples of 64: no padding; no bias: zeros


def test_the_operands_are_derived_again_when_the_parameters_change():
    torch.manual_seed(2)
    conv = _conv(24, 40)
    wp, bp = fused._unit_weight_bf16_of(conv)
    wp_0, bp_0 = wp.clone(), bp.clone()
    state = {k: torch.randn_like(v) for k, v in conv.state_dict().items()}
    conv.load_state_dict(state)                                                           # (in place: the version counters move)
    wp2, bp2 = fused._unit_weight_bf16_of(conv)
    # (the pointers stayed: the KEPT tensors are overwritten in place -- an address a HIP graph holds sees the new weights)
    assert wp2 is wp and bp2 is bp and torch.equal(wp2[:40, :24], state['weight'].view(40, 24)) and torch.equal(bp2[:40], state['bias'].float())
    assert not torch.equal(wp2, wp_0) and not torch.equal(bp2, bp_0)
    conv.bias = nn.Parameter(torch.ones(40, dtype=BF16), requires_grad=False)             # a bias REPLACED: the key holds it
    assert torch.equal(fused._unit_weight_bf16_of(conv)[1][:40], torch.ones(40))
    conv.bias = None
    assert not fused._unit_weight_bf16_of(conv)[1].any()


# ---- unit_conv_bf16_supported ----------------------------------------------------------------------------------------------------------

def test_supported_declines(monkeypatch):
    """Every reason on its own; the base case first, so that the declines below show something."""
    monkeypatch.setattr(fused, 'UNIT_BF16', True)
    conv = _conv()
    with torch.no_grad():
        assert fused.unit_conv_bf16_supported(conv, _t())
        assert fused.unit_conv_bf16_supported(conv, _t(48)[:, 24:])                        # a channel slice, 48 bytes in
        assert fused.unit_conv_bf16_supported(_conv(174, 40), _t(348)[:, 174:])            # k16's: 348 bytes in, a 4-byte boundary only
        assert fused.unit_conv_bf16_supported(conv, _t(), partner=_t(80)[:, 40:]) and fused.unit_conv_bf16_supported(conv, _t(), residual=_t(40))
        # the switch, the device, the dtypes, autocast
        with monkeypatch.context() as m:
            m.setattr(fused, 'UNIT_BF16', False)
            assert not fused.unit_conv_bf16_supported(conv, _t())
        assert not fused.unit_conv_bf16_supported(conv, torch.zeros(2, 24, 9, 7, dtype=BF16).contiguous(memory_format=CL))   # a CPU tensor
        assert not fused.unit_conv_bf16_supported(_conv(dtype=torch.float32), _t(dtype=torch.float32))
        assert not fused.unit_conv_bf16_supported(_conv(dtype=torch.float32), _t())        # autocast's pairing: float32 parameters
        assert not fused.unit_conv_bf16_supported(conv, _t(dtype=torch.float32))
        assert not fused.unit_conv_bf16_supported(conv, _t(dtype=torch.float16))
        with monkeypatch.context() as m:
            m.setattr(torch, 'is_autocast_enabled', lambda *a: True)
            assert not fused.unit_conv_bf16_supported(conv, _t())
        # odd channel counts
        assert not fused.unit_conv_bf16_supported(_conv(23, 40), _t(23)) and not fused.unit_conv_bf16_supported(_conv(24, 41), _t())
        # a view on a 2-byte boundary, an odd pitch, other channels, NCHW, no pixels
        assert not fused.unit_conv_bf16_supported(conv, _t(26)[:, 1:25])
        assert not fused.unit_conv_bf16_supported(conv, _t(25)[:, :24])
        assert not fused.unit_conv_bf16_supported(conv, _t(32))
        assert not fused.unit_conv_bf16_supported(conv, torch.zeros(2, 24, 9, 7, dtype=BF16).as_subclass(_OnDevice))
        assert not fused.unit_conv_bf16_supported(conv, torch.zeros(2, 24, 0, 7, dtype=BF16).as_subclass(_OnDevice))
        # another convolution
        for other in (nn.Conv2d(24, 40, 3, padding=1), nn.Conv2d(24, 40, 1, stride=2), nn.Conv2d(24, 40, 1, groups=2)):
            assert not fused.unit_conv_bf16_supported(other.to(BF16), _t())
        # the third operand: both at once, a 2-byte boundary, other pixels, other channels, float32
        assert not fused.unit_conv_bf16_supported(conv, _t(), partner=_t(40), residual=_t(40))
        assert not fused.unit_conv_bf16_supported(conv, _t(), partner=_t(42)[:, 1:41])
        assert not fused.unit_conv_bf16_supported(conv, _t(), residual=_t(40, hw=(9, 8)))
        assert not fused.unit_conv_bf16_supported(conv, _t(), partner=_t(24))
        assert not fused.unit_conv_bf16_supported(conv, _t(), residual=_t(40, dtype=torch.float32))
    # an operand that autograd follows
    assert not fused.unit_conv_bf16_supported(conv, _t().requires_grad_())
    assert not fused.unit_conv_bf16_supported(conv, _t(), partner=_t(40).requires_grad_())


# ---- the routes -------------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def launches(monkeypatch):
    """A recorder in place of ``fused._launch`` (nothing runs: the outputs hold zeros), outputs that say they are on the GPU like
    their inputs, the library reported as built.  -> the list of launched symbols."""
    symbols = []
    monkeypatch.setattr(fused, '_launch', lambda symbol, *args: symbols.append(symbol))
    empty = fused._empty_nhwc
    monkeypatch.setattr(fused, '_empty_nhwc', lambda *a, **kw: empty(*a, **kw).zero_().as_subclass(_OnDevice))
    monkeypatch.setattr(_lib, 'available', lambda: True)
    return symbols


def _net(leaky=False):
    torch.manual_seed(5)
    net = tc.randomize_(network.ShuffleNetV2K('tiny', config=TINY, leaky_relu=leaky), 5)
    return network.optimize_for_inference_(copy.deepcopy(net)).to(BF16)


def _pointwise(net):
    """The 1x1 convolutions of the stages, and conv5's."""
    stages = [m for stage in (net.stage2, net.stage3, net.stage4) for m in stage.modules()
              if isinstance(m, nn.Conv2d) and m.kernel_size == (1, 1) and m.groups == 1]
    return stages, net.conv5[0]


def _x():
    return torch.randn((2, 3, 33, 25), generator=tc.gen(7)).to(BF16).contiguous(memory_format=CL).as_subclass(_OnDevice)


def test_with_the_switch_off_nothing_launches_the_symbol(launches, monkeypatch):
    assert fused.UNIT_BF16 is False or 'OPA_UNIT_BF16' in os.environ
    monkeypatch.setattr(fused, 'UNIT_BF16', False)
    monkeypatch.setattr(fused, 'UNIT_LEAKY', True)
    for leaky in (False, True):
        net = _net(leaky)
        with torch.no_grad():
            out = net(_x())
        assert out.dtype == BF16 and SYMBOL not in launches
    assert launches and not [s for s in launches if 'unit' in s]                          # the stencil and the interleave, as before


def test_with_the_switch_on_every_pointwise_convolution_launches_it(launches, monkeypatch):
    """One launch per 1x1 convolution of the stages and one for conv5 -- counted from the module tree -- and no interleave pass: the
    shuffled store is the GEMM's.  A LeakyReLU network only where ``UNIT_LEAKY`` is on too; float32 and autocast never."""
    monkeypatch.setattr(fused, 'UNIT_BF16', True)
    net = _net()
    stages, conv5 = _pointwise(net)
    assert len(stages) == 3 * 3 + 2 and isinstance(conv5, nn.Conv2d)                       # (three units first in their stage, one not)
    with torch.no_grad():
        out = net(_x())
    assert tuple(out.shape) == (2, 24, 3, 2) and out.dtype == BF16
    assert launches.count(SYMBOL) == len(stages) + 1 and 'opa_channel_interleave' not in launches
    assert launches[-1] == SYMBOL                                                         # conv5
    # a LeakyReLU network: behind UNIT_LEAKY
    leaky = _net(leaky=True)
    for on in (False, True):
        monkeypatch.setattr(fused, 'UNIT_LEAKY', on)
        del launches[:]
        with torch.no_grad():
            leaky(_x())
        assert launches.count(SYMBOL) == (len(stages) + 1 if on else 0), on
    # float32 keeps its own routes; autocast keeps torch
    del launches[:]
    with torch.no_grad():
        net.float()(_x().float())
    assert SYMBOL not in launches
    monkeypatch.setattr(torch, 'is_autocast_enabled', lambda *a: True)
    del launches[:]
    with torch.no_grad():
        _net()(_x())
    assert SYMBOL not in launches


def test_a_head_with_unaligned_input_channels_launches_it(launches, monkeypatch):
    """``CompositeField4``: K % 64 != 0 takes the bf16 unit mode, K % 64 == 0 stays where it was."""
    from openpifpaf_amd import headmeta
    meta = headmeta.Cif('cif', 'test', keypoints=['a', 'b', 'c'], sigmas=[0.1, 0.1, 0.1], pose=None, draw_skeleton=[])
    meta.upsample_stride = 2                                                              # 3 x 5 x 4 = 60 output channels (an odd count stays with torch)
    for k, want in ((24, 1), (64, 0)):
        head = network.CompositeField4(meta, k).to(BF16).eval()
        for on in (True, False):
            monkeypatch.setattr(fused, 'UNIT_BF16', on)
            del launches[:]
            with torch.no_grad():
                try:
                    head(_t(k, hw=(3, 2)))
                except Exception:                   # noqa: BLE001  (behind the convolution nothing matters here: the epilogue has no device)
                    pass
            assert launches.count(SYMBOL) == (want if on else 0), (k, on, launches)


def test_the_switch_is_read_once_and_ships_off():
    code = 'from openpifpaf_amd import fused; print(int(fused.UNIT_BF16))'
    for env, want in (({}, '0'), ({'OPA_UNIT_BF16': '1'}, '1'), ({'OPA_UNIT_BF16': '0'}, '0')):
        clean = {k: v for k, v in os.environ.items() if k != 'OPA_UNIT_BF16'}
        proc = subprocess.run([sys.executable, '-c', code], env=dict(clean, **env), cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert proc.returncode == 0 and proc.stdout.split('\n')[-2] == want, (env, proc.stdout[-500:], proc.stderr[-500:])


def test_the_header_the_binding_and_the_library_agree():
    with open(os.path.join(ROOT, 'include', 'openpifpaf_amd.h')) as f:
        header = f.read()
    assert SYMBOL + '(' in header and SYMBOL in _lib.SYMBOLS and hasattr(_lib.lib(), SYMBOL)
    assert len(_lib.SYMBOLS[SYMBOL][1]) == 15                                             # 14 arguments and the stream
