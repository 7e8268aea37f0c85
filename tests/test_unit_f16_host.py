"""The float16 ShuffleNetV2K routes on the host: the switch ``fused.UNIT_F16`` (OPA_UNIT_F16), the float16 unit mode
(``fused.UNIT_MODE_F16``: ``opa_gemm_unit_actp_f16``), what ``unit_conv_supported`` and ``dwconv_supported`` answer for float16 operands --
and that they answer for float32 and bfloat16 operands what they answered, whatever ``UNIT_F16`` says --, the derived operands, and the
launches of a whole ``shufflenetv2k16`` cast with ``.half()``, traced on the CPU with the recorder technique of
``test_unit_route_trace.py`` (a recorder in place of ``fused._launch``, tensors that say they are on the GPU, the library reported as
built) and a forward hook on every ``nn.Conv2d`` that records ``miopen:<module name>`` (``test_f16_host.py``).  No GPU is touched and
nothing is timed.

Every test sets ``fused.UNIT_F16`` through monkeypatch, which refuses to set an attribute that does not exist: without the feature
every test of this file fails."""
import copy
import hashlib
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
F16, BF, F32 = torch.float16, torch.bfloat16, torch.float32
GEMM, STENCIL = 'opa_gemm_unit_actp_f16', 'opa_dwconv_actp_f16'


class _OnDevice(torch.Tensor):
    is_cuda = True


def _t(channels=24, dtype=F16, hw=(9, 7)):
    return torch.zeros((2, channels) + hw, dtype=dtype).contiguous(memory_format=CL).as_subclass(_OnDevice)


def _conv(k=24, n=40, bias=True, dtype=F16):
    return nn.Conv2d(k, n, 1, bias=bias).to(dtype).requires_grad_(False)


@pytest.fixture
def on(monkeypatch):
    """``UNIT_F16`` on, every other switch of the unit routes as it ships, the library reported as built."""
    monkeypatch.setattr(fused, 'UNIT_F16', True)
    for name, value in (('UNIT_BF16', False), ('UNIT_LEAKY', False), ('F16', False), ('HEAD16', False), ('X3_UNIT', True), ('X3_TERMS', 6)):
        monkeypatch.setattr(fused, name, value)
    monkeypatch.setattr(_lib, 'available', lambda: True)
    return monkeypatch


# ---- the mode and the switch -----------------------------------------------------------------------------------------------------------

def test_the_mode_of_a_float16_tensor(on):
    mode = fused.unit_mode_of(_t())
    assert mode is fused.UNIT_MODE_F16 and mode.dtype == F16 and mode.align == 4 and mode.gemm == 'conv1x1_unit_f16'
    assert mode.table is False and mode.head() is True and mode.declines_autocast is True and mode.enabled() is True
    assert mode.cache not in (fused.UNIT_MODE_BF16.cache, fused.UNIT_MODE_X3.cache)
    on.setattr(fused, 'UNIT_F16', False)
    assert mode.enabled() is False and fused.unit_mode_of(_t()) is mode
    assert fused.unit_mode_of(_t(dtype=BF)) is fused.UNIT_MODE_BF16 and fused.unit_mode_of(_t(dtype=F32)) is fused.UNIT_MODE_X3
    assert fused.unit_mode_of(_t(dtype=torch.float64)) is None
    # the launcher hands the operands to the float16 symbol, with the code and the parameter and no terms
    calls = []
    on.setattr(fused, '_launch', lambda symbol, *args: calls.append((symbol, args)))
    mode.launch(('a', 1, 'w'), 3, 0.25, None)
    assert calls == [(GEMM, ('a', 1, 'w', 3, 0.25))]


def test_the_switch_reads_opa_unit_f16_and_ships_off():
    code = 'from openpifpaf_amd import fused; print(fused.UNIT_F16, fused.UNIT_BF16, fused.F16, fused.HEAD16, fused.UNIT_LEAKY)'
    env = {k: v for k, v in os.environ.items() if not k.startswith('OPA_')}
    for value, want in ((None, 'False False False False False'), ('1', 'True False False False False'), ('0', 'False False False False False')):
        e = dict(env, **({} if value is None else {'OPA_UNIT_F16': value}))
        out = subprocess.run([sys.executable, '-c', code], env=e, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and out.stdout.strip().split('\n')[-1] == want, (value, out.stdout, out.stderr[-2000:])


def test_the_header_the_binding_and_the_library_agree():
    with open(os.path.join(ROOT, 'include', 'openpifpaf_amd.h')) as f:
        header = f.read()
    for symbol, arguments in ((GEMM, 15), (STENCIL, 16)):              # (the stream included; the stencil's twin has no dtype)
        assert symbol + '(' in header and symbol in _lib.SYMBOLS and hasattr(_lib.lib(), symbol)
        assert len(_lib.SYMBOLS[symbol][1]) == arguments
    assert _lib.SYMBOLS[GEMM] == _lib.SYMBOLS['opa_gemm_unit_actp_bf16']
    actp = _lib.SYMBOLS['opa_dwconv_actp'][1]
    assert _lib.SYMBOLS[STENCIL][1] == actp[:13] + actp[14:]          # opa_dwconv_actp's list without ``dtype``


# ---- the predicates ----------------------------------------------------------------------------------------------------------------------

def test_with_the_switch_off_float16_is_declined(on):
    conv, x = _conv(), _t()
    with torch.no_grad():
        assert fused.unit_conv_supported(conv, x) and fused.unit_conv_f16_supported(conv, x)
        assert fused.dwconv_supported(x, 5, 1) and fused.dwconv_supported(x, 3, 2) and fused.dwconv_supported(x, 7, 1, 4)
        on.setattr(fused, 'UNIT_F16', False)
        assert not fused.unit_conv_supported(conv, x) and not fused.unit_conv_f16_supported(conv, x)
        assert not fused.unit_conv_supported(conv, x, head=True)
        assert not fused.dwconv_supported(x, 5, 1) and not fused.dwconv_supported(x, 3, 2) and not fused.dwconv_supported(x, 7, 1, 4)
        for other in ('UNIT_BF16', 'UNIT_LEAKY', 'F16', 'HEAD16'):       # ... whatever the other switches say
            on.setattr(fused, other, True)
        assert not fused.unit_conv_supported(conv, x) and not fused.dwconv_supported(x, 5, 1)
        on.setattr(fused, 'UNIT_F16', True)
        assert fused.unit_conv_supported(conv, x) and fused.dwconv_supported(x, 5, 1)
        for other in ('UNIT_BF16', 'UNIT_LEAKY', 'F16', 'HEAD16'):       # ... and needs none of them
            on.setattr(fused, other, False)
        assert fused.unit_conv_supported(conv, x, head=True) and fused.dwconv_supported(x, 5, 1)


def _predicate_answers():
    """What every predicate answers for float32 and bfloat16 operands, as one list."""
    out = []
    for dt in (F32, BF):
        conv, x = _conv(dtype=dt), _t(dtype=dt)
        cases = [(conv, x, {}), (conv, _t(48, dt)[:, 24:], {}), (_conv(174, 40, dtype=dt), _t(348, dt)[:, 174:], {}),
                 (conv, x, dict(partner=_t(80, dt)[:, 40:])), (conv, x, dict(residual=_t(40, dt))), (conv, x, dict(head=True)),
                 (conv, _t(26, dt)[:, 1:25], {}), (_conv(23, 40, dtype=dt), _t(23, dt), {}),
                 (_conv(dtype=F16), x, {}), (conv, x, dict(partner=_t(40, F16)))]     # (mixed: a float16 weight, a float16 partner)
        for c, t, kw in cases:
            out.append(bool(fused.unit_conv_supported(c, t, **kw)))
            out.append(bool(fused.unit_conv_bf16_supported(c, t, **{k: v for k, v in kw.items() if k != 'head'})))
            out.append(bool(fused.unit_conv_x3_supported(c, t, **{k: v for k, v in kw.items() if k != 'head'})))
        for k, s, d in ((5, 1, 1), (3, 2, 1), (7, 1, 2), (5, 2, 2), (9, 1, 1)):
            out.append(bool(fused.dwconv_supported(x, k, s, d)))
            out.append(bool(fused.dwconv_supported(x.requires_grad_(False), k, s, d)))
        out.append(fused.unit_mode_of(x).gemm)
    return out


@pytest.mark.parametrize('unit_bf16', [False, True])
def test_float32_and_bfloat16_answer_as_without_the_switch(on, unit_bf16):
    """Every predicate, for float32 and bfloat16 operands, with ``UNIT_F16`` on and off: the answers it gives with the attribute
    REMOVED from the module (the parent commit's module had none), under grad mode, no grad and autocast."""
    on.setattr(fused, 'UNIT_BF16', unit_bf16)
    for autocast in (False, True):
        with on.context() as m:
            if autocast:
                m.setattr(torch, 'is_autocast_enabled', lambda *a: True)
            with m.context() as unset:
                unset.delattr(fused, 'UNIT_F16')
                with torch.no_grad():
                    want = _predicate_answers()
            assert any(want) and not all(v for v in want if isinstance(v, bool))
            for value in (False, True):
                m.setattr(fused, 'UNIT_F16', value)
                with torch.no_grad():
                    assert _predicate_answers() == want, (autocast, value)
                with torch.enable_grad():
                    assert _predicate_answers() == want, (autocast, value)


def test_what_spoils_a_float16_case(on):
    """The base case first, so that the declines below show something; then every reason on its own."""
    conv = _conv()
    with torch.no_grad():
        assert fused.unit_conv_supported(conv, _t())
        assert fused.unit_conv_supported(conv, _t(48)[:, 24:])                                 # a channel slice, 48 bytes in
        assert fused.unit_conv_supported(_conv(174, 40), _t(348)[:, 174:])                     # k16's: 348 bytes in, a 4-byte boundary only
        assert fused.unit_conv_supported(conv, _t(), partner=_t(80)[:, 40:]) and fused.unit_conv_supported(conv, _t(), residual=_t(40))
        spoilt = {
            'odd K': (_conv(23, 40), _t(23), {}),
            'odd N': (_conv(24, 41), _t(), {}),
            'an alignment of 2 bytes only': (conv, _t(26)[:, 1:25], {}),
            'an odd pitch': (conv, _t(25)[:, :24], {}),
            'a bfloat16 weight with a float16 x': (_conv(dtype=BF), _t(), {}),
            'a float32 weight with a float16 x': (_conv(dtype=F32), _t(), {}),
            'a bfloat16 x with a float16 weight': (conv, _t(dtype=BF), {}),
            'a partner and a residual together': (conv, _t(), dict(partner=_t(40), residual=_t(40))),
            'a bfloat16 partner': (conv, _t(), dict(partner=_t(40, BF))),
            'a float32 residual': (conv, _t(), dict(residual=_t(40, F32))),
            'a partner on a 2-byte boundary': (conv, _t(), dict(partner=_t(42)[:, 1:41])),
            'a residual of other pixels': (conv, _t(), dict(residual=_t(40, hw=(9, 8)))),
            'a partner of other channels': (conv, _t(), dict(partner=_t(24))),
            'other input channels': (conv, _t(32), {}),
            'a CPU tensor': (conv, torch.zeros(2, 24, 9, 7, dtype=F16).contiguous(memory_format=CL), {}),
            'NCHW': (conv, torch.zeros(2, 24, 9, 7, dtype=F16).as_subclass(_OnDevice), {}),
            'no pixels': (conv, torch.zeros(2, 24, 0, 7, dtype=F16).as_subclass(_OnDevice), {}),
            'a 3x3 convolution': (nn.Conv2d(24, 40, 3, padding=1).half(), _t(), {}),
            'a strided convolution': (nn.Conv2d(24, 40, 1, stride=2).half(), _t(), {}),
            'groups': (nn.Conv2d(24, 40, 1, groups=2).half(), _t(), {}),
        }
        for what, (c, x, kw) in spoilt.items():
            assert not fused.unit_conv_supported(c, x, **kw), what
            assert not fused.unit_conv_f16_supported(c, x, **kw), what
        with on.context() as m:
            m.setattr(torch, 'is_autocast_enabled', lambda *a: True)
            assert not fused.unit_conv_supported(conv, _t()) and not fused.dwconv_supported(_t(), 5, 1)
        assert fused.unit_conv_supported(conv, _t()) and fused.dwconv_supported(_t(), 5, 1)
    # an operand that autograd follows
    assert not fused.unit_conv_supported(conv, _t().requires_grad_())
    assert not fused.unit_conv_supported(conv, _t(), partner=_t(40).requires_grad_())
    assert not fused.unit_conv_supported(conv, _t(), residual=_t(40).requires_grad_())
    assert not fused.dwconv_supported(_t().requires_grad_(), 5, 1)
    # the stencil's own limits hold for float16 too
    assert not fused.dwconv_supported(_t(), 9, 1) and not fused.dwconv_supported(_t(), 5, 2, 2) and not fused.dwconv_supported(_t(), 5, 3)
    assert not fused.dwconv_supported(torch.zeros(2, 24, 9, 7, dtype=F16).contiguous(memory_format=CL), 5, 1)         # a CPU tensor
    on.setattr(_lib, 'available', lambda: False)
    assert not fused.dwconv_supported(_t(), 5, 1)


def test_a_unit_declines_mixed_16_bit_operands(on):
    """A float16 unit on a bfloat16 activation, and the other way round, takes no kernel of either type: torch raises on the mixed
    convolution, and nothing was launched before it did."""
    symbols = []
    on.setattr(fused, '_launch', lambda symbol, *args: symbols.append(symbol))
    on.setattr(fused, 'UNIT_BF16', True)
    unit = network._InvertedResidualK(24, 24, False)
    network.optimize_for_inference_(unit.eval())
    for module_dtype, x_dtype in ((F16, BF), (BF, F16)):
        unit.to(module_dtype)
        x = _t(24, x_dtype)
        assert not unit._unit_route_supported(x)
        with torch.no_grad(), pytest.raises(RuntimeError):
            unit(x)
        assert not symbols


# ---- the derived operands ------------------------------------------------------------------------------------------------------------------

def test_the_weight_is_padded_and_the_bias_upcast(on):
    torch.manual_seed(1)
    conv = _conv(174, 58)
    wp, bp = fused._unit_weight_f16_of(conv)
    assert wp.dtype == F16 and tuple(wp.shape) == (64, 192) and wp.is_contiguous() and bp.dtype == F32 and tuple(bp.shape) == (64,)
    assert torch.equal(wp[:58, :174], conv.weight.view(58, 174)) and not wp[58:].any() and not wp[:, 174:].any()
    assert torch.equal(bp[:58], conv.bias.float()) and not bp[58:].any()                 # (float16 -> float32 is exact)
    assert fused._unit_weight_f16_of(conv)[0] is wp                                        # kept on the module
    assert getattr(conv, fused.UNIT_MODE_F16.cache) is not None and not hasattr(conv, fused.UNIT_MODE_BF16.cache)
    wq, bq = fused._unit_weight_f16_of(_conv(64, 128, bias=False))
    assert tuple(wq.shape) == (128, 64) and tuple(bq.shape) == (128,) and not bq.any()     # multiples of 64: no padding; no bias: zeros


def test_the_operands_are_derived_again_when_the_parameters_change(on):
    torch.manual_seed(2)
    conv = _conv(24, 40)
    wp, bp = fused._unit_weight_f16_of(conv)
    wp_0, bp_0 = wp.clone(), bp.clone()
    state = {k: torch.randn_like(v) for k, v in conv.state_dict().items()}
    conv.load_state_dict(state)                                                           # (in place: the version counters move)
    wp2, bp2 = fused._unit_weight_f16_of(conv)
    # (the pointers stayed: the KEPT tensors are overwritten in place -- an address a HIP graph holds sees the new weights)
    assert wp2 is wp and bp2 is bp and torch.equal(wp2[:40, :24], state['weight'].view(40, 24)) and torch.equal(bp2[:40], state['bias'].float())
    assert not torch.equal(wp2, wp_0) and not torch.equal(bp2, bp_0)
    wp_2, bp_2 = wp2.clone(), bp2.clone()
    with torch.no_grad():
        conv.weight.mul_(2.0)                                                             # changed in place
    wp3, _ = fused._unit_weight_f16_of(conv)
    assert wp3 is wp2 and torch.equal(wp3, wp_2 * 2)
    conv.half().float().half()                                                            # a round trip through float32: new tensors of equal values
    wp4, bp4 = fused._unit_weight_f16_of(conv)
    assert wp4 is not wp3 and wp4.dtype == F16 and torch.equal(wp4, wp3) and torch.equal(bp4, bp_2)
    conv.weight = nn.Parameter(torch.ones(40, 24, 1, 1, dtype=F16), requires_grad=False)  # the weight REPLACED
    assert torch.equal(fused._unit_weight_f16_of(conv)[0][:40, :24], torch.ones(40, 24, dtype=F16))
    conv.bias = nn.Parameter(torch.ones(40, dtype=F16), requires_grad=False)              # a bias REPLACED: the key holds it
    assert torch.equal(fused._unit_weight_f16_of(conv)[1][:40], torch.ones(40))
    conv.bias = None
    assert not fused._unit_weight_f16_of(conv)[1].any()
    # cast to bfloat16: the bfloat16 mode derives its own, under its own attribute
    conv.to(BF)
    wb, _ = fused._unit_weight_bf16_of(conv)
    assert wb.dtype == BF and getattr(conv, fused.UNIT_MODE_BF16.cache) is not None


# ---- the launches of a whole network ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def k16():
    """``network.factory('shufflenetv2k16')`` with random batch-norm statistics, optimized, float32: the tests cast deep copies."""
    net = network.factory('shufflenetv2k16')
    tc.randomize_(net, 5)
    return network.optimize_for_inference_(net)


@pytest.fixture
def traced(on):
    """-> (trace, run(net, x) -> the trace of one forward): a recorder in place of ``fused._launch``, outputs that say they are on
    the GPU, a hook on every convolution."""
    trace, full = [], []

    def record(symbol, *args):
        trace.append(symbol)
        full.append('%s(%s)' % (symbol, ', '.join(map(str, args))) if args else symbol)
    on.setattr(fused, '_launch', record)
    on.setattr(fused, '_ptr', lambda t: 'null' if t is None else 'ptr')
    empty = fused._empty_nhwc
    on.setattr(fused, '_empty_nhwc', lambda *a, **kw: empty(*a, **kw).zero_().as_subclass(_OnDevice))

    class Stream:
        cuda_stream = 0x7F00DEAD0040
    on.setattr(torch.cuda, 'current_stream', lambda *a: Stream())
    for name, value in (('X3_HEAD', True), ('STEM', False), ('GN', False), ('_CHOICE', {}), ('FORCE_PICK', 'x3')):
        on.setattr(fused, name, value)

    def run(net, x, arguments=False):
        """-> the launched symbols and ``miopen:<module>`` entries of one forward, in order (``arguments``: each launch with its arguments)"""
        hooks = [m.register_forward_hook(lambda mod, args, out, name=name: record('miopen:' + name))
                 for name, m in net.named_modules() if isinstance(m, nn.Conv2d)]
        del trace[:], full[:]
        try:
            with torch.no_grad():
                net(x)
        finally:
            for h in hooks:
                h.remove()
        return list(full if arguments else trace)
    return trace, run


def _x(dtype):
    return torch.randn((1, 3, 33, 25), generator=tc.gen(7)).to(dtype).contiguous(memory_format=CL).as_subclass(_OnDevice)


def _tree(net):
    """(1x1 convolutions of the stages, depthwise convolutions, conv5, the heads' convolutions) from the module tree."""
    base = net.base_net
    stages = [m for stage in (base.stage2, base.stage3, base.stage4) for m in stage.modules() if isinstance(m, nn.Conv2d)]
    pointwise = [m for m in stages if m.kernel_size == (1, 1) and m.groups == 1]
    depthwise = [m for m in stages if m.groups > 1]
    assert len(pointwise) + len(depthwise) == len(stages)
    return pointwise, depthwise, base.conv5[0], [h.conv for h in net.head_nets]


def test_the_half_network_launches_the_float16_symbols(k16, traced):
    """35 + 1 + 2 launches of the GEMM (the units: three in a stage's first, two in every other; conv5; both heads, whose 1392 input
    channels are no multiple of 64), 19 of the stencil, no interleave pass (the shuffled store is the GEMM's), no symbol of another
    element type, and the stem the only convolution that reaches torch."""
    trace, run = traced
    net = copy.deepcopy(k16).half()
    pointwise, depthwise, conv5, heads = _tree(net)
    assert (len(pointwise), len(depthwise), len(heads)) == (35, 19, 2) and isinstance(conv5, nn.Conv2d)
    assert all(h.in_channels == 1392 for h in heads)
    got = run(net, _x(F16))
    assert got.count(GEMM) == len(pointwise) + 1 + len(heads) == 38 and got.count(STENCIL) == len(depthwise) == 19
    assert 'opa_channel_interleave' not in got
    assert [s for s in got if s.startswith('miopen:')] == ['miopen:base_net.input_block.0']
    assert set(got) <= {GEMM, STENCIL, 'opa_head_epilogue', 'opa_bias_act', 'miopen:base_net.input_block.0'}, set(got)
    assert not [s for s in got if 'bf16' in s or 'f32' in s or s in ('opa_dwconv_act', 'opa_dwconv_actp', 'opa_dwconv_dilated_act')]
    assert got.count('opa_head_epilogue') == 2
    # a unit: GEMM, stencil, GEMM; a stage's first: stencil, GEMM, GEMM, stencil, GEMM
    kernels = [s for s in got if s in (GEMM, STENCIL)]
    assert kernels[:5] == [STENCIL, GEMM, GEMM, STENCIL, GEMM] and kernels[5:8] == [GEMM, STENCIL, GEMM]
    assert kernels[-3:] == [GEMM, GEMM, GEMM]                                             # conv5 and the heads


# sha256 of '\n'.join(trace) -- every launch with its arguments, every convolution that reaches torch -- of the ``.half()`` network of the
# ``k16`` fixture on ``_x(F16)`` with ``UNIT_F16`` off, recorded ON THE PARENT COMMIT with this file's ``traced`` fixture (which names no
# ``UNIT_F16`` there); (entries of the trace, of them ``miopen:``)
PARENT_HALF_TRACE = ('70e9efb9634bf2860e13d75e20c9e6ea011ed838fb4809011360506eea26c442', 76, 58)


def test_the_half_network_with_the_switch_off_launches_neither(k16, traced, on):
    """``UNIT_F16`` off -- whatever the bfloat16 and the other float16 switches say: neither new symbol, every convolution with torch,
    the interleave pass per unit as before; launch for launch and argument for argument the parent commit's trace (its digest above)."""
    trace, run = traced
    net = copy.deepcopy(k16).half()
    pointwise, depthwise, conv5, heads = _tree(net)
    on.setattr(fused, 'UNIT_F16', False)
    traces = []
    for others in (False, True):
        for name in ('UNIT_BF16', 'UNIT_LEAKY', 'F16'):
            on.setattr(fused, name, others)
        got = run(net, _x(F16))
        assert GEMM not in got and STENCIL not in got and not [s for s in got if s.startswith('opa_gemm') or s.startswith('opa_dwconv')]
        assert len([s for s in got if s.startswith('miopen:')]) == 1 + len(pointwise) + len(depthwise) + 1 + len(heads)
        assert got.count('opa_channel_interleave') == 16
        traces.append(got)
        off = run(net, _x(F16), arguments=True)
        digest, entries, miopen = PARENT_HALF_TRACE
        assert (len(off), len([s for s in off if s.startswith('miopen:')])) == (entries, miopen)
        assert hashlib.sha256('\n'.join(off).encode()).hexdigest() == digest
    assert traces[0] == traces[1]


def test_the_other_dtypes_trace_the_same_with_the_switch_on_and_off(k16, traced, on):
    trace, run = traced
    for dtype, unit_bf16 in ((F32, False), (BF, False), (BF, True)):
        on.setattr(fused, 'UNIT_BF16', unit_bf16)
        net, x = copy.deepcopy(k16).to(dtype), _x(dtype)
        on.setattr(fused, 'UNIT_F16', False)
        off = run(net, x)
        on.setattr(fused, 'UNIT_F16', True)
        assert run(net, x) == off and off and GEMM not in off and STENCIL not in off
        if dtype == BF:
            assert ('opa_gemm_unit_actp_bf16' in off) == unit_bf16


def test_a_leaky_relu_unit_and_conv5_need_unit_leaky(traced, on):
    """A LeakyReLU network takes the float16 GEMM only where ``UNIT_LEAKY`` is on too (the slope in the GEMM's epilogue); ShuffleNetV2
    x1 (3 x 3 windows) takes both kernels like the K networks."""
    trace, run = traced
    tiny = ([2, 1, 1], [24, 116, 64, 256, 24])
    torch.manual_seed(5)
    leaky = network.optimize_for_inference_(tc.randomize_(network.ShuffleNetV2K('tiny', config=tiny, leaky_relu=True), 5)).half()
    for unit_leaky in (False, True):
        on.setattr(fused, 'UNIT_LEAKY', unit_leaky)
        got = run(leaky, _x(F16))
        assert got.count(GEMM) == ((3 * 3 + 2 + 1) if unit_leaky else 0), (unit_leaky, got)
    on.setattr(fused, 'UNIT_LEAKY', False)
    torch.manual_seed(5)
    x1 = network.optimize_for_inference_(tc.randomize_(network.BASE_FACTORIES['shufflenetv2x1'](), 5)).half()
    convs = [m for stage in (x1.stage2, x1.stage3, x1.stage4) for m in stage.modules() if isinstance(m, nn.Conv2d)]
    got = run(x1, _x(F16))
    assert got.count(GEMM) == len([m for m in convs if m.groups == 1]) + 1 and got.count(STENCIL) == len([m for m in convs if m.groups > 1])
    assert [s for s in got if s.startswith('miopen:')] == ['miopen:conv1.0'] and 'opa_channel_interleave' not in got
