"""Host side of the float16 grouped 3x3 and 7x7 stem routes (``fused.GCONV_F16`` / ``fused.STEM7_F16``: ``opa_gconv3x3_act_f16`` and
``opa_stem7x7_act_f16`` behind the predicates and launchers their bfloat16 twins have): the switches, every decline reason of both
predicates for float16 operands (the rows of ``test_gconv3x3_bf16_host.py`` / ``test_stem7x7_bf16_host.py``), the bfloat16 answers
whatever the new switches say, the derived operands after ``.bfloat16()`` -> ``.half()`` and ``load_state_dict``, and the launches of a
whole ``resnext50.half()`` and of a ``resnet18.half()`` with the input max-pool -- traced on the CPU by ``test_f16_host.py``'s
technique: a recorder in place of ``fused._launch``, a hook on every ``nn.Conv2d``, tensors that say they are on the GPU.  No GPU is
touched."""
import os
import subprocess
import sys

import pytest
import torch
from torch import nn

from openpifpaf_amd import _lib, fused, network

import test_f16_host as tf
import test_gconv3x3_bf16_host as gh
import test_stem7x7_bf16_host as sh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CL = torch.channels_last
F16, BF, F32 = torch.float16, torch.bfloat16, torch.float32
GCONV, STEM = 'opa_gconv3x3_act_f16', 'opa_stem7x7_act_f16'
BF16_SWITCHES = ('CONV3_BF16', 'PAIR_BF16', 'STEM7_BF16', 'GCONV_BF16', 'UNIT_BF16')
OTHER_F16_SWITCHES = ('F16', 'HEAD16', 'UNIT_F16')
_OnDevice = gh._OnDevice


@pytest.fixture
def on(monkeypatch):
    """The two new switches on -- every other 16-bit switch OFF -- and the library reported as built."""
    monkeypatch.setattr(fused, 'GCONV_F16', True)
    monkeypatch.setattr(fused, 'STEM7_F16', True)
    for name in BF16_SWITCHES + OTHER_F16_SWITCHES:
        monkeypatch.setattr(fused, name, False)
    monkeypatch.setattr(_lib, 'available', lambda: True)
    return monkeypatch


# ---- the switches ---------------------------------------------------------------------------------------------------------------------

def test_the_switches_ship_off_and_read_their_own_variables():
    code = 'from openpifpaf_amd import fused; print(int(fused.GCONV_F16), int(fused.STEM7_F16), int(fused.F16), int(fused.GCONV_BF16))'
    names = ('OPA_GCONV_F16', 'OPA_STEM7_F16', 'OPA_F16', 'OPA_GCONV_BF16', 'OPA_STEM7_BF16')
    clean = {k: v for k, v in os.environ.items() if k not in names}
    for env, want in (({}, '0 0 0 0'), ({'OPA_GCONV_F16': '1'}, '1 0 0 0'), ({'OPA_STEM7_F16': '1'}, '0 1 0 0'),
                      ({'OPA_GCONV_F16': '0', 'OPA_STEM7_F16': '0'}, '0 0 0 0'), ({'OPA_F16': '1'}, '0 0 1 0'),
                      ({'OPA_GCONV_BF16': '1', 'OPA_STEM7_BF16': '1'}, '0 0 0 1'), ({'OPA_GCONV_F16': '1', 'OPA_STEM7_F16': '1'}, '1 1 0 0')):
        proc = subprocess.run([sys.executable, '-c', code], env=dict(clean, **env), cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert proc.returncode == 0 and proc.stdout.split('\n')[-2] == want, (env, proc.stdout[-500:], proc.stderr[-500:])


def test_a_route_record_asks_the_routes_own_float16_switch(monkeypatch):
    # (dtype, the route's bfloat16 switch, its float16 switch) -> the suffix
    rows = ((F16, True, True, '_f16'), (F16, False, True, '_f16'), (F16, True, False, None), (F16, False, False, None),
            (BF, True, False, '_bf16'), (BF, True, True, '_bf16'), (BF, False, True, None), (F32, True, True, None))
    for f16 in (False, True):
        monkeypatch.setattr(fused, 'F16', f16)
        # a route with a float16 switch of its own: F16 is not asked, and neither dtype asks the other's switch
        for route, own, own_f16 in ((fused.ROUTE16_GCONV, 'GCONV_BF16', 'GCONV_F16'), (fused.ROUTE16_STEM7, 'STEM7_BF16', 'STEM7_F16')):
            for dtype, bf16_on, f16_on, want in rows:
                monkeypatch.setattr(fused, own, bf16_on)
                monkeypatch.setattr(fused, own_f16, f16_on)
                assert route.suffix(dtype) == want, (route.stem, dtype, bf16_on, f16_on, f16)
        # a route without one: F16, as before
        for route, own in ((fused.ROUTE16_CONV3, 'CONV3_BF16'), (fused.ROUTE16_PAIR, 'PAIR_BF16')):
            monkeypatch.setattr(fused, own, True)
            assert route.suffix(F16) == ('_f16' if f16 else None) and route.suffix(BF) == '_bf16'
        assert fused.ROUTE16_GEMM.suffix(F16) == ('_f16' if f16 else None)
        # the heads: ONE switch for both types, which asks neither F16 nor any switch above
        for head16 in (False, True):
            monkeypatch.setattr(fused, 'HEAD16', head16)
            assert fused.ROUTE16_HEAD.suffix(BF) == ('_bf16' if head16 else None) and fused.ROUTE16_HEAD.suffix(F16) == ('_f16' if head16 else None)
            assert fused.ROUTE16_HEAD.suffix(F32) is None
    assert fused.ROUTE16_GCONV.symbol(F16) == GCONV and fused.ROUTE16_STEM7.symbol(F16) == STEM
    assert fused.ROUTE16_HEAD.symbol(BF) == 'opa_head_conv_fields_bf16' and fused.ROUTE16_HEAD.symbol(F16) == 'opa_head_conv_fields_f16'
    # the declined sets are read from the module when asked: the grouped 3x3 has one per type, the stem float16's alone, the heads one for both
    for name, route, dtypes in (('GCONV_BF16_DECLINED', fused.ROUTE16_GCONV, (BF,)), ('GCONV_F16_DECLINED', fused.ROUTE16_GCONV, (F16,)),
                                ('STEM7_F16_DECLINED', fused.ROUTE16_STEM7, (F16,)), ('HEAD16_DECLINED', fused.ROUTE16_HEAD, (BF, F16)),
                                ('PAIR_BF16_DECLINED', fused.ROUTE16_PAIR, (BF, F16))):
        with monkeypatch.context() as m:
            m.setattr(fused, name, frozenset({'key'}))
            assert [dt for dt in (BF, F16) if 'key' in route.declined_set(dt)] == list(dtypes), name
    assert fused.ROUTE16_CONV3.declined_set(BF) == fused.ROUTE16_GEMM.declined_set(F16) == frozenset()
    assert fused.GCONV_F16_DECLINED == frozenset() or all(len(k) == 3 for k in fused.GCONV_F16_DECLINED)
    assert fused.STEM7_F16_DECLINED == frozenset() or all(len(k) == 3 for k in fused.STEM7_F16_DECLINED)


# ---- gconv3x3_bf16_supported for float16 operands ---------------------------------------------------------------------------------------

def _t(channels=128, dtype=F16, **kw):
    return gh._t(channels, dtype, **kw)


def _gconv(c=128, cg=4, dtype=F16, **kw):
    return gh._conv(c, cg, dtype=dtype, **kw)


def _bias(n=128, dtype=F16):
    return torch.zeros(n, dtype=dtype)


def test_the_grouped_predicate_declines(on):
    """``test_gconv3x3_bf16_host.py``'s rows for float16 operands: every reason on its own; the base cases first."""
    monkeypatch = on
    ok = fused.gconv3x3_bf16_supported
    conv, x, bias = _gconv(), _t(), _bias()
    with torch.no_grad():
        assert ok(conv, x, bias) and ok(conv, x, None) and ok(conv, x, bias.float())
        assert ok(_gconv(stride=2), x, bias) and ok(_gconv(dilation=2), x, bias) and ok(_gconv(dilation=4), x, bias)
        for cg in (8, 16, 32, 64):
            assert ok(_gconv(cg=cg), x, bias), cg
        assert ok(_gconv(192, 64), _t(192), _bias(192)) and ok(_gconv(64, 4), _t(64), _bias(64))
        # the switch -- its own: every other 16-bit switch on does not stand in for it --, the library, the device
        with monkeypatch.context() as m:
            m.setattr(fused, 'GCONV_F16', False)
            assert not ok(conv, x, bias)
            for name in BF16_SWITCHES + OTHER_F16_SWITCHES + ('STEM7_F16',):
                m.setattr(fused, name, True)
            assert not ok(conv, x, bias)
        with monkeypatch.context() as m:
            m.setattr(_lib, 'available', lambda: False)
            assert not ok(conv, x, bias)
        assert not ok(conv, torch.zeros(2, 128, 9, 7, dtype=F16).contiguous(memory_format=CL), bias)          # a CPU tensor
        # the dtypes: float32; mixed 16-bit operands in every place; autocast and its pairing
        assert not ok(_gconv(dtype=F32), _t(dtype=F32), bias.float())
        assert not ok(_gconv(dtype=F32), x, bias)
        assert not ok(conv, _t(dtype=F32), bias) and not ok(conv, _t(dtype=BF), bias)
        assert not ok(_gconv(dtype=BF), x, bias) and not ok(conv, x, _bias(dtype=BF))
        with monkeypatch.context() as m:
            m.setattr(fused, 'GCONV_BF16', True)                                                               # (both types' switches on)
            assert not ok(conv, _t(dtype=BF), bias) and not ok(_gconv(dtype=BF), x, bias) and not ok(conv, x, _bias(dtype=BF))
            assert not ok(_gconv(dtype=BF), _t(dtype=BF), _bias(dtype=F16))
        with monkeypatch.context() as m:
            m.setattr(torch, 'is_autocast_enabled', lambda *a: True)
            assert not ok(conv, x, bias)
        # NCHW, a channel slice (not dense), other channels, no pixels
        assert not ok(conv, torch.zeros(2, 128, 9, 7, dtype=F16).as_subclass(_OnDevice), bias)
        assert not ok(conv, _t(256)[:, :128], bias) and not ok(conv, _t(256), bias)
        assert not ok(conv, _t(hw=(0, 7)), bias)
        # groups: none (the dense route's), one per channel pair, widths that do not divide 64
        assert not ok(nn.Conv2d(128, 128, 3, 1, 1, bias=False).to(F16).requires_grad_(False), x, bias)
        assert not ok(_gconv(cg=2), x, bias) and not ok(_gconv(cg=1), x, bias)
        assert not ok(_gconv(192, 12), _t(192), _bias(192)) and not ok(_gconv(192, 24), _t(192), _bias(192))
        assert not ok(_gconv(384, 128), _t(384), _bias(384))
        # channels: no multiple of 64, more output than input channels
        assert not ok(_gconv(96, 4), _t(96), _bias(96)) and not ok(_gconv(32, 4), _t(32), _bias(32))
        assert not ok(_gconv(128, 4, n=256), x, _bias(256))
        # another convolution: a bias of its own, 1x1, 5x5, padding != dilation, a stride of 3, a dilation of 3, stride 2 dilated
        own = nn.Conv2d(128, 128, 3, 1, 1, groups=32).to(F16).requires_grad_(False)
        assert own.bias is not None and not ok(own, x, bias)
        assert not ok(nn.Conv2d(128, 128, 1, groups=32, bias=False).to(F16).requires_grad_(False), x, bias)
        assert not ok(nn.Conv2d(128, 128, 5, 1, 2, groups=32, bias=False).to(F16).requires_grad_(False), x, bias)
        assert not ok(_gconv(padding=0), x, bias) and not ok(_gconv(dilation=2, padding=1), x, bias) and not ok(_gconv(padding=2), x, bias)
        assert not ok(_gconv(stride=3), x, bias) and not ok(_gconv(dilation=3), x, bias) and not ok(_gconv(stride=2, dilation=2), x, bias)
        assert not ok(nn.Conv2d(128, 128, 3, (1, 2), 1, groups=32, bias=False).to(F16).requires_grad_(False), x, bias)
        # the folded bias: another length
        assert not ok(conv, x, _bias(64))
        # a layer the timing declined: float16's set, not bfloat16's
        with monkeypatch.context() as m:
            m.setattr(fused, 'GCONV_F16_DECLINED', frozenset({(128, 4, 1)}))
            assert not ok(conv, x, bias) and ok(_gconv(stride=2), x, bias) and ok(_gconv(cg=8), x, bias)
        with monkeypatch.context() as m:
            m.setattr(fused, 'GCONV_F16_DECLINED', frozenset())
            m.setattr(fused, 'GCONV_BF16_DECLINED', frozenset({(128, 4, 1)}))
            assert ok(conv, x, bias)
    with pytest.raises(TypeError):                                                                             # no residual operand
        ok(conv, x, bias, _t())
    # grad enabled and something that autograd follows
    assert ok(conv, x, bias)
    assert not ok(conv, _t().requires_grad_(), bias) and not ok(_gconv().requires_grad_(True), x, bias)
    assert not ok(conv, x, _bias(dtype=F32).requires_grad_())


# ---- stem7x7_bf16_supported for float16 operands ----------------------------------------------------------------------------------------

def _x(layout='cl', dtype=F16, **kw):
    return sh._x(layout, dtype, **kw)


def _stem(n=64, dtype=F16, **kw):
    return sh._conv(n, dtype=dtype, **kw)


def test_the_stem_predicate_declines(on):
    """``test_stem7x7_bf16_host.py``'s rows for float16 operands: every reason on its own; the base cases first."""
    monkeypatch = on
    ok = fused.stem7x7_bf16_supported
    conv, x, bias = _stem(), _x(), _bias(64)
    with torch.no_grad():
        assert ok(conv, x, bias) and ok(conv, x, None) and ok(conv, x, bias.float()) and ok(conv, x, bias, True) and ok(conv, x, bias, False)
        assert ok(conv, _x('nchw'), bias) and ok(conv, _x('crop'), bias) and ok(_stem(stride=1), x, bias) and ok(_stem(128), x, _bias(128))
        with monkeypatch.context() as m:                                                  # its own switch: no other stands in for it
            m.setattr(fused, 'STEM7_F16', False)
            assert not ok(conv, x, bias)
            for name in BF16_SWITCHES + OTHER_F16_SWITCHES + ('GCONV_F16',):
                m.setattr(fused, name, True)
            assert not ok(conv, x, bias)
        with monkeypatch.context() as m:
            m.setattr(_lib, 'available', lambda: False)
            assert not ok(conv, x, bias)
        assert not ok(conv, torch.zeros(2, 3, 9, 7, dtype=F16), bias)                     # a CPU tensor
        assert not ok(_stem(dtype=F32), _x(dtype=F32), bias.float())                      # float32
        assert not ok(conv, _x(dtype=F32), bias) and not ok(conv, _x(dtype=BF), bias)     # mixed operands, in every place
        assert not ok(_stem(dtype=F32), x, bias) and not ok(_stem(dtype=BF), x, bias) and not ok(conv, x, _bias(64, BF))
        with monkeypatch.context() as m:
            m.setattr(fused, 'STEM7_BF16', True)                                          # (both types' switches on)
            assert not ok(conv, _x(dtype=BF), bias) and not ok(_stem(dtype=BF), x, bias) and not ok(conv, x, _bias(64, BF))
            assert not ok(_stem(dtype=BF), _x(dtype=BF), _bias(64, F16))
        with monkeypatch.context() as m:                                                  # autocast
            m.setattr(torch, 'is_autocast_enabled', lambda *a: True)
            assert not ok(conv, x, bias)
        assert not ok(_stem(c=4), _x(channels=4), bias)                                   # 4 channels
        assert not ok(conv, _x(channels=4), bias)
        assert not ok(_stem(k=3, padding=1), x, bias)                                     # a 3x3 kernel
        assert not ok(_stem(k=5, padding=2), x, bias)
        assert not ok(_stem(stride=3), x, bias)                                           # stride 3
        assert not ok(nn.Conv2d(3, 64, 7, (1, 2), 3, bias=False).to(F16).requires_grad_(False), x, bias)
        assert not ok(_stem(padding=2), x, bias)                                          # padding 2
        assert not ok(_stem(dilation=2), x, bias)
        own = _stem(bias=True)                                                            # a convolution with a bias
        assert own.bias is not None and not ok(own, x, bias)
        assert not ok(_stem(32), x, _bias(32)) and not ok(_stem(96), x, _bias(96))        # c_out 32
        assert not ok(conv, x, _bias(128))                                                # the folded bias: another length
        assert not ok(conv, _x(hw=(0, 7)), bias) and not ok(conv, _x(batch=0), bias)      # no pixels
        assert not ok(conv, _x('nchw').as_strided((2, 3, 9, 7), (0, 63, 7, 1)).as_subclass(_OnDevice), bias)   # a stride of 0
        assert not ok(conv, torch.zeros(2, 9, 7, 3, dtype=F16).permute(0, 3, 1, 2)[0].as_subclass(_OnDevice), bias)   # 3 dimensions
        # a stem the timing declined: (c_out, stride, pooled)
        with monkeypatch.context() as m:
            m.setattr(fused, 'STEM7_F16_DECLINED', frozenset({(64, 2, True)}))
            assert not ok(conv, x, bias, True) and ok(conv, x, bias, False) and ok(conv, x, bias)
            assert ok(_stem(stride=1), x, bias, True) and ok(_stem(128), x, _bias(128), True)
    # grad enabled and something that autograd follows
    assert ok(conv, x, bias)
    assert not ok(conv, _x(dtype=F32).requires_grad_().to(F16).as_subclass(_OnDevice), bias)
    assert not ok(_stem().requires_grad_(True), x, bias) and not ok(conv, x, _bias(64).requires_grad_())


# ---- the bfloat16 answers ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('new', [False, True])
@pytest.mark.parametrize('own', [False, True])
def test_bfloat16_operands_answer_as_before_whatever_the_new_switches_say(monkeypatch, own, new):
    monkeypatch.setattr(_lib, 'available', lambda: True)
    monkeypatch.setattr(fused, 'GCONV_F16', new)
    monkeypatch.setattr(fused, 'STEM7_F16', new)
    monkeypatch.setattr(fused, 'GCONV_BF16', own)
    monkeypatch.setattr(fused, 'STEM7_BF16', own)
    monkeypatch.setattr(fused, 'GCONV_F16_DECLINED', frozenset({(128, 4, 1)}))            # (float16's sets decline no bfloat16 layer)
    monkeypatch.setattr(fused, 'STEM7_F16_DECLINED', frozenset({(64, 2, True), (64, 2, False)}))
    with torch.no_grad():
        assert fused.gconv3x3_bf16_supported(gh._conv(), gh._t(), gh._bias()) is own
        assert fused.gconv3x3_bf16_supported(gh._conv(), gh._t(), gh._bias().float()) is own
        assert fused.gconv3x3_bf16_supported(gh._conv(cg=2), gh._t(), gh._bias()) is False
        for pooled in ((), (True,), (False,)):
            assert fused.stem7x7_bf16_supported(sh._conv(), sh._x(), sh._bias(), *pooled) is own
        assert fused.stem7x7_bf16_supported(sh._conv(), sh._x('crop'), None) is own
        assert fused.stem7x7_bf16_supported(sh._conv(32), sh._x(), sh._bias(32)) is False


# ---- the derived operands ---------------------------------------------------------------------------------------------------------------

def _unpacked(w9, c, cg):
    co, j = torch.arange(c)[:, None], torch.arange(64)[None, :]
    return w9.permute(0, 2, 1)[(j // cg) == ((co % 64) // cg)].reshape(c, cg, 3, 3)


def test_the_grouped_operands_follow_the_cast_and_the_weights():
    """Run in bfloat16, cast with ``.half()``, run again: the block-diagonal weight is float16 -- exact zeros off the group, the
    weight's own values on it --, the bias float32, and both are derived anew (``derived``'s key, storage and version, is another)."""
    block = gh._optimized_bf16(gh._grouped_block(2))
    conv = block.conv2
    w9, b32 = fused.gconv3x3_bf16_weight_of(conv, block.fb2)
    key = conv._opa_w_gconv_bf16[0]
    assert w9.dtype == BF and b32.dtype == F32
    block.half()
    w9h, b32h = fused.gconv3x3_bf16_weight_of(conv, block.fb2)
    assert conv._opa_w_gconv_bf16[0] != key                                               # the cast gives a new key
    assert w9h is not w9 and w9h.dtype == F16 and tuple(w9h.shape) == (128, 9, 64) and w9h.is_contiguous()
    assert conv.weight.dtype == F16 and torch.equal(_unpacked(w9h, 128, 4), conv.weight)
    co, j = torch.arange(128)[:, None], torch.arange(64)[None, :]
    assert bool((w9h.permute(1, 0, 2)[:, (j // 4) != ((co % 64) // 4)] == 0).all()) and int((w9h != 0).sum()) <= 128 * 9 * 4
    assert b32h is not b32 and b32h.dtype == F32 and block.fb2.dtype == F16 and torch.equal(b32h, block.fb2.float())
    again = fused.gconv3x3_bf16_weight_of(conv, block.fb2)
    assert again[0] is w9h and again[1] is b32h                                           # kept on the module
    torch.manual_seed(3)
    state = {k: torch.randn_like(v) for k, v in block.state_dict().items()}
    old = w9h.clone()
    block.load_state_dict(state)                                                          # (in place: the version counters move)
    w9s, b32s = fused.gconv3x3_bf16_weight_of(conv, block.fb2)
    # (the pointers stayed: the kept tensors are overwritten in place -- an address a HIP graph holds sees the new weights)
    assert w9s is w9h and b32s is b32h and w9s.dtype == F16 and torch.equal(_unpacked(w9s, 128, 4), state['conv2.weight']) and not torch.equal(w9s, old)
    assert torch.equal(b32s, state['fb2'].float()) and b32s.dtype == F32
    assert fused.gconv3x3_bf16_weight_of(conv, block.fb2.float())[1].dtype == F32         # a float32 bias is taken as it is
    assert '_opa_w_gconv_bf16' not in conv.state_dict()


def test_the_stem_operands_follow_the_cast_and_the_weights():
    torch.manual_seed(2)
    net = network.optimize_for_inference_(network.Resnet('resnet18').eval()).to(BF).requires_grad_(False)
    conv = net.input_block[0]
    wk, b32 = fused.stem7x7_bf16_weight_of(conv, net.fb0)
    key = conv._opa_w_stem7_bf16[0]
    assert wk.dtype == BF
    net.half()
    wkh, b32h = fused.stem7x7_bf16_weight_of(conv, net.fb0)
    assert conv._opa_w_stem7_bf16[0] != key                                               # the cast gives a new key
    assert wkh is not wk and wkh.dtype == F16 and tuple(wkh.shape) == (64, 192) and wkh.is_contiguous()
    for k in range(192):                                                                  # element by element, from the definition
        ky, kx, ci = k // 24, k % 24 // 3, k % 3
        if ky < 7 and kx < 7:
            assert torch.equal(wkh[:, k], conv.weight[:, ci, ky, kx]), k
        else:
            assert bool((wkh[:, k] == 0).all()), k                                        # the zero columns of K
    assert b32h is not b32 and b32h.dtype == F32 and net.fb0.dtype == F16 and torch.equal(b32h, net.fb0.float())
    state = {k: torch.randn_like(v) for k, v in net.state_dict().items()}
    old = wkh.clone()
    net.load_state_dict(state)
    wks, b32s = fused.stem7x7_bf16_weight_of(conv, net.fb0)
    assert wks is wkh and b32s is b32h and wks.dtype == F16 and not torch.equal(wks, old)          # (in place: overwritten where they are kept)
    assert torch.equal(wks.view(64, 8, 8, 3)[:, :7, :7], state['input_block.0.weight'].permute(0, 2, 3, 1))
    assert torch.equal(b32s, state['fb0'].float())


# ---- the launches of a whole network ----------------------------------------------------------------------------------------------------

NETWORKS = {'resnext50': ('resnext50', {}), 'resnet18-pool0': ('resnet18', {'pool0_stride': 2})}
# sha256 of '\n'.join(trace) of the ``.half()`` network with ``F16`` on and the new switches off, recorded ON THE PARENT COMMIT with
# ``test_f16_host.py``'s ``_tracer`` (which names neither new switch) -- (entries of the trace, of them ``miopen:``)
PARENT_TRACES = {
    'resnext50': ('a8ab4da277c41393cb1122badcd571eef916c7fd8cae8ccf3a3a54956bbc01f6', 50, 17),
    'resnet18-pool0': ('5e238f4d926611fbdd828bd8f2fe2909d5127d02cc6ef83fff19a7c49b60f897', 21, 1),
}


@pytest.fixture
def traced(monkeypatch):
    for name, entry in NETWORKS.items():
        monkeypatch.setitem(tf.NETWORKS, name, entry)
    trace, cast = tf._tracer(monkeypatch)
    for name in ('GCONV_F16', 'STEM7_F16', 'HEAD16', 'UNIT_F16'):
        monkeypatch.setattr(fused, name, False)
    monkeypatch.setattr(fused, 'F16', True)
    return trace, cast


def _symbols(trace):
    return [launch.split('(')[0] for launch in trace if not launch.startswith('miopen:')]


def _miopen(trace):
    return [launch for launch in trace if launch.startswith('miopen:')]


def test_a_half_resnext50_calls_no_convolution_and_owes_nothing(traced, monkeypatch):
    trace, cast = traced
    net, x = cast('resnext50', F16)
    monkeypatch.setattr(fused, 'GCONV_F16', True)
    monkeypatch.setattr(fused, 'STEM7_F16', True)
    run = tf._forward(trace, net, x)
    symbols = _symbols(run)
    assert _miopen(run) == []                                                             # no nn.Conv2d is called
    assert symbols.count(GCONV) == 16 and symbols.count(STEM) == 1 and run[0].startswith(STEM + '(')
    assert 'opa_gemm_pro_bias_act_f16' not in symbols and 'opa_bias_act' not in symbols   # nothing is owed, no epilogue pass
    assert not [s for s in symbols if s.endswith('_bf16')]
    assert set(symbols) == {STEM, GCONV, 'opa_gemm_bias_act_f16', 'opa_gemm2_bias_act_f16'}
    grouped = [m for m in net.modules() if isinstance(m, nn.Conv2d) and m.groups > 1]
    assert len(grouped) == 16 and {m.in_channels // m.groups for m in grouped} == {4, 8, 16, 32}
    # each switch alone moves its own launches and nothing else
    monkeypatch.setattr(fused, 'STEM7_F16', False)
    only_grouped = tf._forward(trace, net, x)
    assert _miopen(only_grouped) == ['miopen:input_block.0'] and only_grouped[1].startswith('opa_bias_act(') and only_grouped[2:] == run[1:]
    monkeypatch.setattr(fused, 'STEM7_F16', True)
    monkeypatch.setattr(fused, 'GCONV_F16', False)
    only_stem = tf._forward(trace, net, x)
    # (torch's grouped convolutions owe bias + ReLU to the next GEMM's operand prologue: 12 plain blocks, and 4 through the pair's a_bias)
    assert only_stem[0] == run[0] and len(_miopen(only_stem)) == 16 and _symbols(only_stem).count('opa_gemm_pro_bias_act_f16') == 12
    assert GCONV not in _symbols(only_stem) and len(only_stem) == len(run)


def test_the_half_trace_is_the_bfloat16_networks_under_the_float16_names(traced, monkeypatch):
    trace, cast = traced
    monkeypatch.setattr(fused, 'F16', False)
    for name in ('CONV3_BF16', 'PAIR_BF16', 'GCONV_BF16', 'STEM7_BF16'):
        monkeypatch.setattr(fused, name, True)
    brain = {name: tf._forward(trace, *cast(name, BF)) for name in NETWORKS}
    for name in ('CONV3_BF16', 'PAIR_BF16', 'GCONV_BF16', 'STEM7_BF16'):
        monkeypatch.setattr(fused, name, False)
    for name in ('F16', 'GCONV_F16', 'STEM7_F16'):
        monkeypatch.setattr(fused, name, True)
    half = tf._forward(trace, *cast('resnext50', F16))
    assert half == [tf._as_float16(launch) for launch in brain['resnext50']]
    # with the pool, the bfloat16 network has the pool kernel behind the stem, the float16 one F.max_pool2d: the rest is equal
    half = tf._forward(trace, *cast('resnet18-pool0', F16))
    assert brain['resnet18-pool0'][1].startswith('opa_maxpool3x3_bias_act(')
    assert half[0] == tf._as_float16(brain['resnet18-pool0'][0]) and half[0].startswith(STEM + '(') and half[0].endswith(', 2, 1)')
    assert half[1:] == [tf._as_float16(launch) for launch in brain['resnet18-pool0'][2:]]
    assert _miopen(half) == [] and 'opa_maxpool3x3_bias_act' not in _symbols(half) and 'opa_bias_act' not in _symbols(half)


@pytest.mark.parametrize('net_name', sorted(NETWORKS))
def test_with_the_new_switches_off_the_half_network_runs_what_it_ran(traced, monkeypatch, net_name):
    """``F16`` on, the new switches off, every bfloat16 switch on: none of the new symbols, the stem and the grouped convolutions
    called, and the trace is the parent commit's (its digest above)."""
    trace, cast = traced
    for name in BF16_SWITCHES:
        monkeypatch.setattr(fused, name, True)
    off = tf._forward(trace, *cast(net_name, F16))
    assert GCONV not in _symbols(off) and STEM not in _symbols(off) and not [s for s in _symbols(off) if s.endswith('_bf16')]
    grouped = 16 if net_name == 'resnext50' else 0
    assert len(_miopen(off)) == 1 + grouped and off[0] == 'miopen:input_block.0'
    digest, entries, miopen = PARENT_TRACES[net_name]
    assert (len(off), len(_miopen(off))) == (entries, miopen)
    assert tf._digest(off) == digest


def test_the_other_dtypes_trace_the_same_with_the_new_switches_on_and_off(traced, monkeypatch):
    trace, cast = traced
    for dtype in (F32, BF):
        for bf16_switches in (False, True):
            for name in ('CONV3_BF16', 'PAIR_BF16', 'GCONV_BF16', 'STEM7_BF16'):
                monkeypatch.setattr(fused, name, bf16_switches)
            for net_name in sorted(NETWORKS):
                net, x = cast(net_name, dtype)
                monkeypatch.setattr(fused, 'GCONV_F16', False)
                monkeypatch.setattr(fused, 'STEM7_F16', False)
                off = tf._forward(trace, net, x)
                monkeypatch.setattr(fused, 'GCONV_F16', True)
                monkeypatch.setattr(fused, 'STEM7_F16', True)
                assert tf._forward(trace, net, x) == off and off and not [launch for launch in off if '_f16(' in launch]


def test_the_header_the_binding_and_the_library_agree():
    with open(os.path.join(ROOT, 'include', 'openpifpaf_amd.h')) as f:
        header = f.read()
    for symbol, twin, count in ((GCONV, 'opa_gconv3x3_act_bf16', 13), (STEM, 'opa_stem7x7_act_bf16', 15)):
        assert symbol + '(' in header and symbol in _lib.SYMBOLS and hasattr(_lib.lib(), symbol)
        assert len(header.split('int ' + symbol + '(')[1].split(');')[0].split(',')) == count
        assert _lib.SYMBOLS[symbol] == _lib.SYMBOLS[twin] and len(_lib.SYMBOLS[symbol][1]) == count
