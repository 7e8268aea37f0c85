"""The float16 routes on the host: the switch ``fused.F16`` (OPA_F16), what the four predicates of the 16-bit MFMA routes answer for
float16 operands -- and that they answer for bfloat16 operands what they answered, whatever ``F16`` says --, the derived operands,
and the launches of a whole ResNet cast with ``.half()``, traced on the CPU with the technique of ``test_gemm2_bf16_route_trace.py`` (a
recorder in place of ``fused._launch``, tensors that say they are on the GPU, the library reported as built, a forward hook on every
``nn.Conv2d`` that records ``miopen:<module name>``).  Here the parameters and buffers say so too (``_on_device_``), so that the plain
1x1 GEMM, which asks ``weight.is_cuda``, is traced as well.  No GPU is touched and nothing is timed.

Every test sets ``fused.F16`` through monkeypatch, which refuses to set an attribute that does not exist: without the feature every
test of this file fails."""
import copy
import hashlib

import pytest
import torch
from torch import nn

from openpifpaf_amd import _lib, fused, network, winograd

import trunk_common as tc

CL = torch.channels_last
F16, BF = torch.float16, torch.bfloat16
F16_SYMBOLS = ('opa_gemm_bias_act_f16', 'opa_gemm_pro_bias_act_f16', 'opa_conv3x3_act_f16', 'opa_gemm2_bias_act_f16')


class _OnDevice(torch.Tensor):
    is_cuda = True


def _dev(t):
    return t.as_subclass(_OnDevice)


def _on_device_(module):
    """Every parameter and buffer of ``module`` says that it is on the GPU (after the last cast: a cast makes plain tensors again)."""
    for m in module.modules():
        for name, p in list(m._parameters.items()):
            if p is not None:
                m._parameters[name] = nn.Parameter(_dev(p.data), requires_grad=p.requires_grad)
        for name, b in list(m._buffers.items()):
            if b is not None:
                m._buffers[name] = _dev(b)
    return module


def _image(b, c, h, w, dt, seed=0, offset=0):
    """A channels-last ``[b, c, h, w]`` of ``dt`` that says it is on the GPU; ``offset``: elements between a 16-byte boundary and its
    first element."""
    flat = torch.randn(b * h * w * c + 8, generator=tc.gen(seed)).to(dt)
    assert flat.data_ptr() % 16 == 0
    return _dev(flat[offset:offset + b * h * w * c].view(b, h, w, c).permute(0, 3, 1, 2))


def _vector(n, dt, seed=1, offset=0):
    flat = torch.randn(n + 8, generator=tc.gen(seed)).to(dt)
    return _dev(flat[offset:offset + n])


def _conv(c_in, c_out, k, dt, stride=1, dilation=1, **kw):
    pad = dilation if k == 3 else 0
    conv = nn.Conv2d(c_in, c_out, k, stride, pad, dilation=dilation, bias=False, **kw).to(dt).requires_grad_(False)
    return _on_device_(conv)


@pytest.fixture
def built(monkeypatch):
    monkeypatch.setattr(_lib, 'available', lambda: True)
    for name in ('CONV3_BF16', 'PAIR_BF16', 'STEM7_BF16', 'GCONV_BF16', 'UNIT_BF16'):
        monkeypatch.setattr(fused, name, False)
    monkeypatch.setattr(fused, 'F16', True)
    return monkeypatch


# ---- the predicates: a valid case per predicate as keyword arguments, and what spoils it ------------------------------------------------

def _gemm_case(dt):
    return dict(x=_image(2, 64, 5, 3, dt), weight=_dev(torch.randn(128, 64, 1, 1, generator=tc.gen(2)).to(dt)), bias=_vector(128, dt),
                residual=_image(2, 128, 5, 3, dt, 3), a_bias=_vector(64, dt, 4))


def _conv3_case(dt):
    return dict(conv=_conv(64, 128, 3, dt), x=_image(2, 64, 5, 3, dt), bias=_vector(128, dt), residual=_image(2, 128, 5, 3, dt, 3))


def _pair_case(dt):
    return dict(conv=_conv(64, 256, 1, dt), dconv=_conv(128, 256, 1, dt, stride=2), h=_image(2, 64, 3, 2, dt, 5), x=_image(2, 128, 5, 3, dt),
                bias=_vector(256, dt), a_bias=_vector(64, dt, 4))


def _strided_case(dt):
    return dict(dconv=_conv(128, 256, 1, dt, stride=2), x=_image(2, 128, 5, 3, dt))


PREDICATES = {
    'gemm': (lambda: fused.conv1x1_supported, _gemm_case),
    'conv3': (lambda: fused.conv3x3_bf16_supported, _conv3_case),
    'pair': (lambda: fused.pair_bf16_supported, _pair_case),
    'strided': (lambda: fused.conv1x1_strided_bf16_supported, _strided_case),
}
OWN_SWITCH = {'gemm': None, 'conv3': 'CONV3_BF16', 'pair': 'PAIR_BF16', 'strided': 'PAIR_BF16'}


def _with(case, **changes):
    out = dict(case)
    out.update(changes)
    return out


def _requires_grad(t):
    return _dev(t.detach().clone()).requires_grad_(True)


def _spoilt(name, case, other):
    """[(what, the case spoilt)]: ``other``: the same case in the other 16-bit type (for the mixed-dtype cases)."""
    out = []
    if name == 'gemm':
        x, w = case['x'], case['weight']
        out += [('%s of the other 16-bit type' % key, _with(case, **{key: other[key]})) for key in ('weight', 'bias', 'residual', 'a_bias')]
        out += [('%s that autograd follows' % key, _with(case, **{key: _requires_grad(case[key])})) for key in ('x', 'bias', 'residual', 'a_bias')]
        out += [('a float32 bias', _with(case, bias=_dev(case['bias'].float()))),
                ('weight that autograd follows', _with(case, weight=_requires_grad(w))),
                ('K no multiple of 64', _with(case, x=_image(2, 32, 5, 3, F16), weight=_dev(w[:, :32].contiguous()), a_bias=None)),
                ('N no multiple of 64', _with(case, weight=_dev(w[:96].contiguous()), bias=_vector(96, F16), residual=None)),
                ('other input channels', _with(case, x=_image(2, 128, 5, 3, F16), a_bias=None)),
                ('x not channels-last', _with(case, x=_dev(x.contiguous()))),
                ('x of three dimensions', _with(case, x=_dev(x[0]))),
                ('x misaligned', _with(case, x=_image(2, 64, 5, 3, F16, offset=1))),
                ('weight misaligned', _with(case, weight=_dev(torch.randn(128 * 64 + 8).half()[1:1 + 128 * 64].view(128, 64, 1, 1)))),
                ('bias misaligned', _with(case, bias=_vector(128, F16, offset=1))),
                ('bias of another length', _with(case, bias=_vector(64, F16))),
                ('bias not contiguous', _with(case, bias=_dev(_vector(256, F16)[::2]))),
                ('a_bias of another length', _with(case, a_bias=_vector(128, F16))),
                ('residual of another shape', _with(case, residual=_image(2, 128, 3, 5, F16))),
                ('residual not channels-last', _with(case, residual=_dev(case['residual'].contiguous()))),
                ('residual misaligned', _with(case, residual=_image(2, 128, 5, 3, F16, offset=1)))]
    elif name == 'conv3':
        x = case['x']
        out += [('a weight of the other 16-bit type', _with(case, conv=other['conv'])),
                ('a bias of the other 16-bit type', _with(case, bias=other['bias'])),
                ('a residual of the other 16-bit type', _with(case, residual=other['residual'])),
                ('x that autograd follows', _with(case, x=_requires_grad(x))),
                ('a weight that autograd follows', _with(case, conv=_on_device_(_conv(64, 128, 3, F16).requires_grad_(True)))),
                ('a bias that autograd follows', _with(case, bias=_requires_grad(case['bias']))),
                ('a residual that autograd follows', _with(case, residual=_requires_grad(case['residual']))),
                ('groups', _with(case, conv=_conv(64, 128, 3, F16, groups=2))),
                ('a bias of its own', _with(case, conv=_on_device_(nn.Conv2d(64, 128, 3, 1, 1).half().requires_grad_(False)))),
                ('stride 3', _with(case, conv=_conv(64, 128, 3, F16, stride=3), residual=None)),
                ('dilation 3', _with(case, conv=_conv(64, 128, 3, F16, dilation=3))),
                ('dilation 2 with stride 2', _with(case, conv=_conv(64, 128, 3, F16, stride=2, dilation=2), residual=None)),
                ('padding other than the dilation', _with(case, conv=_on_device_(nn.Conv2d(64, 128, 3, 1, 0, bias=False).half().requires_grad_(False)),
                                                          residual=None)),
                ('c_in no multiple of 64', _with(case, conv=_conv(32, 128, 3, F16), x=_image(2, 32, 5, 3, F16))),
                ('c_out no multiple of 64', _with(case, conv=_conv(64, 96, 3, F16), bias=None, residual=None)),
                ('other input channels', _with(case, x=_image(2, 128, 5, 3, F16))),
                ('x not channels-last', _with(case, x=_dev(x.contiguous()))),
                ('x misaligned', _with(case, x=_image(2, 64, 5, 3, F16, offset=1))),
                ('an empty x', _with(case, x=_image(0, 64, 5, 3, F16), residual=None)),
                ('bias of another length', _with(case, bias=_vector(64, F16))),
                ('bias of two dimensions', _with(case, bias=_dev(case['bias'].view(1, -1)))),
                ('residual of another shape', _with(case, residual=_image(2, 128, 3, 5, F16))),
                ('residual not channels-last', _with(case, residual=_dev(case['residual'].contiguous()))),
                ('residual misaligned', _with(case, residual=_image(2, 128, 5, 3, F16, offset=1)))]
    elif name == 'pair':
        h, x = case['h'], case['x']
        out += [('conv of the other 16-bit type', _with(case, conv=other['conv'])), ('dconv of the other 16-bit type', _with(case, dconv=other['dconv'])),
                ('h of the other 16-bit type', _with(case, h=other['h'])), ('a bias of the other 16-bit type', _with(case, bias=other['bias'])),
                ('a_bias of the other 16-bit type', _with(case, a_bias=other['a_bias'])),
                ('h that autograd follows', _with(case, h=_requires_grad(h))), ('x that autograd follows', _with(case, x=_requires_grad(x))),
                ('a bias that autograd follows', _with(case, bias=_requires_grad(case['bias']))),
                ('a_bias that autograd follows', _with(case, a_bias=_requires_grad(case['a_bias']))),
                ('a weight that autograd follows', _with(case, conv=_on_device_(_conv(64, 256, 1, F16).requires_grad_(True)))),
                ('conv of stride 2', _with(case, conv=_conv(64, 256, 1, F16, stride=2))),
                ('dconv of stride 3', _with(case, dconv=_conv(128, 256, 1, F16, stride=3))),
                ('dconv 3x3', _with(case, dconv=_conv(128, 256, 3, F16, stride=2))),
                ('other output channels', _with(case, dconv=_conv(128, 128, 1, F16, stride=2))),
                ('k1 no multiple of 64', _with(case, conv=_conv(32, 256, 1, F16), h=_image(2, 32, 3, 2, F16), a_bias=None)),
                ('k2 no multiple of 64', _with(case, dconv=_conv(96, 256, 1, F16, stride=2), x=_image(2, 96, 5, 3, F16))),
                ('n no multiple of 64', _with(case, conv=_conv(64, 96, 1, F16), dconv=_conv(128, 96, 1, F16, stride=2), bias=None)),
                ('h of other pixels', _with(case, h=_image(2, 64, 5, 3, F16))), ('h of another batch', _with(case, h=_image(1, 64, 3, 2, F16))),
                ('h not channels-last', _with(case, h=_dev(h.contiguous()))), ('x misaligned', _with(case, x=_image(2, 128, 5, 3, F16, offset=1))),
                ('bias of another length', _with(case, bias=_vector(64, F16))),
                ('a_bias of another length', _with(case, a_bias=_vector(128, F16))), ('a_bias misaligned', _with(case, a_bias=_vector(64, F16, offset=1))),
                ('a_bias not contiguous', _with(case, a_bias=_dev(_vector(128, F16)[::2])))]
    else:
        x = case['x']
        out += [('dconv of the other 16-bit type', _with(case, dconv=other['dconv'])), ('x of the other 16-bit type', _with(case, x=other['x'])),
                ('x that autograd follows', _with(case, x=_requires_grad(x))),
                ('a weight that autograd follows', _with(case, dconv=_on_device_(_conv(128, 256, 1, F16, stride=2).requires_grad_(True)))),
                ('stride 3', _with(case, dconv=_conv(128, 256, 1, F16, stride=3))), ('3x3', _with(case, dconv=_conv(128, 256, 3, F16, stride=2))),
                ('k2 no multiple of 64', _with(case, dconv=_conv(96, 256, 1, F16, stride=2), x=_image(2, 96, 5, 3, F16))),
                ('n no multiple of 64', _with(case, dconv=_conv(128, 96, 1, F16, stride=2))),
                ('x not channels-last', _with(case, x=_dev(x.contiguous()))), ('x misaligned', _with(case, x=_image(2, 128, 5, 3, F16, offset=1))),
                ('an empty x', _with(case, x=_image(0, 128, 5, 3, F16)))]
    return out


@pytest.mark.parametrize('name', sorted(PREDICATES))
def test_a_float16_case_is_taken_with_the_switch_on_and_declined_with_it_off(built, name):
    predicate, make = PREDICATES[name]
    case = make(F16)
    assert predicate()(**case)
    for key in [k for k in ('bias', 'residual', 'a_bias') if k in case]:             # (the optional operands)
        assert predicate()(**_with(case, **{key: None}))
    if 'bias' in case and name != 'gemm':                                            # the folded bias may be float32
        assert predicate()(**_with(case, bias=_dev(case['bias'].float())))
    built.setattr(fused, 'F16', False)
    assert not predicate()(**case)
    for own in ('CONV3_BF16', 'PAIR_BF16', 'STEM7_BF16'):                            # ... whatever the bfloat16 switches say
        built.setattr(fused, own, True)
    assert not predicate()(**case)
    built.setattr(fused, 'F16', True)
    assert predicate()(**case)
    built.setattr(_lib, 'available', lambda: False)
    assert name == 'gemm' or not predicate()(**case)                                 # (the plain GEMM never asked)


@pytest.mark.parametrize('name', sorted(PREDICATES))
def test_what_spoils_a_float16_case_with_the_switch_on(built, name):
    predicate, make = PREDICATES[name]
    case, other = make(F16), make(BF)
    for own in ('CONV3_BF16', 'PAIR_BF16'):                                          # (so that no bfloat16 switch is what declines)
        built.setattr(fused, own, True)
    spoilt = _spoilt(name, case, other)
    assert len(spoilt) >= 10
    with torch.enable_grad():
        assert predicate()(**case)
        for what, bad in spoilt:
            assert not predicate()(**bad), what
    with torch.no_grad():                          # nothing is followed without grad mode: those cases are taken
        for what, bad in spoilt:
            assert bool(predicate()(**bad)) == ('autograd follows' in what), what
    with built.context() as m:
        m.setattr(torch, 'is_autocast_enabled', lambda *a: True)
        assert not predicate()(**case)
    assert predicate()(**case)


@pytest.mark.parametrize('f16_switch', [False, True])
@pytest.mark.parametrize('name', sorted(PREDICATES))
def test_a_bfloat16_case_answers_as_before_whatever_the_switch_says(built, name, f16_switch):
    predicate, make = PREDICATES[name]
    case, other = make(BF), make(F16)
    built.setattr(fused, 'F16', f16_switch)
    own = OWN_SWITCH[name]
    if own is None:                                # the plain GEMM has no switch: bfloat16 is taken, also under autocast and grad mode
        assert predicate()(**case)
        with built.context() as m, torch.enable_grad():
            m.setattr(torch, 'is_autocast_enabled', lambda *a: True)
            assert predicate()(**_with(case, x=_requires_grad(case['x'])))
    else:
        assert not predicate()(**case)
        built.setattr(fused, own, True)
        assert predicate()(**case)
        with built.context() as m:
            m.setattr(torch, 'is_autocast_enabled', lambda *a: True)
            assert not predicate()(**case)
    for key in [k for k in case if k != 'x']:      # mixed 16-bit operands are declined in this direction too
        mixed = _with(case, **{key: other[key]})
        assert not predicate()(**mixed), key
    if own is not None and 'bias' in case:
        assert predicate()(**_with(case, bias=_dev(case['bias'].float())))


def test_the_switch_reads_opa_f16_and_ships_off():
    import os
    import subprocess
    import sys
    code = 'from openpifpaf_amd import fused; print(fused.F16, fused.CONV3_BF16, fused.PAIR_BF16)'
    env = {k: v for k, v in os.environ.items() if not k.startswith('OPA_')}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for value, want in ((None, 'False False False'), ('1', 'True False False'), ('0', 'False False False')):
        e = dict(env, **({} if value is None else {'OPA_F16': value}))
        out = subprocess.run([sys.executable, '-c', code], env=e, cwd=root, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and out.stdout.strip() == want, (value, out.stdout, out.stderr[-2000:])
    assert set(F16_SYMBOLS) <= set(_lib.SYMBOLS)


def test_the_symbol_table(built):
    """route record, dtype -> suffix: bfloat16 asks the route's own switch (the 1x1 GEMM has none), float16 asks ``F16``, anything else
    has no route.  (The fixture: every ``*_BF16`` switch off, ``F16`` on.)"""
    gemm, own = fused.ROUTE16_GEMM, {'CONV3_BF16': fused.ROUTE16_CONV3, 'PAIR_BF16': fused.ROUTE16_PAIR}
    assert gemm.suffix(F16) == '_f16' and all(r.suffix(F16) == '_f16' for r in own.values()) and gemm.suffix(BF) == '_bf16'
    assert all(r.suffix(BF) is None for r in own.values()) and gemm.suffix(torch.float32) is None
    assert all(r.suffix(torch.float32) is None for r in own.values())
    built.setattr(fused, 'F16', False)
    assert gemm.suffix(F16) is None and gemm.suffix(BF) == '_bf16'
    for switch, route in own.items():
        built.setattr(fused, switch, True)
        assert route.suffix(F16) is None and route.suffix(BF) == '_bf16'
    assert gemm.symbol(F16) == 'opa_gemm_bias_act_f16' and gemm.symbol(BF, pro=True) == 'opa_gemm_pro_bias_act_bf16'
    assert fused.ROUTE16_CONV3.symbol(F16) == 'opa_conv3x3_act_f16' and fused.ROUTE16_PAIR.symbol(BF) == 'opa_gemm2_bias_act_bf16'
    assert {gemm.symbol(dt, pro) for dt in (F16, BF) for pro in (False, True)} | {r.symbol(dt) for r in own.values() for dt in (F16, BF)} \
        <= set(_lib.SYMBOLS)


# ---- the derived operands ----------------------------------------------------------------------------------------------------------

def test_the_derived_operands_are_float16_with_a_float32_bias_and_follow_the_weights(built):
    conv, bias = _conv(64, 128, 3, F16), _vector(128, F16)
    w9, b32 = fused.conv3x3_bf16_weight_of(conv, bias)
    assert w9.dtype == F16 and tuple(w9.shape) == (128, 9, 64) and w9.is_contiguous() and b32.dtype == torch.float32
    assert torch.equal(w9, conv.weight.detach().permute(0, 2, 3, 1).reshape(128, 9, 64)) and torch.equal(b32, bias.float())
    assert fused.conv3x3_bf16_weight_of(conv, bias)[0] is w9                        # cached
    pconv, dconv, pbias = _conv(64, 256, 1, F16), _conv(128, 256, 1, F16, stride=2), _vector(256, F16)
    wcat, pb32 = fused.pair_bf16_weight_of(pconv, dconv, pbias)
    assert wcat.dtype == F16 and tuple(wcat.shape) == (256, 192) and pb32.dtype == torch.float32 and torch.equal(pb32, pbias.float())
    assert torch.equal(wcat, torch.cat((pconv.weight.detach().reshape(256, 64), dconv.weight.detach().reshape(256, 128)), 1))
    wd, none = fused.pair_bf16_weight_of(None, dconv, None)
    assert none is None and wd.dtype == F16 and torch.equal(wd, dconv.weight.detach().reshape(256, 128))

    def fresh():
        return fused.conv3x3_bf16_weight_of(conv, bias)[0], fused.pair_bf16_weight_of(pconv, dconv, pbias)[0]

    def check():
        a, b = fresh()
        assert a.dtype == F16 and torch.equal(a, conv.weight.detach().permute(0, 2, 3, 1).reshape(128, 9, 64))
        assert b.dtype == F16 and torch.equal(b, torch.cat((pconv.weight.detach().reshape(256, 64), dconv.weight.detach().reshape(256, 128)), 1))
        return a, b
    # load_state_dict (an in-place copy: the version counter moves)
    before = fresh()
    old = [t.clone() for t in before]
    conv.load_state_dict({'weight': torch.randn(128, 64, 3, 3, generator=tc.gen(9)).half()})
    dconv.load_state_dict({'weight': torch.randn(256, 128, 1, 1, generator=tc.gen(10)).half()})
    after = check()
    # (the pointers stayed: the kept tensors are overwritten in place -- an address a HIP graph holds sees the new weights)
    assert after[0] is before[0] and after[1] is before[1] and not torch.equal(after[0], old[0]) and not torch.equal(after[1], old[1])
    old = [t.clone() for t in after]
    # an in-place change
    with torch.no_grad():
        conv.weight.mul_(2.0)
        pconv.weight.add_(1.0)
    again = check()
    assert again[0] is after[0] and again[1] is after[1] and torch.equal(again[0], old[0] * 2) and not torch.equal(again[1], old[1])
    # a round trip through float32: new tensors of equal values
    for m in (conv, pconv, dconv):
        m.half().float().half()
    last = check()
    assert last[0] is not again[0] and last[1] is not again[1] and torch.equal(last[0], again[0]) and torch.equal(last[1], again[1])


# ---- the launches of a whole network --------------------------------------------------------------------------------------------------

NETWORKS = {'resnet18': ('resnet18', {}), 'resnet50': ('resnet50', {}), 'resnet50-dilated': ('resnet50', {'block5_dilation': 2})}
# sha256 of '\n'.join(trace) of the ``.half()`` network with ``F16`` off, recorded ON THE PARENT COMMIT with this file's ``traced``
# fixture (which names no float16 switch there): MIOpen for every convolution, in forward order, with ``opa_bias_act`` (dtype 1) behind
# each one but the downsampling convolutions and in front of conv3 of every Bottleneck (conv2's owed bias + ReLU) -- (entries of the
# trace, of them ``miopen:``)
PARENT_HALF_TRACES = {
    'resnet18': ('ea6f14c12636cd087c2d2f7e2fdf1e7fb258d6f02c1983375a44611c0c2bf505', 37, 20),
    'resnet50': ('e1c28ab8286979dc3b55145df72594b7bd812cc623299fa01aa84dbefb2599b7', 102, 53),
    'resnet50-dilated': ('a5b17edf83f4fffdab8424d70315fb6adcf49b72161ceb11528bc59d3199eeb4', 102, 53),
}


def _digest(trace):
    return hashlib.sha256('\n'.join(trace).encode()).hexdigest()


def _tracer(monkeypatch):
    """-> (trace, cast(net_name, dtype) -> (the optimized network of that dtype with a hook on every convolution, its input))"""
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
    monkeypatch.setenv('OPA_CONV1X1', 'gemm')
    for name, value in (('X3_TERMS', 6), ('_CHOICE', {}), ('FORCE_PICK', 'conv'), ('GCONV', False), ('STEM7_BF16', False),
                        ('CONV3_BF16', False), ('PAIR_BF16', False), ('GCONV_BF16', False), ('UNIT_BF16', False)):
        monkeypatch.setattr(fused, name, value)
    monkeypatch.setattr(winograd, '_mode', winograd.get_mode())
    base = {}

    def cast(net_name, dtype):
        if net_name not in base:
            config, options = NETWORKS[net_name]
            torch.manual_seed(5)
            base[net_name] = network.optimize_for_inference_(copy.deepcopy(tc.randomize_(network.Resnet(config, **options), 5)))
        net = _on_device_(copy.deepcopy(base[net_name]).to(dtype))
        for name, m in net.named_modules():
            if isinstance(m, nn.Conv2d):
                m.register_forward_hook(lambda mod, args, out, name=name: trace.append('miopen:' + name))
        x = torch.randn((1, 3, 33, 25), generator=tc.gen(7)).to(dtype).contiguous(memory_format=CL).as_subclass(_OnDevice)
        return net, x
    return trace, cast


@pytest.fixture
def traced(monkeypatch):
    return _tracer(monkeypatch)


def _forward(trace, net, x):
    del trace[:]
    with torch.no_grad():
        net(x)
    return list(trace)


def _as_float16(launch):
    """A launch of the bfloat16 network as the float16 network makes it: the symbol's suffix, and the element type's code where a launch
    names it (``opa_bias_act``'s dtype, its sixth argument: 2 -> 1)."""
    launch = launch.replace('_bf16(', '_f16(')
    if launch.startswith('opa_bias_act('):
        args = launch[:-1].split(', ')
        assert args[5] == '2'
        args[5] = '1'
        launch = ', '.join(args) + ')'
    return launch


@pytest.mark.parametrize('net_name', sorted(NETWORKS))
def test_the_half_network_launches_what_the_bfloat16_network_launches(traced, monkeypatch, net_name):
    """``F16`` on: the trace of the ``.half()`` network is the trace of the ``.bfloat16()`` network with ``CONV3_BF16`` and ``PAIR_BF16``
    on and ``STEM7_BF16`` off, argument for argument, with ``_f16(`` for ``_bf16(`` (and float16's dtype code in the stem's
    ``opa_bias_act``); the only convolution that reaches MIOpen is the stem."""
    trace, cast = traced
    monkeypatch.setattr(fused, 'F16', False)
    monkeypatch.setattr(fused, 'CONV3_BF16', True)
    monkeypatch.setattr(fused, 'PAIR_BF16', True)
    brain = _forward(trace, *cast(net_name, BF))
    monkeypatch.setattr(fused, 'CONV3_BF16', False)
    monkeypatch.setattr(fused, 'PAIR_BF16', False)
    monkeypatch.setattr(fused, 'F16', True)
    half = _forward(trace, *cast(net_name, F16))
    assert half == [_as_float16(launch) for launch in brain]
    assert [launch for launch in half if launch.startswith('miopen:')] == ['miopen:input_block.0']
    symbols = [launch.split('(')[0] for launch in half if not launch.startswith('miopen:')]
    plain = set() if net_name == 'resnet18' else {'opa_gemm_bias_act_f16'}           # (BasicBlocks have no 1x1 but the downsampling one)
    assert set(symbols) == {'opa_bias_act', 'opa_conv3x3_act_f16', 'opa_gemm2_bias_act_f16'} | plain
    assert symbols.count('opa_bias_act') == 1 and not [s for s in symbols if s.endswith('_bf16')]
    net = cast(net_name, F16)[0]
    convs = [m for m in net.modules() if isinstance(m, nn.Conv2d)]
    dense3 = [m for m in convs if m.kernel_size == (3, 3)]
    down = [m for name, m in net.named_modules() if name.endswith('downsample.0')]
    assert symbols.count('opa_conv3x3_act_f16') == len(dense3) and symbols.count('opa_gemm2_bias_act_f16') == len(down)
    pairs = 0 if net_name == 'resnet18' else len(down)        # a Bottleneck's conv3 goes into the pair's launch
    assert symbols.count('opa_gemm_bias_act_f16') == len(convs) - 1 - len(dense3) - len(down) - pairs


@pytest.mark.parametrize('net_name', sorted(NETWORKS))
def test_the_half_network_with_the_switch_off_runs_what_it_ran(traced, monkeypatch, net_name):
    """``F16`` off, the bfloat16 switches on: no ``_f16`` and no ``_bf16`` symbol; the trace is the parent commit's (its digest above)."""
    trace, cast = traced
    monkeypatch.setattr(fused, 'F16', False)
    monkeypatch.setattr(fused, 'CONV3_BF16', True)
    monkeypatch.setattr(fused, 'PAIR_BF16', True)
    off = _forward(trace, *cast(net_name, F16))
    assert not [launch for launch in off if '_f16(' in launch or '_bf16(' in launch]
    assert {launch.split('(')[0] for launch in off if not launch.startswith('miopen:')} == {'opa_bias_act'}
    digest, entries, miopen = PARENT_HALF_TRACES[net_name]
    assert (len(off), len([launch for launch in off if launch.startswith('miopen:')])) == (entries, miopen)
    assert _digest(off) == digest


@pytest.mark.parametrize('dtype', [torch.float32, BF], ids=['float32', 'bfloat16'])
def test_the_other_dtypes_trace_the_same_with_the_switch_on_and_off(traced, monkeypatch, dtype):
    trace, cast = traced
    for bf16_switches in (False, True):
        monkeypatch.setattr(fused, 'CONV3_BF16', bf16_switches)
        monkeypatch.setattr(fused, 'PAIR_BF16', bf16_switches)
        for net_name in sorted(NETWORKS):
            net, x = cast(net_name, dtype)
            monkeypatch.setattr(fused, 'F16', False)
            off = _forward(trace, net, x)
            monkeypatch.setattr(fused, 'F16', True)
            assert _forward(trace, net, x) == off and off and not [launch for launch in off if '_f16(' in launch]
