"""The 16-bit head route on the host: the switch ``fused.HEAD16`` (OPA_HEAD16), what ``fused.head_conv_fields16_supported`` answers,
the derived operands, and the launches of whole networks cast to bfloat16 and float16, traced on the CPU with the technique of
``test_f16_host.py`` (a recorder in place of ``fused._launch``, tensors that say they are on the GPU, the library reported as built, a
forward hook on every ``nn.Conv2d`` that records ``miopen:<module name>``).  No GPU is touched and nothing is timed.

Every test sets ``fused.HEAD16`` through monkeypatch, which refuses to set an attribute that does not exist: without the feature every
test of this file fails."""
import copy

import pytest
import torch
from torch import nn

from openpifpaf_amd import _lib, fused, network, winograd

import head16_common as hc
import trunk_common as tc

CL = torch.channels_last
F16, BF = torch.float16, torch.bfloat16
SYMBOLS = {BF: 'opa_head_conv_fields_bf16', F16: 'opa_head_conv_fields_f16'}
TRUNK_SWITCHES = ('F16', 'CONV3_BF16', 'PAIR_BF16', 'STEM7_BF16', 'GCONV_BF16', 'UNIT_BF16')


class _OnDevice(torch.Tensor):
    is_cuda = True


def _dev(t):
    return t.as_subclass(_OnDevice)


def _image(b, c, h, w, dt, seed=0, offset=0):
    """A channels-last ``[b, c, h, w]`` of ``dt`` that says it is on the GPU; ``offset``: elements between a 16-byte boundary and its
    first element."""
    flat = torch.randn(b * h * w * c + 8, generator=tc.gen(seed)).to(dt)
    assert flat.data_ptr() % 16 == 0
    return _dev(flat[offset:offset + b * h * w * c].view(b, h, w, c).permute(0, 3, 1, 2))


def _conv(c_in, c_out, dt, k=1, **kw):
    return nn.Conv2d(c_in, c_out, k, **kw).to(dt).requires_grad_(False)


@pytest.fixture
def built(monkeypatch):
    monkeypatch.setattr(_lib, 'available', lambda: True)
    for name in TRUNK_SWITCHES:
        monkeypatch.setattr(fused, name, False)
    monkeypatch.setattr(fused, 'HEAD16', True)
    return monkeypatch


# ---- the predicate ---------------------------------------------------------------------------------------------------------------------

def _case(dt, k=64):
    """A Cif head of 3 fields with upsampling: N = 3 * 5 * 4 = 60 output channels"""
    return dict(conv=_conv(k, 60, dt), x=_image(2, k, 5, 3, dt), meta=hc.meta('cif', 3, 2))


def _with(case, **changes):
    return dict(case, **changes)


def _requires_grad(conv):
    return copy.deepcopy(conv).requires_grad_(True)


@pytest.mark.parametrize('dt', [BF, F16], ids=['bfloat16', 'float16'])
def test_a_16_bit_head_is_taken_with_the_switch_on_whatever_the_other_switches_say(built, dt):
    case = _case(dt)
    assert fused.head_conv_fields16_supported(**case) and fused.head_conv_fields16_supported(training=False, **case)
    for meta in (hc.meta('caf', 2, 1), hc.meta('cifdet', 4, 2)):                        # 16 and 96 output channels
        n = meta.n_fields * hc.n_components(meta) * meta.upsample_stride ** 2
        assert fused.head_conv_fields16_supported(_conv(128, n, dt), _image(1, 128, 1, 300, dt), meta)      # no limit on the row width
    for name in TRUNK_SWITCHES:
        built.setattr(fused, name, True)
    assert fused.head_conv_fields16_supported(**case)
    built.setattr(fused, 'HEAD16', False)
    assert not fused.head_conv_fields16_supported(**case)                               # ... and declined with it off, whatever they say
    built.setattr(fused, 'HEAD16', True)
    built.setattr(_lib, 'available', lambda: False)
    assert not fused.head_conv_fields16_supported(**case)
    built.setattr(_lib, 'available', lambda: True)
    built.setattr(fused, 'HEAD16_DECLINED', frozenset({(64, 60, 2)}))                  # a layer measured slower: (k, n, upsample)
    assert not fused.head_conv_fields16_supported(**case)
    assert fused.head_conv_fields16_supported(**_case(dt, 128))


def _spoilt(case, dt):
    other = BF if dt == F16 else F16
    x, conv = case['x'], case['conv']
    float_bias = copy.deepcopy(conv)
    float_bias.bias = nn.Parameter(conv.bias.detach().float(), requires_grad=False)
    return [
        ('training', _with(case, training=True)),
        ('a float32 x', _with(case, x=_dev(x.float()))),
        ('a float32 head', _with(case, x=_dev(x.float()), conv=_conv(64, 60, torch.float32))),
        ('a weight of the other 16-bit type', _with(case, conv=_conv(64, 60, other))),
        ('float32 parameters (autocast keeps them)', _with(case, conv=_conv(64, 60, torch.float32))),
        ('a float32 bias', _with(case, conv=float_bias)),
        ('x of the other 16-bit type', _with(case, x=_image(2, 64, 5, 3, other))),
        ('x not channels-last (NCHW)', _with(case, x=_dev(x.contiguous()))),
        ('x of three dimensions', _with(case, x=_dev(x[0]))),
        ('x misaligned', _with(case, x=_image(2, 64, 5, 3, dt, offset=1))),
        ('other input channels', _with(case, x=_image(2, 128, 5, 3, dt))),
        ('an empty row', _with(case, x=_image(2, 64, 0, 3, dt))),
        ('in_channels 1392', _with(case, conv=_conv(1392, 60, dt), x=_image(2, 1392, 5, 3, dt))),
        ('upsample_stride 3', _with(case, conv=_conv(64, 3 * 5 * 9, dt), meta=hc.meta('cif', 3, 3))),
        ('a convolution without bias', _with(case, conv=_conv(64, 60, dt, bias=False))),
        ('a 3x3 convolution', _with(case, conv=_conv(64, 60, dt, k=3, padding=1))),
        ('stride 2', _with(case, conv=_conv(64, 60, dt, stride=2))),
        ('padding', _with(case, conv=_conv(64, 60, dt, padding=1))),
        ('groups', _with(case, conv=_conv(64, 60, dt, groups=2))),
        ('output channels that are not the meta\'s', _with(case, meta=hc.meta('cif', 4, 2))),
        ('another meta\'s component count', _with(case, meta=hc.meta('caf', 3, 2))),
        ('a module that is no convolution', _with(case, conv=nn.Linear(64, 60).to(dt))),
    ]


@pytest.mark.parametrize('dt', [BF, F16], ids=['bfloat16', 'float16'])
def test_what_spoils_a_case_each_by_itself(built, dt):
    case = _case(dt)
    spoilt = _spoilt(case, dt)
    assert len(spoilt) >= 20
    with torch.no_grad():
        assert fused.head_conv_fields16_supported(**case)
        for what, bad in spoilt:
            assert not fused.head_conv_fields16_supported(**bad), what
    followed = [('x that autograd follows', _with(case, x=_dev(case['x'].detach().clone()).requires_grad_(True))),
                ('parameters that autograd follows', _with(case, conv=_requires_grad(case['conv'])))]
    with torch.enable_grad():                                                           # requires_grad under grad mode
        assert fused.head_conv_fields16_supported(**case)
        for what, bad in followed:
            assert not fused.head_conv_fields16_supported(**bad), what
    with torch.no_grad():                                                               # nothing is followed without grad mode
        for what, bad in followed:
            assert fused.head_conv_fields16_supported(**bad), what
    with built.context() as m:
        m.setattr(torch, 'is_autocast_enabled', lambda *a: True)
        assert not fused.head_conv_fields16_supported(**case)
    assert fused.head_conv_fields16_supported(**case)


def test_the_switch_reads_opa_head16_and_ships_off():
    import os
    import subprocess
    import sys
    code = 'from openpifpaf_amd import fused; print(fused.HEAD16, fused.F16, fused.PAIR_BF16, sorted(fused.HEAD16_DECLINED))'
    env = {k: v for k, v in os.environ.items() if not k.startswith('OPA_')}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for value, want in ((None, 'False False False []'), ('1', 'True False False []'), ('0', 'False False False []')):
        e = dict(env, **({} if value is None else {'OPA_HEAD16': value}))
        out = subprocess.run([sys.executable, '-c', code], env=e, cwd=root, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and out.stdout.strip() == want, (value, out.stdout, out.stderr[-2000:])
    assert set(SYMBOLS.values()) <= set(_lib.SYMBOLS)


# ---- the derived operands ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dt', [BF, F16], ids=['bfloat16', 'float16'])
def test_the_derived_operands_are_padded_and_follow_the_parameters(built, dt):
    conv = _conv(64, 60, dt)

    def check():
        wp, bp = fused.head16_operands_of(conv)
        assert wp.dtype == dt and tuple(wp.shape) == (64, 64) and wp.is_contiguous() and bp.dtype == torch.float32 and tuple(bp.shape) == (64,)
        assert torch.equal(wp[:60], conv.weight.detach().reshape(60, 64)) and not wp[60:].any()
        assert torch.equal(bp[:60], conv.bias.detach().float()) and not bp[60:].any()
        return wp, bp
    first = check()
    assert fused.head16_operands_of(conv)[0] is first[0] and fused.head16_operands_of(conv)[1] is first[1]       # cached
    old = [t.clone() for t in first]
    with torch.no_grad():                               # an in-place weight update: the KEPT tensors are overwritten in place (an
        conv.weight.mul_(2.0)                           # address a HIP graph holds sees the new weights)
    second = check()
    assert second[0] is first[0] and second[1] is first[1] and torch.equal(second[0], old[0] * 2)
    old = [t.clone() for t in second]
    with torch.no_grad():                               # ... and of the bias alone
        conv.bias.add_(1.0)
    third = check()
    assert third[1] is second[1] and not torch.equal(third[1], old[1])
    old = [t.clone() for t in third]
    conv.load_state_dict({'weight': torch.randn(60, 64, 1, 1, generator=tc.gen(9)).to(dt), 'bias': torch.randn(60, generator=tc.gen(10)).to(dt)})
    fourth = check()
    assert fourth[0] is third[0] and not torch.equal(fourth[0], old[0])
    conv.to(torch.float32).to(dt)                       # a round trip: new tensors of equal values
    fifth = check()
    assert fifth[0] is not fourth[0] and torch.equal(fifth[0], fourth[0]) and torch.equal(fifth[1], fourth[1])


# ---- the launches of a whole network --------------------------------------------------------------------------------------------------

@pytest.fixture
def traced(monkeypatch):
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
    for name, value in (('X3_TERMS', 6), ('_CHOICE', {}), ('FORCE_PICK', 'conv'), ('GCONV', False), ('HEAD16', False)) + tuple(
            (name, False) for name in TRUNK_SWITCHES):
        monkeypatch.setattr(fused, name, value)
    monkeypatch.setattr(winograd, '_mode', winograd.get_mode())
    base = {}

    def cast(net_name, dtype):
        if net_name not in base:
            base[net_name] = network.optimize_for_inference_(tc.randomize_(network.factory(net_name, seed=5), 5))
        net = copy.deepcopy(base[net_name]).to(dtype).requires_grad_(False)
        for name, m in net.named_modules():
            if isinstance(m, nn.Conv2d):
                m.register_forward_hook(lambda mod, args, out, name=name: trace.append('miopen:' + name))
        x = torch.randn((1, 3, 33, 25), generator=tc.gen(7)).to(dtype).contiguous(memory_format=CL).as_subclass(_OnDevice)
        return net, x
    return trace, cast


def _forward(trace, net, x):
    del trace[:]
    with torch.no_grad():
        out = net(x)
    return list(trace), out


def _trunk_on(monkeypatch, dtype, on=True):
    """The 16-bit trunk routes of ``dtype`` on: the trunk's output is then the last kernel's, dense channels-last."""
    for name in (('F16',) if dtype == F16 else ('CONV3_BF16', 'PAIR_BF16', 'STEM7_BF16')):
        monkeypatch.setattr(fused, name, on)


@pytest.mark.parametrize('dtype', [BF, F16], ids=['bfloat16', 'float16'])
@pytest.mark.parametrize('net_name', ['resnet18', 'resnet50'])
def test_a_16_bit_resnet_launches_the_new_symbol_once_per_head(traced, monkeypatch, net_name, dtype):
    trace, cast = traced
    net, x = cast(net_name, dtype)
    _trunk_on(monkeypatch, dtype)
    off, _ = _forward(trace, net, x)
    heads_off = [launch for launch in off if launch.startswith(('miopen:head_nets.', 'opa_head'))]
    assert [launch.split('(')[0] for launch in heads_off] == ['miopen:head_nets.0.conv', 'opa_head_epilogue', 'miopen:head_nets.1.conv', 'opa_head_epilogue']
    monkeypatch.setattr(fused, 'HEAD16', True)
    on, out = _forward(trace, net, x)
    k = net.base_net.out_features
    assert k == (512 if net_name == 'resnet18' else 2048)
    heads_on = [launch for launch in on if launch.startswith(('miopen:head_nets.', 'opa_head'))]
    # x, w, bias, out, batch, hc, wc, k, n_fields, n_components, upsample, confidences, vectors, offset mask, scales (33 x 25 at stride 16: 3 x 2)
    assert heads_on == ['%s(ptr, ptr, ptr, ptr, 1, 3, 2, %d, 17, 5, 2, 1, 1, 1, 1)' % (SYMBOLS[dtype], k),
                        '%s(ptr, ptr, ptr, ptr, 1, 3, 2, %d, 19, 8, 2, 1, 2, 3, 2)' % (SYMBOLS[dtype], k)]
    assert not [launch for launch in on if 'opa_head_epilogue' in launch or launch.startswith('miopen:head_nets.')]
    assert [launch for launch in on if launch not in heads_on] == [launch for launch in off if launch not in heads_off]      # the trunk as it was
    assert [tuple(f.shape) for f in out] == [(1, 17, 5, 5, 3), (1, 19, 8, 5, 3)] and all(f.dtype == torch.float32 for f in out)
    monkeypatch.setattr(fused, 'HEAD16', False)
    assert _forward(trace, net, x)[0] == off


@pytest.mark.parametrize('dtype', [BF, F16, torch.float32], ids=['bfloat16', 'float16', 'float32'])
def test_what_the_route_does_not_take_launches_what_it_launched(traced, monkeypatch, dtype):
    """shufflenetv2k16 (1392 features: no multiple of 64) in every dtype, a float32 ResNet, and a 16-bit ResNet in training mode keep
    exactly the launches they have with the switch off."""
    trace, cast = traced
    cases = [cast('shufflenetv2k16', dtype)]
    if dtype == torch.float32:
        cases.append(cast('resnet18', dtype))
    else:
        monkeypatch.setattr(fused, 'UNIT_BF16', True)                                   # (a bfloat16 k16 head: the unit mode's)
        net, x = cast('resnet18', dtype)
        net.head_nets.train()
        cases.append((net, x))
    for net, x in cases:
        monkeypatch.setattr(fused, 'HEAD16', False)
        off, _ = _forward(trace, net, x)
        monkeypatch.setattr(fused, 'HEAD16', True)
        on, _ = _forward(trace, net, x)
        assert on == off and off and not [launch for launch in on if launch.startswith('opa_head_conv_fields')]
        assert len([launch for launch in on if launch.startswith('miopen:head_nets.') or launch.startswith('opa_gemm_unit_actp_bf16')]) >= 2
