"""Which launches the 3x3 convolutions of a ResNet make, switch by switch, in float32 and in bfloat16 -- every launched symbol of one
forward pass WITH its arguments (an address as null / non-null, every scalar as its value: bias passed or withheld, the residual inside
the kernel or in the pass, the ReLU flag, stride, dilation, terms and variant) and ``miopen:<module name>`` for every ``nn.Conv2d`` that
was called, traced on the CPU like ``test_unit_route_trace.py`` (a recorder in place of ``fused._launch``, tensors that say they are on
the GPU, the library reported as built, a current stream with a known handle that captures nothing) and compared with
``golden/resnet_route_trace.json``.  No GPU is touched and nothing is timed: ``FORCE_PICK`` is always set.

The golden file is the safety net of the change that gave the 3x3 convolutions of the ResNet blocks ONE route procedure
(``network._conv3x3``): it was recorded ONCE, from the tree as it stood before that change (commit 4fb740c, "bf16 MFMA kernels: one
shared tile header, main loop shared by two"), with ``PYTHONPATH=. python tests/test_resnet_route_trace.py``, and is never recorded
again: a route that launches something else than it did there, or the same with other arguments, is a change of behaviour, and this
test fails.

The networks: resnet18 and resnet50 with default options and with ``block5_dilation=2``, resnet50 with ``input_conv2_stride=2``,
resnext50, resnet18 with ``pool0_stride=2``; each optimized, in float32 and cast to bfloat16, at input ``[1, 3, 33, 25]``, across
``winograd.set_mode`` 'auto' / 'winograd' / 'conv' x ``FORCE_PICK`` 'x3' / 'conv' x ``X3_CONV3`` x ``GCONV`` x ``CONV3_BF16`` x
``winograd.X3``.  The parameters are plain CPU tensors, so the 1x1 GEMMs fall to MIOpen: they are not what the file guards."""
import copy
import itertools
import json
import os
import sys

import pytest
import torch
from torch import nn

from openpifpaf_amd import _lib, fused, network, winograd

import trunk_common as tc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'resnet_route_trace.json')
CL = torch.channels_last
DTYPES = {'float32': torch.float32, 'bfloat16': torch.bfloat16}
NETWORKS = {'resnet18': ('resnet18', {}), 'resnet50': ('resnet50', {}),
            'resnet18-dilated': ('resnet18', {'block5_dilation': 2}), 'resnet50-dilated': ('resnet50', {'block5_dilation': 2}),
            'resnet50-conv2': ('resnet50', {'input_conv2_stride': 2}), 'resnext50': ('resnext50', {}),
            'resnet18-pool': ('resnet18', {'pool0_stride': 2})}
SWITCHES = ((fused, 'X3_CONV3'), (fused, 'GCONV'), (fused, 'CONV3_BF16'), (winograd, 'X3'))
SYMBOLS = {'opa_conv3x3_winograd_f32x3', 'opa_conv3x3_winograd_f32', 'opa_conv3x3_f32x3', 'opa_conv3x3_dilated_f32x3',
           'opa_gconv3x3_bias_act_f32', 'opa_conv3x3_act_bf16', 'opa_gemm2_bias_act_f32x3', 'opa_conv_rows_f32x3',
           'opa_maxpool3x3_bias_act', 'opa_bias_act'}


class _OnDevice(torch.Tensor):
    is_cuda = True


def record_all(setattr_):
    """-> {case id: [launch, ...]}, a launch ``'symbol(arg, ...)'`` or ``'miopen:<module>'``; ``setattr_(object, name, value)``:
    monkeypatch's, so that everything is put back."""
    trace = []
    setattr_(fused, '_launch', lambda symbol, *args: trace.append('%s(%s)' % (symbol, ', '.join(map(str, args)))))
    setattr_(fused, '_ptr', lambda t: 'null' if t is None else 'ptr')
    empty = fused._empty_nhwc
    setattr_(fused, '_empty_nhwc', lambda *a, **kw: empty(*a, **kw).zero_().as_subclass(_OnDevice))
    setattr_(_lib, 'available', lambda: True)

    class Stream:
        cuda_stream = 0x7F00DEAD0040
    setattr_(torch.cuda, 'current_stream', lambda *a: Stream())
    setattr_(torch.cuda, 'is_current_stream_capturing', lambda: False)
    for name, value in (('X3_TERMS', 6), ('_CHOICE', {})):
        setattr_(fused, name, value)
    setattr_(winograd, '_mode', winograd.get_mode())            # (put back afterwards, whatever set_mode left)
    result = {}
    for net_name, (config, options) in NETWORKS.items():
        torch.manual_seed(5)
        net = network.optimize_for_inference_(copy.deepcopy(tc.randomize_(network.Resnet(config, **options), 5)))
        for dtype_name, dtype in DTYPES.items():
            cast = copy.deepcopy(net).to(dtype)
            for name, m in cast.named_modules():
                if isinstance(m, nn.Conv2d):
                    m.register_forward_hook(lambda mod, args, out, name=name: trace.append('miopen:' + name))
            x = torch.randn((1, 3, 33, 25), generator=tc.gen(7)).to(dtype).contiguous(memory_format=CL).as_subclass(_OnDevice)
            for mode, pick, values in itertools.product(('auto', 'winograd', 'conv'), ('x3', 'conv'),
                                                        itertools.product((False, True), repeat=len(SWITCHES))):
                winograd.set_mode(mode)
                setattr_(fused, 'FORCE_PICK', pick)
                for (mod, name), on in zip(SWITCHES, values):
                    setattr_(mod, name, on)
                del trace[:]
                with torch.no_grad():
                    cast(x)
                case = '%s/%s/wino-%s/pick-%s/%s' % (net_name, dtype_name, mode, pick,
                                                     '/'.join('%s%d' % (s[1], on) for s, on in zip(SWITCHES, values)))
                result[case] = list(trace)
    return result


def test_every_route_launches_what_it_launched_before(monkeypatch):
    with open(GOLDEN) as f:
        golden = json.load(f)
    golden = {case: [golden['launches'][j] for j in golden['traces'][i]] for case, i in golden['cases'].items()}
    got = record_all(monkeypatch.setattr)
    assert sorted(got) == sorted(golden)
    different = {case: [(a, b) for a, b in itertools.zip_longest(got[case], golden[case]) if a != b][:3]
                 for case in got if got[case] != golden[case]}
    assert not different, (len(different), sorted(different.items())[:3])
    # the traces show something: every kernel a 3x3 convolution can go to, the launches around them, and MIOpen
    seen = {launch.split('(')[0] for trace in got.values() for launch in trace}
    assert SYMBOLS <= seen, SYMBOLS - seen
    assert any(s.startswith('miopen:') for s in seen)


if __name__ == '__main__':                         # records the golden file: ONCE, at the commit the docstring names
    if os.path.exists(GOLDEN):
        sys.exit('golden/resnet_route_trace.json exists: it is recorded once, before the change it guards, and never afterwards')
    with pytest.MonkeyPatch.context() as patch:
        recorded = record_all(patch.setattr)
    # unit_route_trace.json's format (distinct traces, case -> index); a trace lists indices into the distinct launches
    launches = sorted({launch for t in recorded.values() for launch in t})
    index = {launch: j for j, launch in enumerate(launches)}
    traces = sorted({tuple(index[launch] for launch in t) for t in recorded.values()})
    with open(GOLDEN, 'w') as f:
        f.write('{"launches": [\n' + ',\n'.join(json.dumps(launch) for launch in launches) + '\n],\n"traces": [\n')
        f.write(',\n'.join(json.dumps(list(t)) for t in traces) + '\n],\n"cases": {\n')
        f.write(',\n'.join('%s: %d' % (json.dumps(case), traces.index(tuple(index[launch] for launch in recorded[case])))
                           for case in sorted(recorded)) + '\n}}\n')
    print('%d cases, %d different traces, %d different launches -> %s' % (len(recorded), len(traces), len(launches), GOLDEN))
