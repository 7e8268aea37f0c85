"""Which launches a ShuffleNetV2K and a ``CompositeField4`` head make, switch by switch, in float32 and in bfloat16 -- the sequence of
launched symbols of one forward pass, traced on the CPU with the ``launches`` recorder of ``test_unit_bf16_host.py`` (a recorder in place
of ``fused._launch``, outputs that say they are on the GPU, the library reported as built; a current stream with a known handle as in
``test_launch_marshalling.py``) and compared with
``golden/unit_route_trace.json``.  No GPU is touched.

The golden file is the safety net of the change that gave the unit mode ONE route for both element types: it was recorded ONCE, from
the tree as it stood before that change (commit f08ae87, "bfloat16 ShuffleNetV2K trunks: unit-mode 1x1 GEMM on the bf16 MFMA"), with
``PYTHONPATH=. python tests/test_unit_route_trace.py``, and is never recorded again: a route that launches something else than it did there is a
change of behaviour, and this test fails.

The trunk: the tiny ShuffleNetV2K of ``test_unit_bf16_host.py`` (``config=TINY``), optimized, at input ``[2, 3, 33, 25]``, across
dtype x ``leaky_relu`` x ``layer_norm`` None / 'group' x ``conv5_as_stage`` x ``UNIT_BF16`` x ``UNIT_LEAKY`` x ``GN`` x ``FORCE_PICK``
'x3' / 'conv' x autocast reported off / on.  ``TINY`` has stages of 58 channels, which no ``GroupNorm`` of four groups divides: that
network cannot be built and is left out; the group-norm network is the tiny one of ``test_shufflenetv2k_norms_host.py`` instead.
The head: K = 24 and K = 64 input channels in both dtypes, ``X3_HEAD`` on / off, across the same switches."""
import copy
import itertools
import json
import os
import sys

import pytest
import torch

from openpifpaf_amd import _lib, fused, headmeta, network

import trunk_common as tc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'unit_route_trace.json')
CL = torch.channels_last
DTYPES = {'float32': torch.float32, 'bfloat16': torch.bfloat16}
CONFIGS = {'tiny': ([2, 1, 1], [24, 116, 64, 256, 24]), 'tiny-group': ([1, 1, 1], [24, 232, 64, 256, 24])}
SWITCHES = ('UNIT_BF16', 'UNIT_LEAKY', 'GN')


class _OnDevice(torch.Tensor):
    is_cuda = True


def _on_device(shape, dtype, seed):
    return torch.randn(shape, generator=tc.gen(seed)).to(dtype).contiguous(memory_format=CL).as_subclass(_OnDevice)


def _flags(n):
    return itertools.product((False, True), repeat=n)


def _trace(symbols, run):
    """The symbols ``run()`` launched; behind them the name of what it raised, if it raised (a head's epilogue has no device here)."""
    del symbols[:]
    try:
        with torch.no_grad():
            run()
    except Exception as exc:                        # noqa: BLE001
        return list(symbols) + ['raised ' + type(exc).__name__]
    return list(symbols)


def record_all(setattr_):
    """-> {case id: [launched symbols]}; ``setattr_(object, name, value)``: monkeypatch's, so that everything is put back."""
    symbols = []
    setattr_(fused, '_launch', lambda symbol, *args: symbols.append(symbol))
    empty = fused._empty_nhwc
    setattr_(fused, '_empty_nhwc', lambda *a, **kw: empty(*a, **kw).zero_().as_subclass(_OnDevice))
    setattr_(_lib, 'available', lambda: True)

    class Stream:                                   # (the group-norm route keeps its workspace per stream: a handle, with or without a GPU)
        cuda_stream = 0x7F00DEAD0040
    setattr_(torch.cuda, 'current_stream', lambda *a: Stream())
    for name, value in (('X3_UNIT', True), ('X3_TERMS', 6), ('X3_HEAD', True), ('STEM', False), ('_CHOICE', {})):
        setattr_(fused, name, value)
    autocast_off = torch.is_autocast_enabled
    result = {}

    def switch_cases():
        for values in _flags(len(SWITCHES)):
            for name, on in zip(SWITCHES, values):
                setattr_(fused, name, on)
            for pick, autocast in itertools.product(('x3', 'conv'), (False, True)):
                setattr_(fused, 'FORCE_PICK', pick)
                setattr_(torch, 'is_autocast_enabled', (lambda *a: True) if autocast else autocast_off)
                yield '/'.join('%s%d' % (n, v) for n, v in zip(SWITCHES, values)) + '/pick-%s/autocast%d' % (pick, autocast)
        setattr_(torch, 'is_autocast_enabled', autocast_off)

    # ---- the trunk ------------------------------------------------------------------------------------------------------------------
    for (config, layer_norm), leaky, conv5_as_stage in itertools.product((('tiny', None), ('tiny', 'group'), ('tiny-group', 'group')), (False, True), (False, True)):
        torch.manual_seed(5)
        try:
            net = network.ShuffleNetV2K('tiny', config=CONFIGS[config], leaky_relu=leaky, layer_norm=layer_norm, conv5_as_stage=conv5_as_stage)
        except ValueError:                          # (a GroupNorm whose groups do not divide its channels)
            assert (config, layer_norm) == ('tiny', 'group')
            continue
        net = network.optimize_for_inference_(copy.deepcopy(tc.randomize_(net, 5)))
        for dtype_name, dtype in DTYPES.items():
            cast, x = copy.deepcopy(net).to(dtype), _on_device((2, 3, 33, 25), dtype, 7)
            head = 'trunk/%s/%s/leaky%d/norm-%s/conv5-stage%d/' % (config, dtype_name, leaky, layer_norm, conv5_as_stage)
            for case in switch_cases():
                result[head + case] = _trace(symbols, lambda: cast(x))

    # ---- the head -------------------------------------------------------------------------------------------------------------------
    meta = headmeta.Cif('cif', 'test', keypoints=['a', 'b', 'c'], sigmas=[0.1, 0.1, 0.1], pose=None, draw_skeleton=[])
    meta.upsample_stride = 2                        # 3 x 5 x 4 = 60 output channels
    for k, (dtype_name, dtype), x3_head in itertools.product((24, 64), DTYPES.items(), (False, True)):
        torch.manual_seed(6)
        field, x = network.CompositeField4(meta, k).to(dtype).eval(), _on_device((2, k, 3, 2), dtype, 8)
        setattr_(fused, 'X3_HEAD', x3_head)
        for case in switch_cases():
            result['head/k%d/%s/X3_HEAD%d/%s' % (k, dtype_name, x3_head, case)] = _trace(symbols, lambda: field(x))
    return result


def test_every_route_launches_what_it_launched_before(monkeypatch):
    with open(GOLDEN) as f:
        golden = json.load(f)
    golden = {case: golden['traces'][i] for case, i in golden['cases'].items()}
    got = record_all(monkeypatch.setattr)
    assert sorted(got) == sorted(golden)
    different = {case: (got[case], golden[case]) for case in got if got[case] != golden[case]}
    assert not different, (len(different), sorted(different.items())[:3])
    # the traces show something: every unit-mode symbol, the routes around them, and torch alone
    seen = {s for trace in got.values() for s in trace}
    assert {'opa_gemm_unit_act_f32x3', 'opa_gemm_unit_actp_f32x3', 'opa_gemm_unit_actp_bf16', 'opa_gemm_bias_act_f32x3', 'opa_groupnorm_actp',
            'opa_channel_interleave'} <= seen, seen
    assert [] in got.values() or any(not [s for s in t if s.startswith('opa_gemm')] for t in got.values())


if __name__ == '__main__':                         # records the golden file: ONCE, at the commit the docstring names
    if os.path.exists(GOLDEN):
        sys.exit('golden/unit_route_trace.json exists: it is recorded once, before the change it guards, and never afterwards')
    with pytest.MonkeyPatch.context() as patch:
        recorded = record_all(patch.setattr)
    traces = sorted({tuple(t) for t in recorded.values()})
    with open(GOLDEN, 'w') as f:
        f.write('{"traces": [\n' + ',\n'.join(json.dumps(list(t)) for t in traces) + '\n],\n"cases": {\n')
        f.write(',\n'.join('%s: %d' % (json.dumps(case), traces.index(tuple(recorded[case]))) for case in sorted(recorded)) + '\n}}\n')
    print('%d cases, %d different traces -> %s' % (len(recorded), len(traces), GOLDEN))
