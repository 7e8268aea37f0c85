"""What ``fused.conv1x1_unit_x3`` and ``fused.dwconv_bias_act`` hand to the C ABI for the activation codes that take a parameter
(``ACT_LEAKY_RELU``, ``ACT_RELU6``), argument by argument, without a GPU -- recorded like ``test_launch_marshalling.py`` records its
cases (whose tensors and labels this uses, on the harness of ``abi_tables.py``) and compared with ``golden/launch_marshalling_actp.json``
(``golden/make_golden_abi.py launch_marshalling_actp``).  The new codes go to ``opa_gemm_unit_actp_f32x3`` / ``opa_dwconv_actp`` with the
parameter in its place (a float: recorded as it is); one case each with code 1 shows that every other code still goes to the symbol it
has always gone to, parameter or not."""
import ctypes
import itertools
import os

import torch
from torch import nn

from openpifpaf_amd import fused

import abi_tables as at
import test_launch_marshalling as tlm

GOLDEN = at.golden('launch_marshalling_actp')
F32, BF16 = torch.float32, torch.bfloat16
SYMBOLS = {'opa_gemm_unit_actp_f32x3', 'opa_dwconv_actp', 'opa_gemm_unit_act_f32x3', 'opa_dwconv_act', 'opa_dwconv_dilated_act'}


def cases():
    """-> {case id: (call, {label: input tensor}, derived operands after the call -> {label: tensor} or None, ``fused.X3_TERMS``)}"""
    out = {}

    def add(case_id, call, tensors, derived=None, terms=6):
        assert case_id not in out, case_id
        out[case_id] = (call, tensors, derived, terms)

    new_codes = ((fused.ACT_LEAKY_RELU, 0.01), (fused.ACT_LEAKY_RELU, 0.3), (fused.ACT_RELU6, 6.0), (fused.ACT_RELU6, 1.5))
    for terms in (6, 9):
        for layout in ('dense', 'slices'):
            unit = nn.Conv2d(72, 40, 1, bias=terms == 6)
            make = tlm._act if layout == 'dense' else tlm._slice
            ux, third = make(2, 72, 3, 5), make(2, 40, 3, 5) if layout == 'dense' else tlm._slice(2, 40, 3, 5, extra=10, start=4)
            for what, (act, param) in itertools.product(('alone', 'partner'), new_codes):
                if what == 'partner' and act == fused.ACT_RELU6:           # (no caller: MobileNetV2 has no shuffle)
                    continue
                kwargs = {} if what == 'alone' else {what: third}
                add('unit/terms%d/%s/%s/act%d/param%s' % (terms, layout, what, act, param),
                    lambda unit=unit, ux=ux, act=act, param=param, kwargs=kwargs: fused.conv1x1_unit_x3(unit, ux, act=act, act_param=param, **kwargs),
                    {'x': ux, what: third}, lambda unit=unit: tlm._cached_on(unit, 'w3', 'bias_padded'), terms)
            # code 1, with a parameter that nothing reads: the old symbol, the old arguments
            add('unit/terms%d/%s/partner/act1' % (terms, layout),
                lambda unit=unit, ux=ux, third=third: fused.conv1x1_unit_x3(unit, ux, partner=third, act=fused.ACT_RELU, act_param=0.01),
                {'x': ux, 'partner': third}, lambda unit=unit: tlm._cached_on(unit, 'w3', 'bias_padded'), terms)

    for dtype, layout in ((F32, 'dense'), (F32, 'slice'), (BF16, 'dense')):
        dx = tlm._act(2, 8, 7, 5, dtype) if layout == 'dense' else tlm._slice(2, 8, 7, 5, dtype)
        db = torch.zeros(8, dtype=dtype)
        for k, stride, dilation in ((3, 1, 1), (3, 2, 1), (5, 1, 1), (5, 2, 1), (7, 1, 1), (3, 1, 2), (5, 1, 4)):
            taps = torch.zeros((k * k, 8), dtype=dtype)
            for has_bias, cap in itertools.product((False, True), (6.0, 1.5)):
                add('dwconv/%s/%s/k%d/stride%d/dilation%d/bias%d/cap%s' % (dtype, layout, k, stride, dilation, has_bias, cap),
                    lambda dx=dx, taps=taps, bias=db if has_bias else None, k=k, stride=stride, dilation=dilation, cap=cap:
                    fused.dwconv_bias_act(dx, taps, bias, k, stride, act=fused.ACT_RELU6, act_param=cap, dilation=dilation),
                    dict(x=dx, w_taps=taps, bias=db))
            add('dwconv/%s/%s/k%d/stride%d/dilation%d/act1' % (dtype, layout, k, stride, dilation),
                lambda dx=dx, taps=taps, db=db, k=k, stride=stride, dilation=dilation:
                fused.dwconv_bias_act(dx, taps, db, k, stride, act=fused.ACT_RELU, act_param=6.0, dilation=dilation),
                dict(x=dx, w_taps=taps, bias=db))
    return out


def record_all():
    """-> {case id: [[symbol, [arguments]], ...]}"""
    return at.record_all(cases())


def test_every_launch_hands_over_what_the_golden_file_says():
    got = at.marshalling(cases(), GOLDEN)
    assert all(len(calls) == 1 for calls in got.values())
    assert {name for calls in got.values() for name, _ in calls} == SYMBOLS


def test_the_new_codes_take_the_new_symbols_and_no_other_code_does():
    got = record_all()
    for case_id, ((name, row),) in got.items():
        new = not case_id.endswith('/act1')
        if case_id.startswith('unit/'):
            assert name == ('opa_gemm_unit_actp_f32x3' if new else 'opa_gemm_unit_act_f32x3'), case_id
            if new:                                                    # ..., act, act_param, terms, stream
                act, param = int(case_id.split('/act')[1][0]), float(case_id.split('/param')[1])
                assert row[-4:-2] == [act, ctypes.c_float(param).value] and row[-2] == int(case_id.split('/terms')[1][0]), (case_id, row)
                assert row[6:8] == ['null', 0], (case_id, row)         # never a residual
            else:
                assert row[-3] == 1 and all(isinstance(v, (int, str)) for v in row), (case_id, row)
        else:
            if new:                                                    # ..., dtype, act, act_param, stream
                assert name == 'opa_dwconv_actp' and row[-3:-1] == [4, float(case_id.split('/cap')[1])], (case_id, row)
            else:
                k, d = int(case_id.split('/k')[1][0]), int(case_id.split('/dilation')[1][0])
                assert name == ('opa_dwconv_act' if k in (3, 5) and d == 1 else 'opa_dwconv_dilated_act') and row[-2] == 1, (case_id, row)
                assert all(isinstance(v, (int, str)) for v in row), (case_id, row)


def test_the_switches_are_read_once_and_ship_off():
    """``OPA_MBV2`` / ``OPA_UNIT_LEAKY`` are read when ``fused`` is imported, like the other switches, and default to off."""
    import subprocess
    import sys
    code = 'from openpifpaf_amd import fused; print(int(fused.MBV2), int(fused.UNIT_LEAKY))'
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for env, want in (({}, '0 0'), ({'OPA_MBV2': '1', 'OPA_UNIT_LEAKY': '1'}, '1 1')):
        clean = {k: v for k, v in os.environ.items() if k not in ('OPA_MBV2', 'OPA_UNIT_LEAKY')}
        proc = subprocess.run([sys.executable, '-c', code], env=dict(clean, **env), cwd=root, capture_output=True, text=True, timeout=300)
        assert proc.returncode == 0 and proc.stdout.split('\n')[-2] == want, (env, proc.stdout[-500:], proc.stderr[-500:])
    assert (fused.ACT_LEAKY_RELU, fused.ACT_RELU6) == (3, 4)
