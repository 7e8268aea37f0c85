"""Every status and message with which the four float16 entry points of the trunk (``csrc/capi_trunk.hip``: ``opa_gemm_bias_act_f16``,
``opa_gemm_pro_bias_act_f16``, ``opa_conv3x3_act_f16``, ``opa_gemm2_bias_act_f16``) answer a call they do not launch: each shares
its bfloat16 twin's check function, so each must answer every row of the TWIN's table -- ``table()`` of
``test_capi_refusals_conv3x3_bf16.py`` and ``test_capi_refusals_gemm2_bf16.py``, the plain GEMM's rows of ``test_capi_refusals.py`` --
with the twin's status and the twin's message under its own name.  What the twins answer is not recorded again: it is read from
their committed golden files (``golden/capi_refusals_conv3x3_bf16.json``, ``golden/capi_refusals.json``) and, for the pair kernel,
from the messages written beside its rows.  On the harness of ``abi_tables.py``: one fresh child process that sees no GPU."""
import json

import abi_tables as at
import test_capi_refusals as plain
import test_capi_refusals_conv3x3_bf16 as conv3
import test_capi_refusals_gemm2_bf16 as pair

TWINS = {'opa_gemm_bias_act_bf16': 'opa_gemm_bias_act_f16', 'opa_gemm_pro_bias_act_bf16': 'opa_gemm_pro_bias_act_f16',
         'opa_conv3x3_act_bf16': 'opa_conv3x3_act_f16', 'opa_gemm2_bias_act_bf16': 'opa_gemm2_bias_act_f16'}
OPA_ERR_INVALID_ARGUMENT = 1
STATUSES = {OPA_ERR_INVALID_ARGUMENT}                # of a refused row


def _renamed(row_id, symbol):
    assert row_id.startswith(symbol + '(')
    return TWINS[symbol] + row_id[len(symbol):]


def twin_rows():
    """-> {the twin's row id: (kind, the twin's symbol, arguments)} of the four twins"""
    rows = {row_id: row for row_id, row in plain.table().items() if row[1] in ('opa_gemm_bias_act_bf16', 'opa_gemm_pro_bias_act_bf16')}
    rows.update(conv3.table())
    rows.update(pair.table()[0])
    assert {row[1] for row in rows.values()} == set(TWINS)
    return rows


def table():
    """-> {row id: (kind, symbol, arguments)}: the twins' rows with the float16 symbol in their place"""
    return {_renamed(row_id, symbol): (kind, TWINS[symbol], args) for row_id, (kind, symbol, args) in twin_rows().items()}


def twin_answers():
    """-> {the twin's row id: [status, message]} from the committed golden files and the pair kernel's written messages"""
    want = {}
    for path in (plain.GOLDEN, conv3.GOLDEN):
        with open(path) as f:
            want.update(json.load(f)['rows'])
    rows, expected = pair.table()
    for row_id, (kind, symbol, _) in rows.items():
        want[row_id] = [OPA_ERR_INVALID_ARGUMENT, symbol + ': ' + expected[row_id]] if kind == 'refused' else [0, '']
    return want


def test_every_row_is_answered_as_the_twin_answers_it():
    t = table()
    got = at.refusals(__file__, t, STATUSES)['rows']
    assert sorted(got) == sorted(t) and len({symbol for _, symbol, _ in t.values()}) == 4
    want = twin_answers()
    refused = 0
    for row_id, (kind, symbol, _) in twin_rows().items():
        status, message = want[row_id]
        assert message == '' or message.startswith(symbol + ': ')
        mine = [status, TWINS[symbol] + message[len(symbol):] if message else '']
        assert got[_renamed(row_id, symbol)] == mine, (row_id, got[_renamed(row_id, symbol)], mine)
        assert (kind == 'refused') == (status == OPA_ERR_INVALID_ARGUMENT) and (kind == 'empty') == (status == 0)
        refused += kind == 'refused'
    assert refused > 150 and len(t) - refused > 30                # every check of every twin, and the empty calls behind them


def test_the_argument_lists_are_the_twins():
    """Header and binding: each new entry point is declared with its twin's argument list and bound with its twin's types."""
    import os
    import re
    from openpifpaf_amd import _lib
    with open(os.path.join(os.path.dirname(at.HERE), 'include', 'openpifpaf_amd.h')) as f:
        header = f.read()
    for twin, mine in TWINS.items():
        declarations = [re.sub(r'\s+', ' ', header.split('int ' + s + '(')[1].split(');')[0]) for s in (twin, mine)]
        assert declarations[0] == declarations[1], (twin, declarations)
        assert _lib.SYMBOLS[mine] == _lib.SYMBOLS[twin]


if __name__ == '__main__':
    at.child(table())
