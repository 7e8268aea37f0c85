"""Every status and message with which the float16 twins ``opa_gemm_unit_actp_f16`` and ``opa_dwconv_actp_f16`` (``csrc/capi_trunk.hip``:
the unit mode of the 16-bit GEMM and the depthwise stencil for a network cast with ``.half()``) answer a call they do not launch, against
``golden/capi_refusals_unit_f16.json`` (``golden/make_golden_abi.py capi_refusals_unit_f16``).

The rows are the twins' originals': every row of ``test_capi_refusals_unit_bf16.py``'s table under the float16 symbol, and every row that
``test_capi_refusals_actp.py`` has for ``opa_dwconv_actp`` without the ``dtype`` argument, which the twin does not take (the rows that
change it have no counterpart).  Built and run on the harness of ``abi_tables.py``: one fresh child process that sees no GPU.  The
twins share their originals' check functions, so every answer must be the original's under the twin's name -- compared with the
originals' golden files row by row."""
import json

import abi_tables as at
import test_capi_refusals_actp as actp
import test_capi_refusals_unit_bf16 as unit_bf16

GOLDEN = at.golden('capi_refusals_unit_f16')
TWINS = {'opa_gemm_unit_actp_bf16': 'opa_gemm_unit_actp_f16', 'opa_dwconv_actp': 'opa_dwconv_actp_f16'}
ORIGINALS = {'opa_gemm_unit_actp_bf16': 'capi_refusals_unit_bf16', 'opa_dwconv_actp': 'capi_refusals_actp'}
DTYPE_INDEX = 13                                     # of ``dtype`` in opa_dwconv_actp's argument list
OPA_ERR_INVALID_ARGUMENT = 1
STATUSES = {OPA_ERR_INVALID_ARGUMENT}                # of a refused row


def _twin_rows():
    """-> {the twin's row id: (the original's row id, kind, the twin's symbol, the twin's arguments)}"""
    out = {}
    originals = dict(unit_bf16.table())
    originals.update({row_id: row for row_id, row in actp.table().items() if row[1] == 'opa_dwconv_actp'})
    for row_id, (kind, symbol, args) in originals.items():
        assert row_id.startswith(symbol) and symbol in TWINS, row_id
        if symbol == 'opa_dwconv_actp':
            if 'dtype=' in row_id:
                continue
            assert args[DTYPE_INDEX] == 0 and len(args) == 17
            args = args[:DTYPE_INDEX] + args[DTYPE_INDEX + 1:]
        out[TWINS[symbol] + row_id[len(symbol):]] = (row_id, kind, TWINS[symbol], args)
    return out


def table():
    """-> {row id: (kind, symbol, arguments)}"""
    return {row_id: (kind, symbol, args) for row_id, (_, kind, symbol, args) in _twin_rows().items()}


def refusals():
    """The table run and checked -> what the golden file holds"""
    return at.refusals(__file__, table(), STATUSES)


def test_refusals_match_the_golden_table():
    got = refusals()
    assert {symbol for _, symbol, _ in table().values()} == set(TWINS.values())
    with open(GOLDEN) as f:
        at.assert_same(got['rows'], json.load(f)['rows'])


def test_the_table_has_the_originals_rows():
    rows = _twin_rows()
    gemm = [r for r in rows if r.startswith('opa_gemm_unit_actp_f16')]
    stencil = [r for r in rows if r.startswith('opa_dwconv_actp_f16')]
    assert len(gemm) == len(unit_bf16.table()) and len(gemm) > 100
    dw = [r for r, row in actp.table().items() if row[1] == 'opa_dwconv_actp']
    assert len(stencil) == len(dw) - 4 and len(stencil) > 60               # (dtype -1, 1, 3, and 2 with too many rows)
    assert {kind for _, kind, _, _ in rows.values()} == {'refused', 'empty'}


def test_every_answer_is_the_originals_under_the_twins_name():
    """The same checks in the same order with the same words: per row the status and the message of the original's golden file, the
    symbol's name replaced."""
    with open(GOLDEN) as f:
        rows = json.load(f)['rows']
    golden = {}
    for symbol, name in ORIGINALS.items():
        with open(at.golden(name)) as f:
            golden[symbol] = json.load(f)['rows']
    twins = _twin_rows()
    assert sorted(twins) == sorted(rows)
    for row_id, (original_id, _, twin, _) in twins.items():
        original = [s for s, t in TWINS.items() if t == twin][0]
        status, message = golden[original][original_id]
        assert rows[row_id] == [status, message.replace(original, twin)], row_id
    assert rows['opa_gemm_unit_actp_f16(a=P+2)'] == [1, 'opa_gemm_unit_actp_f16: a_dev / partner_dev / residual_dev must be 4-B, '
                                                        'w_dev / bias_dev / out_dev 16-B aligned']
    assert rows['opa_dwconv_actp_f16(act=3)'] == [1, 'opa_dwconv_actp_f16: act must be 0 (none), 1 (ReLU), 2 (hardswish) or 4 (clipped ReLU)']
    assert rows['opa_dwconv_actp_f16(batch=8192)'] == [1, 'opa_dwconv_actp_f16: batch * output rows must not exceed 65535']


if __name__ == '__main__':
    at.child(table())
