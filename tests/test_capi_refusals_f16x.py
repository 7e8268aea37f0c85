"""Every status and message with which the float16 twins ``opa_gconv3x3_act_f16`` and ``opa_stem7x7_act_f16`` (``csrc/capi_trunk.hip``:
the grouped 3x3 convolution and the 7x7 stem for a network cast with ``.half()``) answer a call they do not launch.

The rows are the twins' originals': every row of ``test_capi_refusals_gconv3x3_bf16.py``'s and of
``test_capi_refusals_stem7x7_bf16.py``'s table under the float16 symbol, built and run on the harness of ``abi_tables.py`` in one fresh
child process that sees no GPU.  Each pair shares one checked function, so every answer must be the original's under the twin's name.
No golden file of its own: the grouped twin is compared row by row with ``golden/capi_refusals_gconv3x3_bf16.json``; the stem's
original keeps no golden file (its expectations stand in its test), so its rows run in the same child under BOTH names and are
compared with each other, and the stem's own rules -- one message per check, the earlier check wins -- are asserted on the twin's."""
import json

import abi_tables as at
import test_capi_refusals_gconv3x3_bf16 as gconv_bf16
import test_capi_refusals_stem7x7_bf16 as stem_bf16

TWINS = {'opa_gconv3x3_act_bf16': 'opa_gconv3x3_act_f16', 'opa_stem7x7_act_bf16': 'opa_stem7x7_act_f16'}
OPA_ERR_INVALID_ARGUMENT = 1
STATUSES = {OPA_ERR_INVALID_ARGUMENT}                # of a refused row


def _twin_rows():
    """-> {the twin's row id: (the original's row id, kind, the twin's symbol, the arguments)}"""
    out = {}
    originals = dict(gconv_bf16.table())
    originals.update(stem_bf16.table())
    for row_id, (kind, symbol, args) in originals.items():
        assert row_id.startswith(symbol) and symbol in TWINS, row_id
        out[TWINS[symbol] + row_id[len(symbol):]] = (row_id, kind, TWINS[symbol], args)
    return out


def table():
    """-> {row id: (kind, symbol, arguments)}: the twins' rows, and the stem's original rows (the yardstick of the stem's twin)"""
    t = {row_id: (kind, symbol, args) for row_id, (_, kind, symbol, args) in _twin_rows().items()}
    t.update(stem_bf16.table())
    return t


_GOT = {}


def _rows():
    if not _GOT:
        _GOT.update(at.refusals(__file__, table(), STATUSES)['rows'])      # (check_kinds: refused rows status 1 under the symbol's name, empty rows 0)
    return _GOT


def test_the_table_has_the_originals_rows():
    rows = _twin_rows()
    grouped = [r for r in rows if r.startswith('opa_gconv3x3_act_f16(')]
    stem = [r for r in rows if r.startswith('opa_stem7x7_act_f16(')]
    assert len(grouped) == len(gconv_bf16.table()) and len(grouped) > 70
    assert len(stem) == len(stem_bf16.table()) and len(stem) > 70
    assert {kind for _, kind, _, _ in rows.values()} == {'refused', 'empty'}
    assert sorted(_rows()) == sorted(table())


def test_the_grouped_twin_answers_as_the_originals_golden_table():
    with open(gconv_bf16.GOLDEN) as f:
        golden = json.load(f)['rows']
    got = _rows()
    original, twin = 'opa_gconv3x3_act_bf16', 'opa_gconv3x3_act_f16'
    checked = 0
    for row_id, (original_id, _, symbol, _) in _twin_rows().items():
        if symbol != twin:
            continue
        status, message = golden[original_id]
        assert got[row_id] == [status, message.replace(original, twin)], row_id
        checked += 1
    assert checked == len(golden)
    assert got['opa_gconv3x3_act_f16(group_width=12)'] == [1, 'opa_gconv3x3_act_f16: group_width must be 4, 8, 16, 32 or 64']
    assert got['opa_gconv3x3_act_f16(batch=0)'] == [0, '']


def test_the_stem_twin_answers_as_the_original_in_the_same_process():
    got = _rows()
    original, twin = 'opa_stem7x7_act_bf16', 'opa_stem7x7_act_f16'
    checked = 0
    for row_id, (original_id, _, symbol, _) in _twin_rows().items():
        if symbol != twin:
            continue
        status, message = got[original_id]
        assert got[row_id] == [status, message.replace(original, twin)], row_id
        assert status == 0 or (message.startswith(original + ': ') and twin not in message)
        checked += 1
    assert checked == len(stem_bf16.table())
    assert got['opa_stem7x7_act_f16(x=P+1)'] == [1, 'opa_stem7x7_act_f16: x_dev must be 2-B, w_dev / bias_dev / out_dev 16-B aligned']


def test_every_check_of_the_stem_twin_has_a_message_of_its_own_and_the_earlier_one_wins():
    got = _rows()

    def answer(change):
        return got['opa_stem7x7_act_f16' + stem_bf16._row_id(change)[len(stem_bf16.SYMBOL):]]
    messages = {}
    for name, rows in stem_bf16.CHECKS:
        texts = {tuple(answer(change)) for change in rows}
        assert len(texts) == 1, (name, texts)
        (status, text), = texts
        assert status == OPA_ERR_INVALID_ARGUMENT and text.startswith('opa_stem7x7_act_f16: '), (name, status, text)
        messages[name] = text
    assert len(set(messages.values())) == len(stem_bf16.CHECKS), messages
    for name, first, second in stem_bf16.ORDER:
        assert answer(dict(first, **second)) == [OPA_ERR_INVALID_ARGUMENT, messages[name]], (name, first, second)
    for change in stem_bf16.EMPTY:
        assert answer(change) == [0, ''], change


def test_the_argument_orders_are_the_headers():
    """Each twin's declaration lists the arguments of its original's."""
    import os
    with open(os.path.join(os.path.dirname(at.HERE), 'include', 'openpifpaf_amd.h')) as f:
        header = f.read()

    def names(symbol):
        declaration = header.split('int ' + symbol + '(')[1].split(');')[0]
        return [' '.join(a.split()) for a in declaration.split(',')]
    for original, twin in TWINS.items():
        assert names(original) == names(twin) and len(names(twin)) > 10, twin


if __name__ == '__main__':
    at.child(table())
