"""Every call that ``opa_stem7x7_act_bf16`` (``csrc/capi_trunk.hip``: the 7x7 RGB stem of a bfloat16 ResNet, ``csrc/stem7x7_bf16.hip``)
does not launch, on the harness of ``abi_tables.py`` (``Entry``, the kinds, the child process): one valid base call with fake pointers,
rows that each change one argument (or two, where the point is the ORDER of the checks), in one fresh child process that sees no GPU.

What is expected stands HERE, not in a file recorded from the code: a refused row answers status 1 (OPA_ERR_INVALID_ARGUMENT) with a
message under the entry point's name, an empty row OPA_OK; the eight checks -- null pointers; alignment (``x_dev`` on 2 bytes,
``w_dev``, ``bias_dev`` and ``out_dev`` on 16, a null bias passes); negative sizes; ``c_out``; the stride; the strides of ``x``;
``x``'s extent; ``out``'s size -- have pairwise distinct messages, every row of one check has that check's message, and where two
arguments are bad the EARLIER check's message wins; behind all of them an empty batch, height or width is OPA_OK."""
import abi_tables as at

P, I31 = at.P, at.I31
SYMBOL = 'opa_stem7x7_act_bf16'
OPA_ERR_INVALID_ARGUMENT = 1
STATUSES = {OPA_ERR_INVALID_ARGUMENT}                # of a refused row

# a channels-last [2, 3, 23, 19] image
BASE = dict(x=P, xb=23 * 19 * 3, xc=1, xr=19 * 3, xp=3, w=P, bias=P, out=P, batch=2, h=23, w_in=19, c_out=128, stride=1, relu=1)
# the checks in their order: (name, the rows that fail this check alone)
CHECKS = [
    ('null', [dict(x=None), dict(w=None), dict(out=None)]),
    ('alignment', [dict(x=P + 1), dict(x=P + 3), dict(w=P + 2), dict(w=P + 8), dict(bias=P + 4), dict(bias=P + 8), dict(out=P + 2), dict(out=P + 8)]),
    ('negative', [dict(batch=-1), dict(h=-1), dict(w_in=-1), dict(batch=-I31), dict(h=-I31), dict(w_in=-I31)]),
    ('c_out', [dict(c_out=v) for v in (-64, 0, 32, 63, 65, 96)]),
    ('stride', [dict(stride=v) for v in (-1, 0, 3, 4)]),
    ('x strides', [dict(**{k: v}) for k in ('xb', 'xc', 'xr', 'xp') for v in (0, -1, -2 ** 40)]),
    # the last element addressed 2^31 or more elements from the first: through each stride, and with every size at its largest
    ('x extent', [dict(xb=I31), dict(xc=2 ** 30), dict(xr=I31 // 22 + 1), dict(xr=I31),dict(xp=I31 // 18 + 1), dict(xb=2 ** 62, xc=2 ** 62, xr=2 ** 62, xp=2 ** 62),
                  dict(batch=I31 - 1, h=I31 - 1, w_in=I31 - 1)]),
    # out: 2^31 elements where x spans fewer (a broadcast image: every stride 1), at stride 1 and at stride 2
    ('out size', [dict(batch=2 ** 10, h=2 ** 8, w_in=2 ** 7, xb=1, xc=1, xr=1, xp=1, c_out=64),
                  dict(batch=2 ** 6, h=2 ** 9, w_in=2 ** 8, xb=1, xc=1, xr=1, xp=1, stride=2, c_out=1024)]),
]
# (the earlier check, the later one): both arguments bad, the earlier check's message is expected
ORDER = [
    ('null', dict(x=None), dict(w=P + 8)), ('alignment', dict(out=P + 8), dict(batch=-1)), ('negative', dict(batch=-1), dict(c_out=63)),
    ('c_out', dict(c_out=63), dict(stride=3)), ('stride', dict(stride=3), dict(xr=0)), ('x strides', dict(xp=-1), dict(xb=I31)),
    ('x extent', dict(xb=I31), dict(c_out=2 ** 30)),
    # ... and every check before the empty call's OPA_OK
    ('null', dict(x=None), dict(batch=0)), ('alignment', dict(bias=P + 4), dict(batch=0)), ('alignment', dict(x=P + 1), dict(h=0)),
    ('negative', dict(batch=-1), dict(h=0)), ('c_out', dict(c_out=0), dict(w_in=0)), ('stride', dict(stride=3), dict(batch=0)),
    ('x strides', dict(xc=0), dict(batch=0)), ('x extent', dict(xc=2 ** 30), dict(batch=0)), ('x extent', dict(xr=I31), dict(w_in=0)),
]
EMPTY = [dict(batch=0), dict(h=0), dict(w_in=0), dict(batch=0, h=0, w_in=0), dict(batch=0, bias=None), dict(batch=0, relu=0), dict(batch=0, stride=2),
         dict(h=0, stride=2), dict(batch=0, c_out=2048), dict(batch=0, h=2 ** 30, w_in=2 ** 30 - 2, xb=1, xc=1, xr=1, xp=1),
         # the stride of a dimension without elements addresses nothing
         dict(batch=0, xb=2 ** 62), dict(h=0, xr=2 ** 62), dict(w_in=0, xp=2 ** 62)]


def _row_id(change):
    return '%s(%s)' % (SYMBOL, ', '.join('%s=%s' % (k, 'null' if v is None else 'P+%d' % (v - P) if P < v < P + 16 else v) for k, v in change.items()))


def table():
    """-> {row id: (kind, symbol, arguments)}"""
    t = {}
    e = at.Entry(t, SYMBOL, **BASE)
    for _, rows in CHECKS:
        e.refused(*rows)
    e.refused(*[dict(first, **second) for _, first, second in ORDER])
    e.empty(*EMPTY)
    return t


def test_the_argument_order_is_the_headers():
    """``BASE`` lists the arguments as the C declaration does (the harness passes them in this order and appends the stream)."""
    import os
    with open(os.path.join(os.path.dirname(at.HERE), 'include', 'openpifpaf_amd.h')) as f:
        declaration = f.read().split('int ' + SYMBOL + '(')[1].split(');')[0]
    names = [a.split()[-1].lstrip('*') for a in declaration.split(',')]
    assert names == ['x_dev', 'x_batch_stride', 'x_channel_stride', 'x_row_stride', 'x_pixel_stride', 'w_dev', 'bias_dev', 'out_dev', 'batch', 'h', 'w',
                     'c_out', 'stride', 'relu', 'stream']
    assert list(BASE) == ['x', 'xb', 'xc', 'xr', 'xp', 'w', 'bias', 'out', 'batch', 'h', 'w_in', 'c_out', 'stride', 'relu']


def test_every_check_refuses_with_a_message_of_its_own_and_the_earlier_one_wins():
    got = at.refusals(__file__, table(), STATUSES)['rows']       # (check_kinds: refused rows status 1 under the symbol's name, empty rows 0)
    assert sorted(got) == sorted(table())
    messages = {}
    for name, rows in CHECKS:
        texts = {tuple(got[_row_id(change)]) for change in rows}
        assert len(texts) == 1, (name, texts)                                        # one message per check
        (status, text), = texts
        assert status == OPA_ERR_INVALID_ARGUMENT and text.startswith(SYMBOL + ': ') and len(text) > len(SYMBOL) + 2, (name, status, text)
        messages[name] = text
    assert len(set(messages.values())) == len(CHECKS), messages                     # pairwise distinct

    for name, first, second in ORDER:
        assert first in dict(CHECKS)[name]                                           # (the earlier change alone fails that check)
        status, text = got[_row_id(dict(first, **second))]
        assert status == OPA_ERR_INVALID_ARGUMENT and text == messages[name], (name, first, second, text)
    for change in EMPTY:
        assert got[_row_id(change)] == [0, ''], change


if __name__ == '__main__':
    at.child(table())
