"""Every status and message with which ``opa_gconv3x3_act_bf16`` (``csrc/capi_trunk.hip``: the grouped 3x3 convolution of a bfloat16
ResNeXt, ``csrc/gconv3x3_bf16.hip``) answers a call it does not launch, against ``golden/capi_refusals_gconv3x3_bf16.json``
(``golden/make_golden_abi.py capi_refusals_gconv3x3_bf16``).

The table is built and run like ``test_capi_refusals_conv3x3_bf16.py``'s, on the harness of ``abi_tables.py`` (``Entry``, the kinds, the
child process): one valid base call with fake pointers, rows that each change one argument (or two, where the point is the ORDER of
the checks), in one fresh child process that sees no GPU.  One row per check, each with a message of its own: null pointers, the
alignment of all four (a null bias passes), negative sizes, the channel multiple, the group width, a group width equal to the
channels, the stride, the dilation, a stride with a dilation above 1, ``x`` and ``out`` below 2^31 elements; behind them an empty
batch, height or width is OPA_OK."""
import json

import abi_tables as at

GOLDEN = at.golden('capi_refusals_gconv3x3_bf16')
P, I31 = at.P, at.I31
SYMBOL = 'opa_gconv3x3_act_bf16'
OPA_ERR_INVALID_ARGUMENT = 1
STATUSES = {OPA_ERR_INVALID_ARGUMENT}                # of a refused row


def table():
    """-> {row id: (kind, symbol, arguments)}"""
    t = {}
    base = dict(x=P, w=P, bias=P, out=P, batch=2, h_in=23, w_in=19, channels=128, group_width=4, stride=1, dilation=1, relu=1)
    e = at.Entry(t, SYMBOL, **base)
    e.null('x w out')
    e.off('x w bias out', by=[2, 4, 8])
    e.each('batch h_in w_in', [-1, -I31])
    e.each('channels', [-64, 0, 32, 63, 65, 96])
    e.each('group_width', [-4, 0, 1, 2, 3, 12, 24, 48, 128, 256])
    e.refused(dict(channels=64, group_width=64))                                          # one group: the dense convolution's
    e.each('stride', [-1, 0, 3, 4])
    e.each('dilation', [-1, 0, 3, 5, 8])
    e.refused(dict(stride=2, dilation=2), dict(stride=2, dilation=4))
    # x: 2^31 elements, and far more; out: 2^31 elements where x would have them too is x's message, so out alone cannot be reached at
    # stride 1 (as many output as input channels) -- its row is the check's place in the order, at stride 2 behind x's
    e.refused(dict(batch=2 ** 9, h_in=2 ** 8, w_in=2 ** 7), dict(batch=I31 - 1, h_in=I31 - 1, w_in=I31 - 1, channels=I31 - 63),
              dict(batch=2 ** 9, h_in=2 ** 8, w_in=2 ** 7, stride=2))
    # the empty calls: OPA_OK only behind every check; a null bias passes every check too
    e.empty(dict(batch=0), dict(h_in=0), dict(w_in=0), dict(batch=0, h_in=0, w_in=0), dict(batch=0, bias=None), dict(batch=0, relu=0),
            dict(batch=0, stride=2), dict(h_in=0, stride=2), dict(batch=0, dilation=2), dict(batch=0, dilation=4),
            dict(batch=0, channels=2048, group_width=64), dict(batch=0, group_width=32), dict(batch=0, h_in=I31 - 1, w_in=I31 - 1))
    # which message wins: null, alignment, negative sizes, channels, group width, one group, stride, dilation, their combination, x
    # -- and all before empty
    e.refused(dict(x=None, w=P + 8), dict(out=P + 8, batch=-1), dict(batch=-1, channels=63), dict(channels=96, group_width=12),
              dict(group_width=12, stride=3), dict(channels=64, group_width=64, stride=3), dict(stride=3, dilation=3),
              dict(dilation=3, batch=2 ** 9, h_in=2 ** 8, w_in=2 ** 7), dict(stride=2, dilation=2, batch=2 ** 9, h_in=2 ** 8, w_in=2 ** 7),
              dict(x=None, batch=0), dict(bias=P + 4, batch=0), dict(batch=-1, h_in=0), dict(channels=63, batch=0),
              dict(group_width=12, w_in=0), dict(channels=64, group_width=64, batch=0), dict(stride=3, batch=0), dict(dilation=3, batch=0),
              dict(stride=2, dilation=2, batch=0))
    return t


def refusals():
    """The table run and checked -> what the golden file holds"""
    return at.refusals(__file__, table(), STATUSES)


def test_refusals_match_the_golden_table():
    got = refusals()
    assert {symbol for _, symbol, _ in table().values()} == {SYMBOL}
    with open(GOLDEN) as f:
        at.assert_same(got['rows'], json.load(f)['rows'])


def test_every_check_has_a_message_of_its_own():
    with open(GOLDEN) as f:
        rows = json.load(f)['rows']

    def message(change):
        status, text = rows[SYMBOL + '(' + change + ')']
        assert status == OPA_ERR_INVALID_ARGUMENT
        return text
    one_per_check = [message(c) for c in ('x=null', 'x=P+8', 'batch=-1', 'channels=96', 'group_width=12', 'channels=64, group_width=64',
                                          'stride=3', 'dilation=3', 'stride=2, dilation=2', 'batch=512, h_in=256, w_in=128')]
    assert len(set(one_per_check)) == len(one_per_check), one_per_check
    # the order of the checks: the earlier one's message
    assert message('x=null, w=P+8') == message('x=null') and message('out=P+8, batch=-1') == message('x=P+8')
    assert message('batch=-1, channels=63') == message('batch=-1') and message('channels=96, group_width=12') == message('channels=96')
    assert message('group_width=12, stride=3') == message('group_width=12')
    assert message('channels=64, group_width=64, stride=3') == message('channels=64, group_width=64')
    assert message('stride=3, dilation=3') == message('stride=3')
    assert message('dilation=3, batch=512, h_in=256, w_in=128') == message('dilation=3')
    assert message('stride=2, dilation=2, batch=512, h_in=256, w_in=128') == message('stride=2, dilation=2')
    assert message('batch=512, h_in=256, w_in=128, stride=2') == message('batch=512, h_in=256, w_in=128')
    assert message('bias=P+4, batch=0') == message('x=P+8')
    assert message('stride=2, dilation=2, batch=0') == message('stride=2, dilation=2')
    assert message('channels=64, group_width=64, batch=0') == message('channels=64, group_width=64')


if __name__ == '__main__':
    at.child(table())
