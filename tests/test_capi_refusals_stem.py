"""Every status and message with which ``opa_stem3x3_actp`` (``csrc/capi_trunk.hip``: the 3x3 RGB stem of the non-ResNet backbones,
``csrc/stem.hip``) answers a call it does not launch, against ``golden/capi_refusals_stem.json``
(``golden/make_golden_abi.py capi_refusals_stem``).

The table is built and run like ``test_capi_refusals.py``'s, on the harness of ``abi_tables.py`` (``Entry``, the kinds, the child
process): one valid base call with fake pointers, rows that each change one argument (or two, where the point is the ORDER of the checks), in one fresh child
process that sees no GPU.  A refusing row has status 1 (``OPA_ERR_INVALID_ARGUMENT``) in the table itself; the JSON pins the messages."""
import json

import abi_tables as at

GOLDEN = at.golden('capi_refusals_stem')
P, I31 = at.P, at.I31
NAN, INF = float('nan'), float('inf')
SYMBOL = 'opa_stem3x3_actp'
OPA_ERR_INVALID_ARGUMENT = 1
STATUSES = {OPA_ERR_INVALID_ARGUMENT}                # of a refused row


def table():
    """-> {row id: (kind, symbol, arguments)}"""
    t = {}
    # a channels-last [2, 3, 9, 7] input: strides 189, 1, 21, 3
    e = at.Entry(t, SYMBOL, x=P, x_batch_stride=189, x_channel_stride=1, x_row_stride=21, x_pixel_stride=3, w=P, bias=P, out=P, batch=2, h=9,
                  width=7, channels_out=32, stride=2, act=4, act_param=6.0)
    e.null('x w out'); e.off('w bias out'); e.off('x', by=[1, 2, 3])
    e.each('batch', [-1]); e.each('h width', [-1, 0])
    e.each('x_batch_stride x_channel_stride x_row_stride x_pixel_stride', [-1, 0])
    e.each('stride', [-1, 0, 3]); e.each('channels_out', [-1, 0, 8, 23, 40, 48, 65]); e.each('act', [-1, 5])
    # the parameter: finite for every code, a slope >= 0 for code 3, a cap > 0 for code 4
    for code in (0, 1, 2, 3, 4):
        e.refused(dict(act=code, act_param=NAN), dict(act=code, act_param=INF), dict(act=code, act_param=-INF))
    e.refused(dict(act=3, act_param=-0.01), dict(act_param=0.0), dict(act_param=-0.0), dict(act_param=-6.0))
    # one past the limits: the last element of x -- (batch - 1) 189 + 2 * 1 + (h - 1) 21 + (width - 1) 3 in the base call -- at index
    # 2^31 through each of the four terms, 2^31 output elements, batch 65536
    e.refused(dict(x_batch_stride=I31 - 188), dict(x_channel_stride=(I31 - 374) // 2), dict(h=2, x_row_stride=I31 - 209),
              dict(width=2, x_pixel_stride=I31 - 359),
              dict(batch=65535, h=I31 - 1, width=I31 - 1), dict(batch=16384, h=128, width=64, stride=1, channels_out=16),
              dict(batch=65536, h=1, width=1), dict(batch=I31 - 1, h=1, width=1, channels_out=16))
    # an empty batch is OPA_OK, behind every check of a single argument and before the checks of the sizes' products
    e.empty(dict(batch=0), dict(batch=0, bias=None), dict(batch=0, x=P + 4), dict(batch=0, x_batch_stride=I31 * 4),
            dict(batch=0, h=I31 - 1, width=I31 - 1), dict(batch=0, act=0, act_param=-1.0), dict(batch=0, act=3, act_param=0.0),
            dict(batch=0, stride=1, channels_out=42, act=2, act_param=0.0))
    e.refused(dict(batch=0, x=None), dict(batch=0, out=P + 8), dict(batch=0, h=0), dict(batch=0, x_pixel_stride=0), dict(batch=0, stride=3),
              dict(batch=0, channels_out=40), dict(batch=0, act=5), dict(batch=0, act_param=NAN), dict(batch=0, act_param=0.0))
    # which message wins: null before alignment before the sizes before the strides before the stride before the channels before the
    # code before the parameter before the 32-bit limits before the grid
    e.refused(dict(x=None, w=P + 4), dict(w=P + 4, h=0), dict(h=0, x_row_stride=0), dict(x_row_stride=0, stride=3), dict(stride=3, channels_out=40),
              dict(channels_out=40, act=5), dict(act=5, act_param=NAN), dict(act_param=NAN, batch=65536),
              dict(batch=65536, x_batch_stride=I31), dict(batch=65536, h=1024, width=1024, stride=1))
    return t


def refusals():
    """The table run and checked -> what the golden file holds"""
    return at.refusals(__file__, table(), STATUSES)


def test_refusals_match_the_golden_table():
    got = refusals()
    assert {symbol for _, symbol, _ in table().values()} == {SYMBOL}
    with open(GOLDEN) as f:
        at.assert_same(got['rows'], json.load(f)['rows'])


def test_the_refusals_name_what_is_wrong():
    with open(GOLDEN) as f:
        rows = json.load(f)['rows']

    def message(**change):
        (row_id,) = [k for k in rows if k == '%s(%s)' % (SYMBOL, ', '.join('%s=%s' % kv for kv in change.items()))]
        assert rows[row_id][0] == OPA_ERR_INVALID_ARGUMENT
        return rows[row_id][1]
    assert 'NULL' in message(x='null') and 'aligned' in message(out='P+4') and 'aligned' in message(x='P+2')
    assert 'stride must be 1 or 2' in message(stride=3) and 'positive' in message(x_row_stride=0) and 'positive' in message(h=0)
    assert '16, 24, 32, 42 or 64' in message(channels_out=40)
    assert 'finite' in message(act=0, act_param='nan') and 'negative' in message(act=3, act_param=-0.01) and 'positive' in message(act_param=0.0)
    assert '2^31' in message(h=2, x_row_stride=I31 - 209) and 'x must' in message(x_batch_stride=I31 - 188) and '2^31' in message(batch=16384, h=128, width=64, stride=1, channels_out=16)
    assert '65535' in message(batch=65536, h=1, width=1)
    # the order of the checks
    assert 'NULL' in message(x='null', w='P+4') and 'stride must be 1 or 2' in message(stride=3, channels_out=40)
    assert 'finite' in message(act_param='nan', batch=65536) and '2^31' in message(batch=65536, x_batch_stride=I31)


if __name__ == '__main__':
    at.child(table())
