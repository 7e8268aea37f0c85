"""Every status and message with which ``opa_gemm2_bias_act_bf16`` (``csrc/capi_trunk.hip``: a bfloat16 block's last 1x1 convolution and
its downsampling 1x1 convolution as one product, ``csrc/gemm2_bf16.hip``) answers a call it does not launch.

The table is built and run like ``test_capi_refusals_conv3x3_bf16.py``'s, on the harness of ``abi_tables.py`` (``Entry``, the kinds, the
child process): one valid base call with fake pointers, rows that each change one argument (or two, where the point is the ORDER of
the checks), in one fresh child process that sees no GPU.  What every row is answered with is WRITTEN HERE, beside the row
(``table()`` returns it), not recorded from the library: the checks in the header's order -- null pointers (``a2_dev``, ``wcat_dev``,
``out_dev``; ``a1_dev`` null exactly when ``k1 == 0``; ``a_bias_dev`` only with ``k1 > 0``), the alignment of all six (a null one
passes), negative sizes, ``k1``, ``k2``, ``n``, the stride, the three tensors below 2^31 elements -- each with a message of its own;
behind them an empty batch, height or width is OPA_OK."""
import os
import re

import abi_tables as at

P, I31 = at.P, at.I31
SYMBOL = 'opa_gemm2_bias_act_bf16'
OPA_ERR_INVALID_ARGUMENT = 1
STATUSES = {OPA_ERR_INVALID_ARGUMENT}                # of a refused row
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# one message per check, in the order of the checks
NULL = 'a2_dev, wcat_dev and out_dev must not be NULL'
A1_NULL = 'a1_dev must be NULL with k1 == 0 and with no other k1'
A_BIAS = 'a_bias_dev needs k1 > 0'
ALIGNED = 'pointers must be 16-B aligned'
NEGATIVE = 'negative batch, h_in or w_in'
K1 = 'k1 must be 0 or a positive multiple of 64'
K2 = 'k2 must be a positive multiple of 64'
N = 'n must be a positive multiple of 64'
STRIDE = 'stride must be 1 or 2'
A2_SIZE = 'a2 must hold fewer than 2^31 elements (32-bit offsets)'
A1_SIZE = 'a1 must hold fewer than 2^31 elements (32-bit offsets)'
OUT_SIZE = 'out must hold fewer than 2^31 elements (32-bit offsets)'
IN_ORDER = (NULL, A1_NULL, A_BIAS, ALIGNED, NEGATIVE, K1, K2, N, STRIDE, A2_SIZE, A1_SIZE, OUT_SIZE)

BASE = dict(a1_dev=P, k1=64, a2_dev=P, k2=128, batch=2, h_in=23, w_in=19, stride=1, a_bias_dev=P, wcat_dev=P, bias_dev=P, out_dev=P,
            n=128, relu=1)
# sizes: a2 of 2^31 elements; a1 of 2^31 where a2 has 2^29; out of 2^31 where a2 and a1 have 2^29, at stride 1 and at stride 2
A2_BIG = dict(batch=2 ** 10, h_in=2 ** 8, w_in=2 ** 6)
A1_BIG = dict(batch=2 ** 10, h_in=2 ** 8, w_in=2 ** 5, k1=256, k2=64)
OUT_BIG = dict(batch=2 ** 10, h_in=2 ** 8, w_in=2 ** 5, k1=64, k2=64, n=256)
OUT_BIG_S2 = dict(batch=2 ** 6, h_in=2 ** 9, w_in=2 ** 8, stride=2, k1=64, k2=64, n=1024)


def table():
    """-> ({row id: (kind, symbol, arguments)}, {row id of a refused row: the message expected, without the symbol's name})"""
    t, expected = {}, {}
    e = at.Entry(t, SYMBOL, **BASE)

    def refused(message, *changes):
        before = set(t)
        e.refused(*changes)
        for row_id in set(t) - before:
            expected[row_id] = message
    # one argument each
    refused(NULL, dict(a2_dev=None), dict(wcat_dev=None), dict(out_dev=None))
    refused(A1_NULL, dict(a1_dev=None), dict(k1=0), dict(a1_dev=None, k1=64, a_bias_dev=None), dict(k1=0, a_bias_dev=None))
    refused(A_BIAS, dict(a1_dev=None, k1=0), dict(k1=-64))
    refused(ALIGNED, *[{name: P + by} for name in ('a1_dev', 'a2_dev', 'a_bias_dev', 'wcat_dev', 'bias_dev', 'out_dev') for by in (2, 4, 8)])
    refused(NEGATIVE, *[{name: v} for name in ('batch', 'h_in', 'w_in') for v in (-1, -I31)])
    refused(K1, dict(k1=-64, a_bias_dev=None), *[dict(k1=v) for v in (32, 63, 65, 96)])
    refused(K2, *[dict(k2=v) for v in (-64, 0, 32, 63, 65, 96)])
    refused(N, *[dict(n=v) for v in (-64, 0, 32, 63, 65, 96)])
    refused(STRIDE, *[dict(stride=v) for v in (-1, 0, 3, 4)])
    refused(A2_SIZE, A2_BIG, dict(batch=I31 - 1, h_in=I31 - 1, w_in=I31 - 1, k2=I31 - 64))
    refused(A1_SIZE, A1_BIG)
    refused(OUT_SIZE, OUT_BIG, OUT_BIG_S2)
    # the empty calls: OPA_OK only behind every check; a null bias, a null a_bias and the k1 == 0 form pass every check too
    e.empty(dict(batch=0), dict(h_in=0), dict(w_in=0), dict(batch=0, h_in=0, w_in=0), dict(batch=0, bias_dev=None), dict(batch=0, a_bias_dev=None),
            dict(batch=0, a1_dev=None, k1=0, a_bias_dev=None), dict(h_in=0, a1_dev=None, k1=0, a_bias_dev=None, bias_dev=None, relu=0),
            dict(batch=0, relu=0), dict(batch=0, stride=2), dict(h_in=0, stride=2), dict(batch=0, k1=2048, k2=1024, n=512),
            dict(batch=0, h_in=I31 - 1, w_in=I31 - 1))
    # which message wins where two arguments are bad: the earlier check's -- and every check before the empty call
    refused(NULL, dict(a2_dev=None, a1_dev=None), dict(out_dev=None, k1=0), dict(a2_dev=None, batch=0))
    refused(A1_NULL, dict(a1_dev=None, wcat_dev=P + 8), dict(k1=0, batch=0))
    refused(A_BIAS, dict(a1_dev=None, k1=0, out_dev=P + 8), dict(a1_dev=None, k1=0, w_in=0))
    refused(ALIGNED, dict(out_dev=P + 8, batch=-1), dict(bias_dev=P + 4, batch=0), dict(a_bias_dev=P + 2, h_in=0))
    refused(NEGATIVE, dict(batch=-1, k1=32), dict(batch=-1, h_in=0))
    refused(K1, dict(k1=32, k2=32), dict(k1=32, batch=0))
    refused(K2, dict(k2=32, n=32), dict(k2=0, w_in=0))
    refused(N, dict(n=32, stride=3), dict(n=0, batch=0))
    refused(STRIDE, dict(stride=3, **A2_BIG), dict(stride=3, batch=0))
    refused(A2_SIZE, dict(A2_BIG, k1=256, n=1024))                                        # (a1 and out too large as well)
    refused(A1_SIZE, dict(A1_BIG, n=256))                                                  # (out too large as well)
    return t, expected


def test_every_row_is_answered_as_written_here():
    t, expected = table()
    got = at.refusals(__file__, t, STATUSES)['rows']
    assert {symbol for _, symbol, _ in t.values()} == {SYMBOL} and sorted(got) == sorted(t)
    for row_id, (kind, _, _) in t.items():
        if kind == 'refused':
            assert got[row_id] == [OPA_ERR_INVALID_ARGUMENT, SYMBOL + ': ' + expected[row_id]], (row_id, got[row_id], expected[row_id])
        else:
            assert kind == 'empty' and got[row_id] == [0, ''], (row_id, got[row_id])
    assert sum(kind == 'empty' for kind, _, _ in t.values()) == 13
    assert set(expected.values()) == set(IN_ORDER)                                         # every check has rows of its own


def test_every_check_has_a_message_of_its_own():
    assert len(set(IN_ORDER)) == len(IN_ORDER) == 12


def test_the_argument_names_are_the_headers():
    with open(os.path.join(ROOT, 'include', 'openpifpaf_amd.h')) as f:
        declaration = f.read().split('int ' + SYMBOL + '(')[1].split(');')[0]
    names = [re.sub(r'.*[\s*]', '', a.strip()) for a in declaration.split(',')]
    assert names == list(BASE) + ['stream'], names


if __name__ == '__main__':
    at.child(table()[0])
