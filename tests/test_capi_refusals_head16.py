"""Every status and message with which ``opa_head_conv_fields_bf16`` and ``opa_head_conv_fields_f16`` (``csrc/capi_trunk.hip``: a 16-bit
head's 1x1 convolution and the head epilogue as one kernel, ``csrc/head16.hip``) answer a call they do not launch, against
``golden/capi_refusals_head16.json`` (``golden/make_golden_abi.py capi_refusals_head16``).

The table is built and run like ``test_capi_refusals_gemm2_bf16.py``'s, on the harness of ``abi_tables.py`` (``Entry``, the kinds, the
child process): one valid base call with fake pointers, rows that each change one argument (or two, where the point is the ORDER of
the checks), in one fresh child process that sees no GPU.  The message of every check is WRITTEN HERE, in the header's order -- null
pointers (all four), alignment (16 bytes of ``x_dev`` / ``w_dev``, 4 of ``bias_dev`` / ``out_dev``), a negative batch, non-positive sizes,
``k % 64``, ``upsample``, the component counts, ``x``'s size, ``N``, ``out``'s size --; behind them an empty batch is OPA_OK.  Both entry
points share one check function: the float16 one answers every row as the bfloat16 one does, under its own name."""
import json
import os
import re

import abi_tables as at

GOLDEN = at.golden('capi_refusals_head16')
P, I31 = at.P, at.I31
SYMBOLS = ('opa_head_conv_fields_bf16', 'opa_head_conv_fields_f16')
OPA_ERR_INVALID_ARGUMENT = 1
STATUSES = {OPA_ERR_INVALID_ARGUMENT}                # of a refused row
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# one message per check, in the order of the checks
NULL = 'x_dev, w_dev, bias_dev and out_dev must not be NULL'
ALIGNED = 'x_dev / w_dev must be 16-B, bias_dev / out_dev 4-B aligned'
BATCH = 'negative batch'
SIZES = 'hc, wc, k, n_fields and n_components must be positive'
K64 = 'k must be a multiple of 64'
UPSAMPLE = 'upsample must be 1 or 2'
COUNTS = 'n_components must be 1 + n_confidences + 2 * n_vectors + n_scales, no count negative'
X_SIZE = 'x must hold fewer than 2^31 elements (32-bit offsets)'
N_SIZE = 'n_fields * n_components * upsample^2 must not exceed 2^31 - 64'
OUT_SIZE = 'out must hold fewer than 2^31 elements (32-bit offsets)'
IN_ORDER = (NULL, ALIGNED, BATCH, SIZES, K64, UPSAMPLE, COUNTS, X_SIZE, N_SIZE, OUT_SIZE)

# the COCO Cif head of a ResNet-50 on a 5 x 7 trunk output
BASE = dict(x_dev=P, w_dev=P, bias_dev=P, out_dev=P, batch=2, hc=5, wc=7, k=2048, n_fields=17, n_components=5, upsample=2, n_confidences=1,
            n_vectors=1, vector_offset_mask=1, n_scales=1)
X_BIG = dict(batch=2 ** 10, hc=2 ** 5, wc=2 ** 5)                          # 2^20 pixels of 2^11 channels
N_BIG = dict(hc=1, wc=1, batch=1, n_fields=2 ** 27, upsample=2, n_components=4, n_scales=0)      # N = 2^31 where out holds 2^29
OUT_BIG = dict(batch=2 ** 7, hc=2 ** 8, wc=2 ** 8, k=64)                   # x: 2^29 elements; out: 2^7 * 85 * 511 * 511 >= 2^31


def table():
    """-> ({row id: (kind, symbol, arguments)}, {row id of a refused row: the message expected, without the symbol's name})"""
    t, expected = {}, {}
    for symbol in SYMBOLS:
        e = at.Entry(t, symbol, **BASE)

        def refused(message, *changes):
            before = set(t)
            e.refused(*changes)
            for row_id in set(t) - before:
                expected[row_id] = message
        # one argument each
        refused(NULL, *[{name: None} for name in ('x_dev', 'w_dev', 'bias_dev', 'out_dev')])
        refused(ALIGNED, *[{name: P + by} for name in ('x_dev', 'w_dev') for by in (2, 4, 8)],
                *[{name: P + by} for name in ('bias_dev', 'out_dev') for by in (1, 2)])
        refused(BATCH, dict(batch=-1), dict(batch=-I31))
        refused(SIZES, *[{name: v} for name in ('hc', 'wc', 'k', 'n_fields', 'n_components') for v in (0, -1, -I31)])
        refused(K64, *[dict(k=v) for v in (32, 63, 65, 96, 1392)])
        refused(UPSAMPLE, *[dict(upsample=v) for v in (-1, 0, 3, 4)])
        refused(COUNTS, dict(n_components=4), dict(n_components=6), dict(n_confidences=2), dict(n_vectors=2), dict(n_scales=0),
                dict(n_confidences=-1, n_scales=3), dict(n_vectors=-1, n_scales=5), dict(n_scales=-1, n_confidences=3),
                dict(n_confidences=I31 - 1, n_vectors=I31 - 1, n_scales=I31 - 1))
        refused(X_SIZE, X_BIG, dict(batch=I31 - 1, hc=I31 - 1, wc=I31 - 1, k=I31 - 64))
        refused(N_SIZE, N_BIG)
        refused(OUT_SIZE, OUT_BIG)
        # the empty call: OPA_OK only behind every check; bias_dev and out_dev need 4 bytes alone; CifDet's counts, no upsampling
        e.empty(dict(batch=0), dict(batch=0, bias_dev=P + 4, out_dev=P + 8), dict(batch=0, upsample=1), dict(batch=0, k=64),
                dict(batch=0, n_fields=80, n_components=6, n_vectors=2, n_scales=0, vector_offset_mask=1), dict(batch=0, hc=I31 - 1, wc=I31 - 1),
                dict(batch=0, vector_offset_mask=2 ** 32 - 1))
        # which message wins where two arguments are bad: the earlier check's -- and every check before the empty call
        refused(NULL, dict(x_dev=None, w_dev=P + 8), dict(out_dev=None, batch=0))
        refused(ALIGNED, dict(out_dev=P + 2, batch=-1), dict(w_dev=P + 8, batch=0))
        refused(BATCH, dict(batch=-1, hc=0))
        refused(SIZES, dict(k=0, upsample=3), dict(wc=0, batch=0))
        refused(K64, dict(k=32, upsample=3), dict(k=32, batch=0))
        refused(UPSAMPLE, dict(upsample=3, n_components=4), dict(upsample=0, batch=0))
        refused(COUNTS, dict(n_components=4, **X_BIG), dict(n_scales=2, batch=0))
        refused(X_SIZE, dict(X_BIG, n_fields=2 ** 27, n_components=4, n_scales=0))               # (N and out too large as well)
        refused(N_SIZE, dict(N_BIG, batch=2 ** 4))                                              # (out too large as well)
    return t, expected


def refusals():
    """The table run and checked -> what the golden file holds"""
    return at.refusals(__file__, table()[0], STATUSES)


def test_refusals_match_the_golden_table():
    got = refusals()
    with open(GOLDEN) as f:
        at.assert_same(got['rows'], json.load(f)['rows'])


def test_every_row_is_answered_as_written_here_and_the_float16_rows_as_the_bfloat16_rows():
    t, expected = table()
    with open(GOLDEN) as f:
        rows = json.load(f)['rows']
    assert sorted(rows) == sorted(t) and {symbol for _, symbol, _ in t.values()} == set(SYMBOLS)
    for row_id, (kind, symbol, _) in t.items():
        if kind == 'refused':
            assert rows[row_id] == [OPA_ERR_INVALID_ARGUMENT, symbol + ': ' + expected[row_id]], (row_id, rows[row_id], expected[row_id])
        else:
            assert kind == 'empty' and rows[row_id] == [0, ''], (row_id, rows[row_id])
    assert sum(kind == 'empty' for kind, _, _ in t.values()) == 2 * 7
    assert set(expected.values()) == set(IN_ORDER) and len(set(IN_ORDER)) == len(IN_ORDER) == 10      # every check has rows and a message of its own
    bf16, f16 = SYMBOLS
    for row_id in [r for r in rows if r.startswith(bf16 + '(')]:
        status, message = rows[row_id]
        twin = rows[f16 + row_id[len(bf16):]]
        assert twin == [status, f16 + message[len(bf16):] if message else ''], (row_id, twin)


def test_the_argument_lists_are_the_headers_and_each_others():
    from openpifpaf_amd import _lib
    with open(os.path.join(ROOT, 'include', 'openpifpaf_amd.h')) as f:
        header = f.read()
    declarations = [re.sub(r'\s+', ' ', header.split('int ' + s + '(')[1].split(');')[0]) for s in SYMBOLS]
    assert declarations[0] == declarations[1]
    names = [re.sub(r'.*[\s*]', '', a.strip()) for a in declarations[0].split(',')]
    assert names == list(BASE) + ['stream'], names
    assert _lib.SYMBOLS[SYMBOLS[0]] == _lib.SYMBOLS[SYMBOLS[1]] and len(_lib.SYMBOLS[SYMBOLS[0]][1]) == len(BASE) + 1
    assert re.search(r'#define OPA_ABI_VERSION 9\b', header)                                   # (as the float16 twins: no struct changed)


if __name__ == '__main__':
    at.child(table()[0])
