"""Every status and message with which ``opa_gemm_unit_actp_bf16`` (``csrc/capi_trunk.hip``: the unit mode of the bf16 GEMM,
``csrc/gemm_unit_bf16.hip``) answers a call it does not launch, against ``golden/capi_refusals_unit_bf16.json``
(``golden/make_golden_abi.py capi_refusals_unit_bf16``).

The table is built and run like ``test_capi_refusals_actp.py``'s, on the harness of ``abi_tables.py`` (``Entry``, the kinds, the child process):
one valid base call with fake pointers, rows that each change one argument (or two, where the point is the ORDER of the checks), in one
fresh child process that sees no GPU.  The checks are ``opa_gemm_unit_actp_f32x3``'s in its order and, where the rule is the same, with
its words; what differs: no ``terms``, and the activation operands need 4 bytes, not 8 -- an offset of 4, 8 or 12 is accepted (shown by
the empty call, which returns OPA_OK only behind every check), an offset of 2 refused."""
import json

import abi_tables as at

GOLDEN = at.golden('capi_refusals_unit_bf16')
P, I31 = at.P, at.I31
NAN, INF = float('nan'), float('inf')
SYMBOL = 'opa_gemm_unit_actp_bf16'
OPA_ERR_INVALID_ARGUMENT = 1
STATUSES = {OPA_ERR_INVALID_ARGUMENT}                # of a refused row


def table():
    """-> {row id: (kind, symbol, arguments)}"""
    t = {}
    base = dict(a=P, a_pitch=64, w=P, bias=P, partner=P, partner_pitch=64, residual=None, residual_pitch=0, out=P, m=128, n=64, k=64,
                act=3, act_param=0.01)
    e = at.Entry(t, SYMBOL, **base)
    e.null('a w bias out'); e.off('w bias out', by=[2, 4, 8]); e.off('a partner', by=[1, 2, 3, 6, 10, 14])
    # 4-byte offsets are accepted: the empty call is OPA_OK only behind every check
    e.empty(dict(m=0), dict(m=0, a=P + 4), dict(m=0, a=P + 8), dict(m=0, a=P + 12), dict(m=0, partner=P + 4), dict(m=0, partner=P + 12),
            dict(m=0, a=P + 4, partner=P + 12), dict(m=0, partner=None), dict(m=0, partner=None, partner_pitch=63), dict(m=0, a_pitch=2 ** 21),
            dict(m=0, partner_pitch=I31 - 2), dict(m=0, n=2, k=2, a_pitch=2, partner_pitch=2), dict(m=0, n=174, k=24, a_pitch=348, partner_pitch=174))
    e.each('m', [-1, I31, 2 ** 40]); e.each('n k', [-1, 0, 63, 65, 66])
    e.each('a_pitch', [-1, 62, 63, 65, 2 ** 21 + 2]); e.each('partner_pitch', [-1, 62, 63, 65, I31])
    e.each('act', [-1, 5, 6])
    # the parameter: finite for every code, a slope >= 0 for code 3, a cap > 0 for code 4; read by no other code
    e.each('act_param', [NAN, INF, -INF, -0.01])
    for code in (0, 1, 2, 3, 4):
        e.refused(dict(act=code, act_param=NAN), dict(act=code, act_param=INF))
    e.refused(dict(act=4, act_param=0.0), dict(act=4, act_param=-6.0), dict(act=4, act_param=-0.0))
    e.empty(dict(m=0, act=3, act_param=0.0), dict(m=0, act=3, act_param=0.3), dict(m=0, act=4, act_param=6.0), dict(m=0, act=4, act_param=1.5),
            dict(m=0, act=0, act_param=-1.0), dict(m=0, act=1, act_param=0.0), dict(m=0, act=2, act_param=0.0),
            dict(m=0, act=4, act_param=6.0, partner=None, partner_pitch=0))
    # which message wins: the range of the code, the parameter, partner + residual, residual + code, the sizes, the pitches, the alignment
    e.refused(dict(act=5, act_param=NAN), dict(act_param=NAN, residual=P, residual_pitch=64), dict(act_param=-0.01, n=63),
              dict(residual=P, residual_pitch=64), dict(residual=P, residual_pitch=64, m=0), dict(n=63, a_pitch=63),
              dict(a_pitch=63, a=P + 2), dict(a=P + 2, m=0), dict(bias=P + 4, m=0), dict(out=P + 8, m=0), dict(w=P + 8, m=0))
    r = at.Entry(t, SYMBOL, '[residual]', **dict(base, partner=None, partner_pitch=0, residual=P, residual_pitch=64, act=0, act_param=0.0))
    r.each('act', [3, 4], act_param=1.0)
    r.refused(dict(act=3, act_param=0.01, m=0), dict(act=4, act_param=6.0, m=0), dict(act=4, act_param=6.0, n=63), dict(act=4, act_param=0.0))
    r.off('residual', by=[1, 2, 3, 6]); r.each('residual_pitch', [-1, 62, 63, 65, I31])
    r.empty(dict(m=0), dict(m=0, act=1), dict(m=0, act=2), dict(m=0, residual=P + 4), dict(m=0, residual=P + 8), dict(m=0, residual_pitch=I31 - 2))
    return t


def refusals():
    """The table run and checked -> what the golden file holds"""
    return at.refusals(__file__, table(), STATUSES)


def test_refusals_match_the_golden_table():
    got = refusals()
    assert {symbol for _, symbol, _ in table().values()} == {SYMBOL}
    with open(GOLDEN) as f:
        at.assert_same(got['rows'], json.load(f)['rows'])


def test_the_refusals_use_the_float32_unit_modes_words():
    """Where the rule is the same the message is ``opa_gemm_unit_actp_f32x3``'s (``golden/capi_refusals_actp.json``) under the new name;
    the alignment message names 4 bytes."""
    with open(GOLDEN) as f:
        rows = json.load(f)['rows']
    with open(at.golden('capi_refusals_actp')) as f:
        f32 = json.load(f)['rows']
    other = 'opa_gemm_unit_actp_f32x3'
    same = ['(a=null)', '(m=-1)', '(n=63)', '(k=65)', '(a_pitch=62)', '(partner_pitch=%d)' % I31, '(act=5)', '(act_param=nan)', '(act_param=-0.01)',
            '(act=4, act_param=0.0)', '(residual=%d, residual_pitch=64)' % P, '[residual](act=3, act_param=1.0)', '[residual](act=4, act_param=1.0)',
            '(act=5, act_param=nan)', '(act_param=-0.01, n=63)', '(n=63, a_pitch=63)', '[residual](residual_pitch=63)']
    for row in same:
        status, message = f32[other + row]
        assert rows[SYMBOL + row] == [status, message.replace(other, SYMBOL)], row
    assert rows[SYMBOL + '(a=P+2)'] == [1, SYMBOL + ': a_dev / partner_dev / residual_dev must be 4-B, w_dev / bias_dev / out_dev 16-B aligned']
    assert rows[SYMBOL + '(a=P+2)'] == rows[SYMBOL + '(partner=P+6)'] == rows[SYMBOL + '[residual](residual=P+2)'] == rows[SYMBOL + '(bias=P+8)']
    assert 'pitch' in rows[SYMBOL + '(a_pitch=63, a=P+2)'][1] and 'aligned' in rows[SYMBOL + '(a=P+2, m=0)'][1]


if __name__ == '__main__':
    at.child(table())
