"""Every status and message with which ``opa_gemm_unit_actp_f32x3`` and ``opa_dwconv_actp`` (``csrc/capi_trunk.hip``: the unit-mode GEMM
and the depthwise stencil with the activation codes that take a parameter, 3 LeakyReLU(slope) and 4 clipped ReLU(cap)) answer a call
they do not launch, against ``golden/capi_refusals_actp.json`` (``golden/make_golden_abi.py capi_refusals_actp``).

The table is built and run like ``test_capi_refusals.py``'s, on the harness of ``abi_tables.py`` (``Entry``, the kinds, the child
process): per entry point one valid base call with fake pointers, rows that each change one argument (or two, where the point is the ORDER of the checks), in one
fresh child process that sees no GPU.  What is new here: the parameter (NaN, +-Inf, a negative slope, a cap of zero or below), a
residual together with the codes 3 and 4, code 3 at the stencil -- and that the older entry points still refuse the new codes."""
import json

import abi_tables as at

GOLDEN = at.golden('capi_refusals_actp')
P, I31 = at.P, at.I31
NAN, INF = float('nan'), float('inf')
ENTRY_POINTS = 5
STATUSES = {1}                                    # of a refused row: OPA_ERR_INVALID_ARGUMENT


def table():
    """-> {row id: (kind, symbol, arguments)}"""
    t = {}
    terms = [-1, 0, 5, 7, 8, 10]

    base = dict(a=P, a_pitch=64, w3=P, bias=P, partner=P, partner_pitch=64, residual=None, residual_pitch=0, out=P, m=128, n=64, k=64,
                act=3, act_param=0.01, terms=6)
    e = at.Entry(t, 'opa_gemm_unit_actp_f32x3', **base)
    e.null('a w3 bias out'); e.off('w3 bias out'); e.off('a partner', by=[4])
    e.empty(dict(m=0), dict(m=0, a=P + 8), dict(m=0, partner=P + 8), dict(m=0, partner=None), dict(m=0, partner=None, partner_pitch=63),
            dict(m=0, a_pitch=2 ** 21), dict(m=0, partner_pitch=I31 - 2), dict(m=0, terms=9))
    e.each('m', [-1, I31]); e.each('n k', [-1, 0, 63, 65, 66]); e.each('terms', terms)
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
    # which message wins: the range of the code, the parameter, partner + residual, residual + code, the sizes
    e.refused(dict(act=5, act_param=NAN), dict(act_param=NAN, residual=P, residual_pitch=64), dict(act_param=-0.01, n=63),
              dict(residual=P, residual_pitch=64), dict(residual=P, residual_pitch=64, m=0), dict(terms=7, n=63), dict(n=63, a_pitch=63),
              dict(a_pitch=63, a=P + 4), dict(a=P + 4, m=0), dict(bias=P + 4, m=0))
    r = at.Entry(t, 'opa_gemm_unit_actp_f32x3', '[residual]', **dict(base, partner=None, partner_pitch=0, residual=P, residual_pitch=64, act=0,
                                                                      act_param=0.0))
    r.each('act', [3, 4], act_param=1.0)
    r.refused(dict(act=3, act_param=0.01, m=0), dict(act=4, act_param=6.0, m=0), dict(act=4, act_param=6.0, n=63), dict(act=4, act_param=0.0))
    r.off('residual', by=[4]); r.each('residual_pitch', [-1, 62, 63, 65, I31])
    r.empty(dict(m=0), dict(m=0, act=1), dict(m=0, act=2), dict(m=0, residual=P + 8), dict(m=0, residual_pitch=I31 - 2))

    e = at.Entry(t, 'opa_dwconv_actp', x=P, x_pixel_stride=64, w=P, bias=P, out=P, out_pixel_stride=64, batch=1, h=8, width=8, channels=64, k=3,
                  stride=1, dilation=1, dtype=0, act=4, act_param=6.0)
    rows = dict(batch=8192)                                                          # 65536 output rows: one too many
    e.null('x w out'); e.off('x w bias out', **rows); e.null('bias', **rows)         # (no alignment is tested, the bias may be null)
    e.each('batch h width channels', [-1, 0]); e.each('x_pixel_stride out_pixel_stride', [63]); e.each('k', [1, 2, 4, 6, 9])
    e.each('stride', [0, 3]); e.each('dtype', [-1, 1, 3]); e.each('dilation', [-1, 0, 3, 8])
    e.refused(dict(dilation=2, stride=2), dict(dilation=4, stride=2))
    e.refused(rows, dict(batch=65536, h=1), dict(batch=32768, h=3, stride=2), dict(batch=13108, h=7, k=5), dict(batch=9363, h=7, k=7),
              dict(x=None, **rows), dict(k=7, **rows), dict(dilation=2, **rows), dict(dtype=2, **rows))
    e.each('act', [-1, 3, 5]); e.refused(dict(act=3, act_param=0.01), dict(act=3, x=None))
    e.each('act_param', [NAN, INF, -INF, 0.0, -0.0, -6.0])
    for code in (0, 1, 2):
        e.refused(dict(act=code, act_param=NAN), dict(act=code, x=None), dict(act=code, k=4), dict(act=code, act_param=-1.0, **rows))
    e.refused(dict(act=3, act_param=NAN), dict(act_param=NAN, x=None), dict(act_param=0.0, x=None), dict(act_param=1.5, x=None))

    # the older entry points keep their ranges: the new codes are refused there, with the words they have always used
    e = at.Entry(t, 'opa_gemm_unit_act_f32x3', a=P, a_pitch=64, w3=P, bias=P, partner=P, partner_pitch=64, residual=None, residual_pitch=0, out=P,
                  m=128, n=64, k=64, act=1, terms=6)
    e.each('act', [3, 4, 5]); e.refused(dict(act=4, m=0), dict(act=4, partner=None, residual=P, residual_pitch=64))
    for symbol, dilated in (('opa_dwconv_act', {}), ('opa_dwconv_dilated_act', dict(dilation=1))):
        e = at.Entry(t, symbol, x=P, x_pixel_stride=64, w=P, bias=P, out=P, out_pixel_stride=64, batch=1, h=8, width=8, channels=64, k=3, stride=1,
                      **dilated, dtype=0, act=1)
        e.each('act', [3, 4, 5]); e.refused(dict(act=4, x=None))
    return t


def refusals():
    """The table run and checked -> what the golden file holds"""
    return at.refusals(__file__, table(), STATUSES)


def test_refusals_match_the_golden_table():
    got = refusals()
    assert len({symbol for _, symbol, _ in table().values()}) == ENTRY_POINTS
    with open(GOLDEN) as f:
        at.assert_same(got['rows'], json.load(f)['rows'])


def test_the_refusals_name_what_is_wrong():
    """The messages the issue asks for, read from the golden file: the parameter, the residual, the stencil's code 3."""
    with open(GOLDEN) as f:
        rows = json.load(f)['rows']
    assert rows['opa_gemm_unit_actp_f32x3(act_param=nan)'] == [1, 'opa_gemm_unit_actp_f32x3: act_param must be finite']
    assert 'negative' in rows['opa_gemm_unit_actp_f32x3(act_param=-0.01)'][1]
    assert 'positive' in rows['opa_gemm_unit_actp_f32x3(act=4, act_param=0.0)'][1] and 'positive' in rows['opa_dwconv_actp(act_param=0.0)'][1]
    for code in (3, 4):
        assert rows['opa_gemm_unit_actp_f32x3[residual](act=%d, act_param=1.0)' % code] == \
            [1, 'opa_gemm_unit_actp_f32x3: a residual cannot be combined with act 3 or 4']
    assert rows['opa_dwconv_actp(act=3)'] == [1, 'opa_dwconv_actp: act must be 0 (none), 1 (ReLU), 2 (hardswish) or 4 (clipped ReLU)']
    assert rows['opa_dwconv_act(act=4)'] == [1, 'opa_dwconv_act: act must be 0 (none), 1 (ReLU) or 2 (hardswish)']
    assert rows['opa_gemm_unit_act_f32x3(act=4)'] == [1, 'opa_gemm_unit_act_f32x3: bad arguments']


if __name__ == '__main__':
    at.child(table())
