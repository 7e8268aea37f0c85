"""Every status and message with which the trunk's C entry points (``csrc/capi_trunk.hip``: ``opa_bias_act`` ... ``opa_head_epilogue``
and ``opa_se_workspace_bytes``) answer a call they do not launch, against ``golden/capi_refusals.json``
(``golden/make_golden_abi.py capi_refusals``; written from the commit before the entry points moved into their own file), on the
harness of ``abi_tables.py``.

Per entry point one valid base call with fake pointers, and rows that each change one argument -- or two, where the point is the
ORDER of the checks (which message wins), a pointer the entry point does not test, or a bound's accepting side.  A row is of one of
four kinds, and the kind is part of what is asserted:

    refused   status != 0 and != OPA_ERR_HIP, with a message
    empty     OPA_OK: nothing to compute, returned before the launcher
    variant   a Winograd variant of diagnostic builds: past the checks, answered by the production launcher's dispatch with
              hipErrorInvalidValue before any call that touches a device (OPA_ERR_HIP, "...: invalid argument")
    size      ``opa_se_workspace_bytes``: the row records the size

NO row may reach a kernel launch: the pointers address nothing.  A pointer or alignment that an entry point does not test therefore
appears only together with an empty call or with a later check that refuses (``opa_channel_interleave`` and ``opa_head_epilogue``
have a single check and test no alignment: their pointers appear as null only).  The table runs in ONE fresh child process that
sees no GPU and says so (``opa_device_count() == 0``) before its first row: a check that a later change drops meets "no device"
there, not a fake pointer on a card.
"""
import json

import abi_tables as at

P, I31, Entry = at.P, at.I31, at.Entry
GOLDEN = at.golden('capi_refusals')
ENTRY_POINTS = 23
STATUSES = {1, at.OPA_ERR_WORKSPACE}              # of a refused row: OPA_ERR_INVALID_ARGUMENT; a workspace too small (squeeze-excite)


def table():
    """-> {row id: (kind, symbol, arguments)}"""
    t = {}
    terms = [-1, 0, 5, 7, 8, 10]

    e = Entry(t, 'opa_bias_act', x=P, bias=P, residual=P, rows=10, channels=64, dtype=0, relu=1)
    e.null('x bias'); e.off('x bias residual')
    e.empty(dict(rows=0), dict(rows=0, residual=None))
    e.each('rows', [-1]); e.each('channels', [-1, 0, 62, 63, 65]); e.each('dtype', [-1, 3])
    e.refused(dict(dtype=1, channels=4), dict(dtype=2, channels=4), dict(dtype=2, channels=12), dict(dtype=2, channels=63))
    e.refused(dict(rows=-1, channels=63), dict(channels=63, rows=0), dict(x=P + 4, rows=0))

    for symbol, pro in (('opa_gemm_bias_act_bf16', {}), ('opa_gemm_pro_bias_act_bf16', dict(a_bias=P))):
        e = Entry(t, symbol, a=P, **pro, w=P, bias=P, residual=P, out=P, m=128, n=64, k=64, relu=1)
        e.null('a w bias out ' + ' '.join(pro)); e.off('a w out residual ' + ' '.join(pro))
        e.empty(dict(m=0), dict(m=0, residual=None), dict(m=0, bias=P + 4), dict(m=0, bias=P + 8))       # (bias_dev's alignment: not tested)
        e.each('m', [-1, I31]); e.each('n k', [-1, 0, 32, 63, 65])
        e.refused(dict(a=None, k=63), dict(k=63, a=P + 4), dict(n=63, m=0), dict(a=P + 4, m=0), dict(m=I31, k=63))

    e = Entry(t, 'opa_gemm_bias_act_f32', a=P, a_bias=P, w=P, bias=P, residual=P, out=P, m=128, n=64, k=32, relu=1)
    e.null('a w bias out'); e.off('a a_bias w bias residual out')
    e.empty(dict(m=0), dict(m=0, a_bias=None), dict(m=0, residual=None))
    e.each('m', [-1, I31]); e.each('n', [-1, 0, 32, 63, 65]); e.each('k', [-1, 0, 16, 31, 33])
    e.refused(dict(a=None, k=31), dict(k=31, a=P + 4), dict(n=63, m=0), dict(bias=P + 4, m=0))

    e = Entry(t, 'opa_gemm_bias_act_f32x3', a=P, a_bias=P, w3=P, bias=P, residual=P, out=P, m=128, n=64, k=64, relu=1, terms=6)
    e.null('a w3 bias out'); e.off('a a_bias w3 bias residual out')
    e.empty(dict(m=0), dict(m=0, terms=9), dict(m=0, a_bias=None), dict(m=0, residual=None))
    e.each('m', [-1, I31]); e.each('n k', [-1, 0, 32, 63, 65]); e.each('terms', terms)
    e.refused(dict(terms=7, k=63), dict(k=63, a=P + 4), dict(n=63, m=0), dict(bias=P + 4, m=0))

    e = Entry(t, 'opa_gemm2_bias_act_f32x3', a1=P, k1=32, a2=P, k2=32, batch=1, h_in=8, w_in=8, stride=1, a_bias=P, w3cat=P, bias=P,
              out=P, n=64, relu=1, terms=6)
    crowd = dict(batch=2048, h_in=1024, w_in=1024)                                       # 2^31 pixels: one too many
    e.null('a1 a2 w3cat bias out'); e.off('a1 a2 a_bias w3cat bias out')
    e.each('batch h_in w_in k1 k2 n', [-1, 0]); e.each('stride', [-1, 0]); e.each('terms', terms)
    e.each('k1', [16, 31, 33, 64]); e.each('k2', [30, 31, 33, 64]); e.each('n', [32, 63, 65])
    e.refused(crowd, dict(crowd, stride=2), dict(crowd, a_bias=None), dict(crowd, a1=P + 4), dict(a1=None, k1=31), dict(k1=31, a1=P + 4))

    e = Entry(t, 'opa_conv_rows_f32x3', x=P, w3=P, bias=P, out=P, batch=1, hp=10, wp=10, pix=32, ho=8, wo=8, stride=1, ntaps=2,
              tap_floats=96, c_out=64, relu=1, terms=6)
    e.null('x w3 bias out'); e.off('x w3 bias out')
    e.each('batch hp wp pix ho wo tap_floats c_out', [-1, 0]); e.each('stride', [-1, 0]); e.each('ntaps', [-1, 0, 33]); e.each('terms', terms)
    e.each('tap_floats', [16, 95, 97]); e.each('ntaps', [1, 3]); e.each('c_out', [32, 63, 65]); e.each('pix', [3, 30, 33])
    # the taps of the last output pixel: rows 7 + 2 <= 10, floats 7 * 32 + 96 <= 10 * 32
    e.refused(dict(hp=8), dict(wp=9), dict(ho=10), dict(wo=9), dict(stride=2), dict(batch=167773), dict(batch=I31 - 1))
    e.refused(dict(x=None, pix=3), dict(pix=3, x=P + 4), dict(x=P + 4, hp=8))

    for symbol, dilated in (('opa_conv3x3_f32x3', {}), ('opa_conv3x3_dilated_f32x3', dict(dilation=2))):
        e = Entry(t, symbol, x=P, w3=P, bias=P, out=P, batch=2, h_in=9, w_in=7, c_in=64, c_out=128, stride=1, **dilated, relu=1, terms=6)
        e.null('x w3 bias out'); e.off('x w3 bias out')
        e.each('batch h_in w_in', [-1]); e.each('stride ' + ' '.join(dilated), [-1, 0]); e.each('c_in c_out', [-1, 0, 32, 63, 65, 96])
        e.each('terms', terms)
        (e.empty if dilated else e.refused)(dict(batch=0), dict(h_in=0), dict(w_in=0))
        e.refused(dict(batch=0, c_in=32), dict(batch=0, x=P + 4), dict(x=None, c_in=32), dict(c_in=32, x=P + 4))
        # (batch h w + d (w + 1)) c_in 4 < 2^31
        e.refused(dict(batch=1, h_in=559240, w_in=15), dict(batch=I31 - 1, h_in=I31 - 1, w_in=I31 - 1), dict(x=P + 4, batch=1, h_in=559240, w_in=15))
        if dilated:
            e.empty(dict(batch=0, w_in=15, dilation=2 ** 19 - 1))
            e.refused(dict(batch=0, w_in=15, dilation=2 ** 19), dict(batch=1, h_in=559207, w_in=15, dilation=32))

    e = Entry(t, 'opa_maxpool3x3_bias_act', x=P, bias=P, out=P, dtype=0, batch=2, h=9, w=7, c=64, stride=2, relu=1)
    e.null('x out'); e.off('x bias out')
    e.empty(dict(batch=0), dict(h=0), dict(w=0), dict(batch=0, bias=None), dict(batch=0, dtype=2))
    e.each('batch h w', [-1]); e.each('c', [-1, 0, 4, 12, 63, 65]); e.each('dtype', [-1, 1, 3]); e.each('stride', [-1, 0, 1, 3])
    e.refused(dict(batch=2 ** 10, h=2 ** 8, w=2 ** 8, c=8), dict(dtype=2, batch=2 ** 11, h=2 ** 8, w=2 ** 8, c=8), dict(h=I31 - 1, w=I31 - 1))
    e.refused(dict(batch=0, c=4), dict(batch=0, stride=1), dict(x=None, dtype=1), dict(dtype=1, stride=1), dict(stride=1, c=4),
              dict(c=4, x=P + 4), dict(x=P + 4, batch=2 ** 10, h=2 ** 8, w=2 ** 8, c=8))

    for symbol, third in (('opa_gemm_unit_bias_act_f32x3', {}), ('opa_gemm_unit_act_f32x3', dict(residual=None, residual_pitch=0))):
        e = Entry(t, symbol, a=P, a_pitch=64, w3=P, bias=P, partner=P, partner_pitch=64, **third, out=P, m=128, n=64, k=64,
                  **{'act' if third else 'relu': 1}, terms=6)
        e.null('a w3 bias out'); e.off('w3 bias out'); e.off('a partner', by=[4])
        e.empty(dict(m=0), dict(m=0, a=P + 8), dict(m=0, partner=P + 8), dict(m=0, partner=None), dict(m=0, partner=None, partner_pitch=63),
                dict(m=0, a_pitch=2 ** 21), dict(m=0, partner_pitch=I31 - 2), dict(m=0, terms=9))
        e.each('m', [-1, I31]); e.each('n k', [-1, 0, 63, 65, 66]); e.each('terms', terms)
        e.each('a_pitch', [-1, 62, 63, 65, 2 ** 21 + 2]); e.each('partner_pitch', [-1, 62, 63, 65, I31])
        e.refused(dict(terms=7, n=63), dict(n=63, a_pitch=63), dict(a_pitch=63, a=P + 4), dict(a=P + 4, m=0), dict(bias=P + 4, m=0))
        if third:
            e.each('act', [-1, 3]); e.empty(dict(m=0, act=0), dict(m=0, act=2))
            e.refused(dict(residual=P), dict(residual=P, m=0), dict(residual=P, n=63), dict(act=3, residual=P))
            r = Entry(t, symbol, '[residual]', **dict(e.base, partner=None, partner_pitch=0, residual=P, residual_pitch=64))
            r.off('residual', by=[4]); r.each('residual_pitch', [-1, 62, 63, 65, I31])
            r.empty(dict(m=0, act=2), dict(m=0, residual=P + 8), dict(m=0, residual_pitch=I31 - 2))

    for symbol, variant, others, diagnostic in (('opa_conv3x3_winograd_f32', 0, [-1, 4, 5, 10, 19, 20], range(11, 19)),
                                                ('opa_conv3x3_winograd_f32x3', 4, [-1, 0, 1, 3, 5, 20, 24], range(21, 24))):
        e = Entry(t, symbol, x=P, u=P, bias=P, out=P, batch=1, h=8, w=8, c_in=16, c_out=64, relu=1, variant=variant, order=0)
        large = dict(h=2 ** 13, w=2 ** 13)                                               # 2^30 elements: one too many
        e.null('x u out'); e.off('x u bias out')
        e.each('batch h w c_in c_out', [-1, 0]); e.each('c_in', [8, 15, 17]); e.each('c_out', [32, 63, 65]); e.each('variant', others)
        e.refused(large, dict(batch=I31 - 1, h=1, w=1), dict(bias=None, x=P + 4), dict(x=None, c_in=15), dict(c_in=15, **large),
                  dict(x=P + 4, **large))
        if symbol.endswith('_f32'):                                                      # variant 1's narrower tiles
            e.each('c_in', [4, 12], variant=1); e.each('c_out', [16, 48], variant=1)
        for v in diagnostic:
            e.row('variant', variant=v)
        e.refused(dict(variant=diagnostic[0], c_in=15), dict(variant=diagnostic[0], x=P + 4))

    for symbol, act in (('opa_dwconv_bias_act', 'relu'), ('opa_dwconv_act', 'act')):
        e = Entry(t, symbol, x=P, x_pixel_stride=64, w=P, bias=P, out=P, out_pixel_stride=64, batch=1, h=8, width=8, channels=64, k=3,
                  stride=1, dtype=0, **{act: 2})
        rows = dict(batch=8192)                                                          # 65536 output rows: one too many
        e.null('x w out'); e.off('x w bias out', **rows); e.null('bias', **rows)         # (no alignment is tested, the bias may be null)
        e.each('batch h width channels', [-1, 0]); e.each('x_pixel_stride out_pixel_stride', [63]); e.each('k', [1, 2, 4, 6])
        e.each('stride', [0, 3]); e.each('dtype', [-1, 1, 3])
        e.refused(rows, dict(batch=65536, h=1), dict(batch=32768, h=3, stride=2), dict(batch=13108, h=7, k=5), dict(x=None, **rows))
        if act == 'act':
            e.each('act', [-1, 3]); e.refused(dict(act=3, x=None))
            for code in (0, 1):
                e.refused(dict(act=code, x=None), dict(act=code, k=4), dict(act=code, **rows))
        else:
            e.refused(dict(relu=0, x=None), dict(relu=-1, **rows), dict(relu=3, **rows))

    e = Entry(t, 'opa_gconv3x3_bias_act_f32', x=P, x_pixel_stride=64, wt=P, bias=P, out=P, out_pixel_stride=64, batch=1, h=8, w=8,
              channels=64, group_width=4, stride=1, relu=1)
    e.null('x wt out'); e.off('x wt bias out')
    e.empty(dict(batch=0), dict(h=0), dict(w=0), dict(batch=0, bias=None), dict(batch=65536, h=0))
    e.each('group_width', [-4, 0, 2, 3, 5, 128]); e.each('channels', [-1, 0, 62, 66]); e.each('stride', [0, 3])
    e.each('x_pixel_stride out_pixel_stride', [60, 63, 66]); e.each('batch h w', [-1])
    e.refused(dict(group_width=64, channels=32), dict(batch=65536), dict(h=2 ** 30, w=2 ** 30))
    e.refused(dict(x=None, group_width=3), dict(group_width=3, channels=0), dict(channels=0, stride=3), dict(stride=3, x_pixel_stride=63),
              dict(x_pixel_stride=63, x=P + 4), dict(x=P + 4, batch=-1), dict(batch=-1, h=0), dict(batch=0, x=P + 4))

    se = dict(batch=1, pixels=1000, channels=64)                                         # (its workspace: 1 * 2 * 64 * 8 bytes)
    for symbol, base, tested, untested in (
            ('opa_se_pool', dict(x=P, x_pixel_stride=64, **se, workspace=P, workspace_bytes=1024), 'x workspace', ''),
            ('opa_se_gate', dict(workspace=P, workspace_bytes=1024, **se, squeeze=16, w1=P, b1=P, w2=P, b2=P, gate=P, mean=P), 'workspace',
             'w1 b1 w2 b2 gate mean'),
            ('opa_se_scale', dict(x=P, x_pixel_stride=64, **se, gate=P), 'x gate', '')):
        e = Entry(t, symbol, **base)
        e.null(' '.join(n for n in base if base[n] == P and n != 'mean')); e.off(tested)
        e.each('batch', [-1, 0, 65536]); e.each('pixels', [-1, 0, 65535 * 512 + 1]); e.each('channels', [-1, 0, 62, 63, 8193, 8196])
        if 'x_pixel_stride' in base:
            e.each('x_pixel_stride', [60, 62, 63, 66])
        e.refused(dict({tested.split()[0]: None}, batch=0), dict({tested.split()[0]: P + 4}, batch=0))
        if 'workspace_bytes' in base:
            e.each('workspace_bytes', [0, 1023]); e.off(untested, workspace_bytes=0)
            e.refused(dict(workspace=P + 4, workspace_bytes=0), dict(pixels=1025, workspace_bytes=1024))
        if 'squeeze' in base:
            e.each('squeeze', [-1, 0, 4097]); e.null('mean', workspace_bytes=0); e.refused(dict(squeeze=0, batch=0))

    e = Entry(t, 'opa_channel_interleave', a=P, a_pixel_stride=32, b=P, b_pixel_stride=32, out=P, rows=10, half=32, dtype=0)
    e.null('a b out'); e.each('rows half', [-1, 0]); e.each('a_pixel_stride b_pixel_stride', [31]); e.each('dtype', [-1, 3])

    e = Entry(t, 'opa_head_epilogue', conv=P, dtype=0, batch=1, hc=8, wc=8, n_fields=17, n_components=5, upsample=1, n_confidences=1,
              n_vectors=1, vector_offset_mask=1, n_scales=1, out=P)
    e.null('conv out'); e.each('dtype', [-1, 3]); e.each('batch hc wc n_fields n_components', [-1, 0]); e.each('upsample', [0, 3])
    e.each('n_confidences n_vectors n_scales', [-1]); e.each('n_components', [4]); e.each('n_confidences n_vectors n_scales', [2])

    e = Entry(t, 'opa_se_workspace_bytes', batch=2, pixels=1000, channels=64)
    for change in (dict(), dict(batch=0), dict(batch=-1), dict(pixels=0), dict(pixels=-1), dict(channels=0), dict(channels=-1),
                   dict(batch=1, pixels=512, channels=4), dict(batch=1, pixels=513, channels=4)):
        e.row('size', **change)
    return t


def canonical(symbol, message):
    """Before the twins were folded, ``opa_dwconv_act`` forwarded the activation codes 0 / 1 to ``opa_dwconv_bias_act`` and such a
    call was refused under the twin's name; it is now refused under its own.  The text behind the prefix and the status are the
    same: the old prefix is read as the new one, so that the golden file holds ONE spelling."""
    old = 'opa_dwconv_bias_act: '
    return 'opa_dwconv_act: ' + message[len(old):] if symbol == 'opa_dwconv_act' and message.startswith(old) else message


def refusals():
    """The table run and checked -> what the golden file holds"""
    return at.refusals(__file__, table(), STATUSES)


def test_refusals_match_the_golden_table():
    got = refusals()
    assert len({symbol for _, symbol, _ in table().values()}) == ENTRY_POINTS
    with open(GOLDEN) as f:
        at.assert_same(got['rows'], json.load(f)['rows'])


if __name__ == '__main__':
    at.child(table(), canonical)
