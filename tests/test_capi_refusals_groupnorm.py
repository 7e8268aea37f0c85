"""Every status and message with which ``opa_groupnorm_actp`` (``csrc/capi_trunk.hip``: group norm + activation of a ShuffleNetV2K built
with ``--shufflenetv2k-group-norm``, ``csrc/groupnorm.hip``) answers a call it does not launch, against
``golden/capi_refusals_groupnorm.json`` (``golden/make_golden_abi.py capi_refusals_groupnorm``).

The table is built and run like ``test_capi_refusals_stem.py``'s: one valid base call with fake pointers, rows that each change one
argument (or two, where the point is the ORDER of the checks), in one fresh child process that sees no GPU.  A refusing row has status
1 (``OPA_ERR_INVALID_ARGUMENT``), a ``workspace`` row 4 (``OPA_ERR_WORKSPACE``) in the table itself; the JSON pins the messages.

The documented order (``include/openpifpaf_amd.h``): NULL, alignment, sizes, ``channels % groups``, an odd ``channels / groups``, the
strides, ``eps``, ``act``, ``act_param``, in place with unequal strides -- the empty batch's ``OPA_OK`` -- the grid and index limits,
the workspace."""
import json

import abi_tables as at

GOLDEN = at.golden('capi_refusals_groupnorm')
P, I31 = at.P, at.I31
NAN, INF = float('nan'), float('inf')
SYMBOL = 'opa_groupnorm_actp'
OPA_ERR_INVALID_ARGUMENT, OPA_ERR_WORKSPACE = 1, 4
STATUSES = {OPA_ERR_INVALID_ARGUMENT}                # of a refused row; a ``workspace`` row: OPA_ERR_WORKSPACE (``at.check_kinds``)
CHUNK = 512


def need(batch, pixels, channels):
    """``opa_groupnorm_workspace_bytes``, written out: (sum, sum of squares) in float64 per (image, chunk, channel), (a, s) in float32
    per (image, channel)."""
    return batch * ((pixels + CHUNK - 1) // CHUNK) * channels * 16 + batch * channels * 8


def table():
    """-> {row id: (kind, symbol, arguments)}"""
    t = {}
    # [2, 63, 24] in 4 groups, out of place, LeakyReLU
    e = at.Entry(t, SYMBOL, x=P, x_pixel_stride=24, gamma=P, beta=P, out=2 * P, out_pixel_stride=24, batch=2, pixels=63, channels=24,
                  groups=4, eps=1e-5, act=3, act_param=0.01, workspace=3 * P, workspace_bytes=need(2, 63, 24))
    e.null('x out'); e.off('x out', by=[4, 12]); e.off('gamma beta', by=[1, 2, 3]); e.off('workspace', by=[4, 8])
    e.each('batch', [-1]); e.each('pixels channels groups', [-1, 0])
    e.each('groups', [5, 7, 9, 16, 48])                                  # channels % groups
    e.each('groups', [8, 24]); e.refused(dict(channels=174, groups=58, x_pixel_stride=174, out_pixel_stride=174))      # odd channels / groups
    e.each('x_pixel_stride out_pixel_stride', [-24, 0, 22, 23, 25])
    e.each('eps', [NAN, INF, -INF, -1e-5])
    e.each('act', [-1, 5])
    # the parameter: finite for every code, a slope >= 0 for code 3, a cap > 0 for code 4
    for code in (0, 1, 2, 3, 4):
        e.refused(dict(act=code, act_param=NAN), dict(act=code, act_param=INF), dict(act=code, act_param=-INF))
    e.refused(dict(act_param=-0.01), dict(act=4, act_param=0.0), dict(act=4, act_param=-0.0), dict(act=4, act_param=-6.0))
    # in place needs the same pitch
    e.refused(dict(out=P, out_pixel_stride=48), dict(out=P, x_pixel_stride=26))
    # one past the limits: grid.y / .z, the coefficients kernel's LDS, 32-bit vector indices within an image
    big = need(1, 1, 8)
    e.refused(dict(batch=65536, pixels=1, channels=8, groups=4), dict(batch=I31 - 1, pixels=1, channels=8, groups=4),
              dict(batch=1, pixels=65535 * CHUNK + 1, channels=8, groups=4, workspace_bytes=big), dict(batch=1, pixels=2 ** 62, channels=8, groups=4),
              dict(batch=1, pixels=1, channels=4200, groups=1, x_pixel_stride=4200, out_pixel_stride=4200),
              dict(batch=1, pixels=1, channels=I31 - 2, groups=1, x_pixel_stride=I31, out_pixel_stride=I31),
              dict(batch=1, pixels=2 ** 20, channels=4096, groups=2, x_pixel_stride=4096, out_pixel_stride=4096),
              dict(batch=1, pixels=65535 * CHUNK, channels=256, groups=32, x_pixel_stride=256, out_pixel_stride=256))
    # the workspace: NULL, one byte short, none
    for change in (dict(workspace=None), dict(workspace_bytes=need(2, 63, 24) - 1), dict(workspace_bytes=0),
                   dict(pixels=513, workspace_bytes=need(2, 512, 24)), dict(batch=3), dict(channels=48, groups=4, x_pixel_stride=48, out_pixel_stride=48),
                   dict(workspace=None, workspace_bytes=0)):
        e.row('workspace', **change)
    # an empty batch is OPA_OK, behind every check of a single argument and before the limits and the workspace
    e.empty(dict(batch=0), dict(batch=0, gamma=None, beta=None), dict(batch=0, workspace=None, workspace_bytes=0), dict(batch=0, out=P),
            dict(batch=0, pixels=2 ** 62), dict(batch=0, channels=8192, groups=2, x_pixel_stride=8192, out_pixel_stride=8192),
            dict(batch=0, act=0, act_param=-1.0), dict(batch=0, eps=0.0))
    e.refused(dict(batch=0, x=None), dict(batch=0, out=2 * P + 4), dict(batch=0, pixels=0), dict(batch=0, groups=5), dict(batch=0, groups=8),
              dict(batch=0, x_pixel_stride=22), dict(batch=0, eps=NAN), dict(batch=0, act=5), dict(batch=0, act_param=NAN),
              dict(batch=0, out=P, out_pixel_stride=48))
    # which message wins: each check before the next one of the documented order
    e.refused(dict(x=None, out=2 * P + 4), dict(out=2 * P + 4, pixels=0), dict(pixels=0, groups=5), dict(groups=5, x_pixel_stride=23),
              dict(groups=8, x_pixel_stride=23), dict(x_pixel_stride=23, eps=NAN), dict(eps=NAN, act=5), dict(act=5, act_param=NAN),
              dict(act_param=NAN, out=P, out_pixel_stride=48), dict(out=P, out_pixel_stride=48, batch=65536),
              dict(batch=65536, workspace_bytes=0), dict(batch=65536, pixels=2 ** 62),
              dict(pixels=2 ** 62, channels=4200, groups=1, x_pixel_stride=4200, out_pixel_stride=4200),
              dict(batch=1, pixels=2 ** 20, channels=8192, groups=2, x_pixel_stride=8192, out_pixel_stride=8192),
              dict(batch=1, pixels=2 ** 20, channels=4096, groups=2, x_pixel_stride=4096, out_pixel_stride=4096, workspace=None))
    # accepted up to the workspace check (so everything before it passed): no affine terms, in place, a slice, a zero eps
    for change in (dict(gamma=None, beta=None), dict(gamma=None), dict(out=P), dict(x_pixel_stride=48, out_pixel_stride=26), dict(eps=0.0),
                   dict(act=3, act_param=0.0), dict(batch=65535, pixels=1, channels=8, groups=4),
                   dict(batch=1, pixels=1, channels=4096, groups=2, x_pixel_stride=4096, out_pixel_stride=4096)):
        e.row('workspace', **dict(change, workspace_bytes=15))
    return t


# opa_groupnorm_workspace_bytes: (batch, pixels, channels)
SIZES = [(2, 63, 24), (1, 512, 8), (1, 513, 8), (32, 321 * 321, 24), (3, 1, 2048), (0, 5, 8), (-1, 5, 8), (1, 0, 8), (1, -1, 8), (1, 5, 0), (1, 5, -2)]


def refusals():
    """The table run and checked, and the sizes ``need``'s -> what the golden file holds"""
    got = at.refusals(__file__, table(), STATUSES)
    for a in SIZES:
        assert got['sizes']['%d,%d,%d' % a] == (need(*a) if min(a) > 0 else 0), a
    return got


def test_refusals_match_the_golden_table():
    got = refusals()
    assert {symbol for _, symbol, _ in table().values()} == {SYMBOL}
    with open(GOLDEN) as f:
        want = json.load(f)
    assert got['sizes'] == want['sizes']
    at.assert_same(got['rows'], want['rows'])


def test_the_refusals_name_what_is_wrong():
    with open(GOLDEN) as f:
        rows = json.load(f)['rows']

    def message(status=OPA_ERR_INVALID_ARGUMENT, **change):
        (row_id,) = [k for k in rows if k == '%s(%s)' % (SYMBOL, ', '.join('%s=%s' % kv for kv in change.items()))]
        assert rows[row_id][0] == status
        return rows[row_id][1]
    assert 'NULL' in message(x='null') and 'aligned' in message(out='P+4') and 'aligned' in message(gamma='P+2') and 'aligned' in message(workspace='P+8')
    assert 'positive' in message(pixels=0) and 'negative' in message(batch=-1)
    assert 'multiple of groups' in message(groups=5) and 'even' in message(groups=8) and 'channels / groups' in message(groups=24)
    assert 'strides' in message(x_pixel_stride=23) and 'strides' in message(out_pixel_stride=22)
    assert 'eps' in message(eps='nan') and 'eps' in message(eps=-1e-05)
    assert 'act must be' in message(act=5)
    assert 'finite' in message(act=0, act_param='nan') and 'negative' in message(act_param=-0.01) and 'positive' in message(act=4, act_param=0.0)
    assert 'in place' in message(out=P, out_pixel_stride=48)
    assert '65535' in message(batch=65536, pixels=1, channels=8, groups=4) and '2048' in message(batch=1, pixels=1, channels=4200, groups=1, x_pixel_stride=4200, out_pixel_stride=4200)
    assert '2^31' in message(batch=1, pixels=2 ** 20, channels=4096, groups=2, x_pixel_stride=4096, out_pixel_stride=4096)
    assert 'too small' in message(OPA_ERR_WORKSPACE, workspace_bytes=need(2, 63, 24) - 1) and 'NULL' in message(OPA_ERR_WORKSPACE, workspace='null')
    # the order of the checks
    assert 'NULL' in message(x='null', out=2 * P + 4) and 'aligned' in message(out=2 * P + 4, pixels=0) and 'positive' in message(pixels=0, groups=5)
    assert 'multiple' in message(groups=5, x_pixel_stride=23) and 'channels / groups' in message(groups=8, x_pixel_stride=23)
    assert 'strides' in message(x_pixel_stride=23, eps='nan') and 'eps' in message(eps='nan', act=5) and 'act must be' in message(act=5, act_param='nan')
    assert 'finite' in message(act_param='nan', out=P, out_pixel_stride=48) and 'in place' in message(out=P, out_pixel_stride=48, batch=65536)
    assert '65535' in message(batch=65536, workspace_bytes=0)


if __name__ == '__main__':
    at.child(table(), also=lambda lib: {'sizes': {'%d,%d,%d' % a: lib.opa_groupnorm_workspace_bytes(*a) for a in SIZES}})
