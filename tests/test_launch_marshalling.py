"""What every launcher of ``fused.py`` and ``winograd.py`` hands to the C ABI, argument by argument, without a GPU: the launchers do
not ask where their tensors live (the ``*_supported`` predicates do), so they run here on small CPU tensors against a stand-in for
``_lib.lib()`` that calls nothing and returns 0.  Per native call the symbol and every argument are recorded: an integer as it is,
a pointer as the label of the input tensor it addresses (``x``, ``bias``, ... as the case names them; a derived operand the launcher
keeps on the module under the names the case gives it), ``new<i>`` for the i-th tensor the launcher allocated itself, ``null``.
``ctypes.c_void_p`` objects and plain integers are read alike.  Recorder, labels and comparison are ``abi_tables.py``'s; the record is
compared with ``golden/launch_marshalling.json`` (``golden/make_golden_abi.py launch_marshalling``): an argument that moves, a pitch taken from the wrong tensor, an activation code
that changes shows as a difference in one line.

``bias_act_`` and ``channel_interleave`` do ask ``is_cuda`` before they launch: they get a tensor subclass that answers yes."""
import ctypes
import itertools

import torch
from torch import nn

from openpifpaf_amd import fused, headmeta, winograd

import abi_tables as at

GOLDEN = at.golden('launch_marshalling')
CL = torch.channels_last
F32, BF16 = torch.float32, torch.bfloat16
# every symbol fused.py and winograd.py launch (the two retired twins under the name of their superset: ``canonical``)
SYMBOLS = {'opa_bias_act', 'opa_gemm_bias_act_bf16', 'opa_gemm_pro_bias_act_bf16', 'opa_gemm_bias_act_f32', 'opa_gemm_bias_act_f32x3',
           'opa_gemm_unit_act_f32x3', 'opa_conv_rows_f32x3', 'opa_conv3x3_f32x3', 'opa_gemm2_bias_act_f32x3', 'opa_conv3x3_winograd_f32',
           'opa_conv3x3_winograd_f32x3', 'opa_dwconv_act', 'opa_gconv3x3_bias_act_f32', 'opa_se_workspace_bytes', 'opa_se_pool',
           'opa_se_gate', 'opa_se_scale', 'opa_channel_interleave', 'opa_head_epilogue'}


class _OnDevice(torch.Tensor):
    is_cuda = True


def _act(b, c, h, w, dtype=F32):
    return torch.zeros((b, c, h, w), dtype=dtype).contiguous(memory_format=CL)


def _slice(b, c, h, w, dtype=F32, extra=6, start=2):
    return _act(b, c + extra, h, w, dtype)[:, start:start + c]


def _dev(t):
    return t.as_subclass(_OnDevice)


def _cached_on(module, *names):
    """The one derived operand (``fused.derived``) the launcher left on ``module``, a tensor or a tuple of them -> {label: tensor}."""
    attrs = [a for a in vars(module) if a.startswith('_opa_')]
    assert len(attrs) == 1, attrs
    value = getattr(module, attrs[0])[1]
    value = value if isinstance(value, tuple) else (value,)
    assert len(value) == len(names), (attrs, len(value), names)
    return {n: t for n, t in zip(names, value) if t is not None}


def cases():
    """-> {case id: (call, {label: input tensor}, derived operands after the call -> {label: tensor} or None, ``fused.X3_TERMS``)}"""
    out = {}

    def add(case_id, call, tensors, derived=None, terms=6):
        assert case_id not in out, case_id
        out[case_id] = (call, tensors, derived, terms)

    def flags(n):
        return itertools.product((False, True), repeat=n)

    # ---- the epilogue pass, the interleave pass -----------------------------------------------------------------------------
    for dtype in (F32, BF16):
        x, b, r = _dev(_act(2, 8, 3, 5, dtype)), torch.zeros(8, dtype=dtype), _act(2, 8, 3, 5, dtype)
        for has_res, relu in flags(2):
            add('bias_act/%s/res%d/relu%d' % (dtype, has_res, relu),
                lambda x=x, b=b, res=r if has_res else None, relu=relu: fused.bias_act_(x, b, res, relu), dict(x=x, bias=b, residual=r))
        p, q = _dev(_act(2, 8, 3, 5, dtype)), _dev(_slice(2, 8, 3, 5, dtype))
        add('interleave/%s' % dtype, lambda p=p, q=q: fused.channel_interleave(p, q), dict(a=p, b=q))
        add('interleave/%s/swapped' % dtype, lambda p=p, q=q: fused.channel_interleave(q, p), dict(a=q, b=p))
    x2, b2 = _dev(torch.zeros((6, 8))), torch.zeros(8)
    add('bias_act/rows', lambda: fused.bias_act_(x2, b2, None, True), dict(x=x2, bias=b2))

    # ---- the 1x1 GEMMs ------------------------------------------------------------------------------------------------------
    for dtype in (F32, BF16):
        x, w, b = _act(2, 64, 3, 5, dtype), torch.zeros((128, 64), dtype=dtype), torch.zeros(128, dtype=dtype)
        r, ab = _act(2, 128, 3, 5, dtype), torch.zeros(64, dtype=dtype)
        for has_res, has_ab, relu in flags(3):
            add('gemm/%s/res%d/abias%d/relu%d' % (dtype, has_res, has_ab, relu),
                lambda x=x, w=w, b=b, res=r if has_res else None, relu=relu, a=ab if has_ab else None: fused.conv1x1_bias_act(x, w, b, res, relu, a),
                dict(x=x, weight=w, bias=b, residual=r, a_bias=ab))
    x, w3, b = _act(2, 64, 3, 5), torch.zeros((3, 128, 64), dtype=BF16), torch.zeros(128)
    r, ab = _act(2, 128, 3, 5), torch.zeros(64)
    for terms in (6, 9):
        for has_res, has_ab, relu in flags(3):
            add('gemm3/terms%d/res%d/abias%d/relu%d' % (terms, has_res, has_ab, relu),
                lambda res=r if has_res else None, relu=relu, a=ab if has_ab else None, terms=terms:
                fused.conv1x1_bias_act_x3(x, w3, b, res, relu, a, terms), dict(x=x, w3=w3, bias=b, residual=r, a_bias=ab))
    add('gemm3/defaults', lambda: fused.conv1x1_bias_act_x3(x, w3, b), dict(x=x, w3=w3, bias=b))

    # ---- the pair product, the strided and grouped 3x3, the stem, the heads (module attribute X3_TERMS) -----------------------
    for terms in (6, 9):
        for stride in (1, 2):
            conv, dconv = nn.Conv2d(16, 32, 1, bias=False), nn.Conv2d(8, 32, 1, stride, bias=False)     # (small: nothing here checks a tile)
            h, xx, pb, pab = _act(2, 16, 3, 2) if stride == 2 else _act(2, 16, 5, 3), _act(2, 8, 5, 3), torch.zeros(32), torch.zeros(16)
            for has_ab, relu in flags(2):
                add('pair/terms%d/stride%d/abias%d/relu%d' % (terms, stride, has_ab, relu),
                    lambda conv=conv, dconv=dconv, h=h, xx=xx, pb=pb, relu=relu, a=pab if has_ab else None:
                    fused.conv1x1_pair_bias_act_x3(conv, dconv, h, xx, pb, relu, a), dict(h=h, x=xx, bias=pb, a_bias=pab),
                    lambda conv=conv: _cached_on(conv, 'w3', 'a_bias_padded'), terms)
            conv3 = nn.Conv2d(16, 32, 3, stride, 1, bias=False)
            cx, cb = _act(2, 16, 5, 3), torch.zeros(32)
            gconv = nn.Conv2d(16, 16, 3, stride, 1, groups=4, bias=False)
            gb = torch.zeros(16)
            for relu in (False, True):
                add('conv3x3/terms%d/stride%d/relu%d' % (terms, stride, relu),
                    lambda conv3=conv3, cx=cx, cb=cb, relu=relu: fused.conv3x3_bias_act_x3(conv3, cx, cb, relu), dict(x=cx, bias=cb),
                    lambda conv3=conv3: _cached_on(conv3, 'w3'), terms)
                for has_bias in (False, True):
                    add('gconv/terms%d/stride%d/bias%d/relu%d' % (terms, stride, has_bias, relu),
                        lambda gconv=gconv, cx=cx, bias=gb if has_bias else None, relu=relu: fused.gconv3x3_bias_act(gconv, cx, bias, relu),
                        dict(x=cx, bias=gb), lambda gconv=gconv: _cached_on(gconv, 'weight_taps'), terms)
        stem, sx, sb = nn.Conv2d(3, 64, 7, 2, 3, bias=False), torch.zeros((2, 3, 9, 6)), torch.zeros(64)
        for relu in (False, True):
            add('stem/terms%d/relu%d' % (terms, relu), lambda stem=stem, sx=sx, sb=sb, relu=relu: fused.stem7x7_bias_act_x3(stem, sx, sb, relu),
                dict(x=sx, bias=sb), lambda stem=stem: _cached_on(stem, 'w3'), terms)
        hx = _act(2, 64, 3, 5)
        for n, has_bias in ((40, True), (40, False), (128, True)):
            head = nn.Conv2d(64, n, 1, bias=has_bias)
            add('head_conv/terms%d/n%d/bias%d' % (terms, n, has_bias), lambda head=head, hx=hx: fused.head_conv_x3(head, hx), dict(x=hx),
                lambda head=head: _cached_on(head, 'w3', 'bias_padded'), terms)

    # ---- the unit mode --------------------------------------------------------------------------------------------------------
    acts = ((True, None), (False, None), (True, fused.ACT_NONE), (False, fused.ACT_RELU), (False, fused.ACT_HARDSWISH))
    for terms in (6, 9):
        for layout in ('dense', 'slices'):
            unit = nn.Conv2d(72, 40, 1, bias=terms == 6)
            make = _act if layout == 'dense' else _slice
            ux, third = make(2, 72, 3, 5), make(2, 40, 3, 5) if layout == 'dense' else _slice(2, 40, 3, 5, extra=10, start=4)
            for what, (relu, act) in itertools.product(('alone', 'partner', 'residual'), acts):
                kwargs = {} if what == 'alone' else {what: third}
                if act is not None:
                    kwargs['act'] = act
                add('unit/terms%d/%s/%s/relu%d/act%s' % (terms, layout, what, relu, act),
                    lambda unit=unit, ux=ux, relu=relu, kwargs=kwargs: fused.conv1x1_unit_x3(unit, ux, relu, **kwargs), {'x': ux, what: third},
                    lambda unit=unit: _cached_on(unit, 'w3', 'bias_padded'), terms)
    unit, ux = nn.Conv2d(72, 40, 1), _act(2, 72, 3, 5)
    add('unit/defaults', lambda: fused.conv1x1_unit_x3(unit, ux), dict(x=ux), lambda: _cached_on(unit, 'w3', 'bias_padded'))

    # ---- the depthwise stencil ------------------------------------------------------------------------------------------------
    for dtype, layout in ((F32, 'dense'), (F32, 'slice'), (BF16, 'dense')):
        dx = _act(2, 8, 7, 5, dtype) if layout == 'dense' else _slice(2, 8, 7, 5, dtype)
        db = torch.zeros(8, dtype=dtype)
        for k, stride in itertools.product((3, 5), (1, 2)):
            taps = torch.zeros((k * k, 8), dtype=dtype)
            for has_bias, (relu, act) in itertools.product((False, True), acts):
                kwargs = {} if act is None else {'act': act}
                add('dwconv/%s/%s/k%d/stride%d/bias%d/relu%d/act%s' % (dtype, layout, k, stride, has_bias, relu, act),
                    lambda dx=dx, taps=taps, bias=db if has_bias else None, k=k, stride=stride, relu=relu, kwargs=kwargs:
                    fused.dwconv_bias_act(dx, taps, bias, k, stride, relu, **kwargs), dict(x=dx, w_taps=taps, bias=db))
    dx, taps, db = _act(2, 8, 7, 5), torch.zeros((9, 8)), torch.zeros(8)
    add('dwconv/defaults', lambda: fused.dwconv_bias_act(dx, taps, db, 3, 1), dict(x=dx, w_taps=taps, bias=db))

    # ---- squeeze and excitation -------------------------------------------------------------------------------------------------
    fc1, fc2 = nn.Conv2d(8, 4, 1), nn.Conv2d(4, 8, 1)
    gate, mean = torch.zeros((2, 8)), torch.zeros((2, 8))
    for layout in ('dense', 'slice'):
        sx = _act(2, 8, 33, 17) if layout == 'dense' else _slice(2, 8, 33, 17, extra=8, start=4)
        se_tensors = {'x': sx, 'fc1.weight': fc1.weight, 'fc1.bias': fc1.bias, 'fc2.weight': fc2.weight, 'fc2.bias': fc2.bias, 'mean_out': mean}
        for has_mean in (False, True):
            add('se_gate/%s/mean%d' % (layout, has_mean), lambda sx=sx, m=mean if has_mean else None: fused.se_gate(sx, fc1, fc2, m), se_tensors)
        add('se_scale/%s' % layout, lambda sx=sx: fused.scale_channels_(sx, gate), dict(x=sx, gate=gate))

    # ---- the head epilogue ------------------------------------------------------------------------------------------------------
    for i, meta in enumerate(headmeta.cocokp_metas()):
        n_comp = 1 + meta.n_confidences + meta.n_vectors * 2 + meta.n_scales
        for dtype in (F32, BF16):
            ex = _act(2, meta.n_fields * n_comp * meta.upsample_stride ** 2, 3, 5, dtype)
            add('head_epilogue/meta%d/%s' % (i, dtype), lambda ex=ex, meta=meta: fused.head_epilogue(ex, meta), dict(x=ex))

    # ---- Winograd ---------------------------------------------------------------------------------------------------------------
    wx, u, wb, wout = _act(2, 16, 5, 3), torch.zeros(64), torch.zeros(64), _act(2, 64, 5, 3)
    for fn, name in ((winograd.conv3x3, 'wino'), (winograd.conv3x3_x3, 'wino_x3')):
        for has_bias, relu, has_out in flags(3):
            add('%s/bias%d/relu%d/out%d' % (name, has_bias, relu, has_out),
                lambda fn=fn, bias=wb if has_bias else None, relu=relu, o=wout if has_out else None: fn(wx, u, 64, bias=bias, relu=relu, out=o),
                dict(x=wx, u=u, bias=wb, out=wout))
        add('%s/defaults' % name, lambda fn=fn: fn(wx, u, 64), dict(x=wx, u=u))
        add('%s/variant_order' % name, lambda fn=fn: fn(wx, u, 64, variant=2, order=1), dict(x=wx, u=u))
    return out


def record_all():
    """-> {case id: [[symbol, [arguments]], ...]}"""
    return at.record_all(cases())


def test_every_launch_hands_over_what_the_golden_file_says():
    got = at.marshalling(cases(), GOLDEN)
    assert all(calls for calls in got.values())
    assert {name for calls in got.values() for name, _ in calls} == SYMBOLS


def test_a_pointer_is_read_alike_as_an_object_and_as_an_integer():
    t = torch.zeros(4)
    raw = [('opa_se_scale', (ctypes.c_void_p(t.data_ptr()), 4, 1, 1, 4, None, ctypes.c_void_p(at.STREAM))),
           ('opa_se_scale', (t.data_ptr(), 4, 1, 1, 4, ctypes.c_void_p(None), at.STREAM))]
    a, b = at.normalise(raw, {t.data_ptr(): 'x'})
    assert a == b == ['opa_se_scale', ['x', 4, 1, 1, 4, 'null', 'stream']]
