"""The truth table of the 16-bit MFMA routes' predicates (``fused.conv1x1_supported``, ``conv3x3_bf16_supported``,
``gconv3x3_bf16_supported``, ``stem7x7_bf16_supported``, ``pair_bf16_supported``, ``conv1x1_strided_bf16_supported``,
``head_conv_fields16_supported``): what each answers over a grid that CROSSES the causes of a decline, against
``tests/golden/routes16_truth.json`` as ``tests/golden/make_golden_routes16.py`` wrote it from the commit before the predicates
were rearranged.  The other host tests take one cause at a time; this one pins the combinations, the order of the early-outs
included: a case in which a predicate raises is recorded as ``raises:<ExceptionType>``, and one that answered False must go on
answering False.

The grid: per predicate an ordered list of axes (the first value of each is the base case's).  For each of the three operand dtypes:
the base case, every single deviation, and every pair of deviations on NEIGHBOURING axes.  Every case is asked under every on/off
combination of the route's own switches and ``F16``, with every other 16-bit switch off and again with every other one on.  One
character per case -- ``1`` True, ``0`` False, ``-`` torch cannot build the case's module, a letter for an exception type (the
file's ``legend``) -- one string per (predicate, switch setting).  Tensors of at most 5 x 4 pixels that say they are on the GPU
(``test_conv3x3_bf16_host.py``'s technique), the library reported as built.  No GPU is touched."""
import contextlib
import functools
import hashlib
import itertools
import json
import os

import torch
from torch import nn

from openpifpaf_amd import _lib, fused

import head16_common as hc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'routes16_truth.json')
CL = torch.channels_last
F32, F16, BF = torch.float32, torch.float16, torch.bfloat16
DTYPES = (F32, F16, BF)
SWITCHES16 = ('F16', 'CONV3_BF16', 'PAIR_BF16', 'GCONV_BF16', 'GCONV_F16', 'STEM7_BF16', 'STEM7_F16', 'HEAD16', 'UNIT_BF16', 'UNIT_F16')
DECLINED_SETS = ('PAIR_BF16_DECLINED', 'GCONV_BF16_DECLINED', 'GCONV_F16_DECLINED', 'STEM7_F16_DECLINED', 'HEAD16_DECLINED')
B, H, W = 2, 5, 4


class _OnDevice(torch.Tensor):
    is_cuda = True


class _Unbuildable(Exception):
    """torch refuses to build the module of a case (channels that the groups do not divide)."""


def _alternatives(dt):
    return [d for d in DTYPES if d != dt]


def _other16(dt):
    return F16 if dt == BF else BF


def _tensor(shape, dt, layout='cl', grad=False):
    """``[b, c, h, w]`` zeros of ``dt`` in one of the layouts of the operand axes."""
    b, c, h, w = shape
    if layout == 'zeropix':
        h = 0
    elif layout == 'wrongch':
        c += 64
    elif layout == 'wronghw':
        w += 1
    elif layout == 'batch3':
        b += 1
    elif layout in DTYPES:
        dt = layout
    if layout == 'nchw':
        t = torch.zeros((b, c, h, w), dtype=dt)
    elif layout == 'slice':
        t = torch.zeros((b, 2 * c, h, w), dtype=dt).contiguous(memory_format=CL)[:, :c]
    elif layout == 'misaligned':                       # one element behind a 16-byte boundary
        flat = torch.zeros(b * h * w * c + 8, dtype=dt)
        assert flat.data_ptr() % 16 == 0
        t = flat[1:1 + b * h * w * c].view(b, h, w, c).permute(0, 3, 1, 2)
    elif layout == 'expanded':                         # a stride of zero
        t = torch.zeros((b, 1, h, w), dtype=dt).expand(b, c, h, w)
    else:
        t = torch.zeros((b, c, h, w), dtype=dt).contiguous(memory_format=CL)
    if layout == 'dim3':
        t = t[0]
    if layout != 'cpu':
        t = t.as_subclass(_OnDevice)
    return t.requires_grad_() if grad else t


VECTOR_FORMS = ('same', 'none', 'f32', 'other16', 'wronglen', '2d', 'misaligned', 'noncontig')


def _vector(form, n, dt, grad=False):
    """A bias of ``n`` elements in one of the forms of the bias axes."""
    if form == 'none':
        return None
    if form == 'misaligned':
        t = torch.zeros(n + 8, dtype=dt)[1:1 + n]
    elif form == 'noncontig':
        t = torch.zeros(2 * n, dtype=dt)[::2]
    else:
        shape = {'wronglen': (n // 2,), '2d': (1, n)}.get(form, (n,))
        t = torch.zeros(shape, dtype={'f32': F32, 'other16': _other16(dt)}.get(form, dt))
    t = t.as_subclass(_OnDevice)
    return t.requires_grad_() if grad else t


@functools.lru_cache(maxsize=None)
def _module(kind, cin, cout, k, stride, padding, dilation, groups, own_bias, dt, wgrad=False, bgrad=False, bias_dt=None):
    """The module in the convolution's place; cached: no predicate writes to it."""
    if kind == 'linear':
        m = nn.Linear(cin, cout, bias=own_bias)
    elif kind == 'identity':
        return nn.Identity()
    else:
        try:
            m = nn.Conv2d(cin, cout, k, stride, padding, dilation=dilation, groups=groups, bias=own_bias)
        except ValueError as e:
            raise _Unbuildable(str(e))
    m = m.to(dt).requires_grad_(False)
    if own_bias and bias_dt is not None:
        m.bias = nn.Parameter(m.bias.detach().to(bias_dt), requires_grad=False)
    m.weight.requires_grad_(wgrad)
    if own_bias:
        m.bias.requires_grad_(bgrad)
    return m


def _s0(stride):
    return stride[0] if isinstance(stride, tuple) else stride


def _out_hw(s):
    return (H - 1) // s + 1, (W - 1) // s + 1


def _wdtype(spec, dt):
    return dt if spec['wdtype'] == 'same' else _alternatives(dt)[spec['wdtype'] == 'alt2']


def _conv_of(spec, dt, cin, cout, wgrad=False, bgrad=False, bias_dt=None):
    k, d = spec['kernel'], spec['dilation']
    padding = d * (k // 2) + (spec['padding'] == 'uneq')
    return _module(spec['module'], cin, cout, k, spec['stride'], padding, d, spec['groups'], spec['ownbias'], _wdtype(spec, dt),
                   wgrad, bgrad, bias_dt)


# ---- the axes ----------------------------------------------------------------------------------------------------------------------------

COMMON = [('wdtype', ('same', 'alt1', 'alt2')), ('autocast', (False, True)), ('grad', (False, True))]
LAYOUTS = ('cl', 'nchw', 'slice', 'misaligned', 'zeropix', 'wrongch', 'cpu', 'dim3')
THIRD = ('none', 'cl', 'nchw', 'slice', 'misaligned', 'wronghw', 'wrongch', 'batch3', 'cpu', F32, F16, BF)


def _geometry(kernel, groups=(1, 2, 32), own_bias=(False, True)):
    return [('module', ('conv', 'linear', 'identity')), ('kernel', (kernel,) + tuple(k for k in (1, 3, 5, 7) if k != kernel)),
            ('stride', (1, 2, 3, (1, 2))), ('dilation', (1, 2, 3, 4)), ('padding', ('eq', 'uneq')), ('groups', groups),
            ('ownbias', own_bias)]


def _conv1x1(spec, dt):
    k, n, who = spec['channels'], spec['nout'], spec['who']
    weight = torch.zeros((n, k, 1, 1), dtype=_wdtype(spec, dt)).as_subclass(_OnDevice).requires_grad_(who == 'weight')
    third = 'cl' if who == 'third' and spec['third'] == 'none' else spec['third']
    residual = None if third == 'none' else _tensor((B, n, H, W), dt, third, who == 'third')
    abias = 'same' if who == 'abias' and spec['abias'] == 'none' else spec['abias']
    return fused.conv1x1_supported, (_tensor((B, k, H, W), dt, spec['layout'], who == 'x'), weight, _vector(spec['bias'], n, dt, who == 'bias'),
                                     residual, _vector(abias, k, dt, who == 'abias')), {}


def _conv3(spec, dt):
    c, n, who = spec['channels'], spec['nout'], spec['who']
    conv = _conv_of(spec, dt, c, n, wgrad=who == 'weight')
    third = 'cl' if who == 'third' and spec['third'] == 'none' else spec['third']
    residual = None if third == 'none' else _tensor((B, n) + _out_hw(_s0(spec['stride'])), dt, third, who == 'third')
    return fused.conv3x3_bf16_supported, (conv, _tensor((B, c, H, W), dt, spec['layout'], who == 'x'),
                                          _vector(spec['bias'], n, dt, who == 'bias'), residual), {}


def _gconv(spec, dt):
    c, who = spec['channels'], spec['who']
    n = c if spec['nout'] == 'same' else spec['nout']
    conv = _conv_of(spec, dt, c, n, wgrad=who == 'weight')
    key = (c, c // spec['groups'], _s0(spec['stride']))
    return fused.gconv3x3_bf16_supported, (conv, _tensor((B, c, H, W), dt, spec['layout'], who == 'x'),
                                           _vector(spec['bias'], n, dt, who == 'bias')), {spec['declined']: key}


def _stem(spec, dt):
    n, who, groups = spec['nout'], spec['who'], spec['groups']
    if groups == 3 and n % 3:
        n = 192                                        # (torch builds no 3-group convolution of 64 output channels)
    conv = _conv_of(spec, dt, spec['cin'], n, wgrad=who == 'weight')
    x = _tensor((B, 3, H, W), dt, spec['layout'], who == 'x')
    if spec['layout'] == 'wrongch':
        x = _tensor((B, 4, H, W), dt, 'cl', who == 'x')
    key = (n, _s0(spec['stride']), False)
    return fused.stem7x7_bf16_supported, (conv, x, _vector(spec['bias'], n, dt, who == 'bias'), spec['pooled']), {spec['declined']: key}


CONV_FORMS = {'plain': {}, 'k3': dict(kernel=3), 'stride2': dict(stride=2), 'ownbias': dict(ownbias=True), 'groups2': dict(groups=2),
              'dilation2': dict(dilation=2), 'uneq': dict(padding='uneq'), 'linear': dict(module='linear'),
              'identity': dict(module='identity'), 'alt1': dict(wdtype='alt1'), 'alt2': dict(wdtype='alt2'), 'nout64': {}}


def _pair(spec, dt):
    k1, k2, n, who = spec['channels'], spec['k2'], spec['nout'], spec['who']
    base = dict(module='conv', kernel=1, stride=1, dilation=1, padding='eq', groups=1, ownbias=False, wdtype='same')
    conv = _conv_of(dict(base, **CONV_FORMS[spec['conv']]), dt, k1, 64 if spec['conv'] == 'nout64' else n, wgrad=who == 'weight')
    dconv = _conv_of(spec, dt, k2, n, wgrad=who == 'dweight')
    s = _s0(spec['stride'])
    abias = 'same' if who == 'abias' and spec['abias'] == 'none' else spec['abias']
    return fused.pair_bf16_supported, (conv, dconv, _tensor((B, k1) + _out_hw(s), dt, spec['third'], who == 'third'),
                                       _tensor((B, k2, H, W), dt, spec['layout'], who == 'x'), _vector(spec['bias'], n, dt, who == 'bias'),
                                       _vector(abias, k1, dt, who == 'abias')), {spec['declined']: (k1, k2, n, s)}


def _strided(spec, dt):
    k2, n, who = spec['channels'], spec['nout'], spec['who']
    dconv = _conv_of(spec, dt, k2, n, wgrad=who == 'weight')
    return fused.conv1x1_strided_bf16_supported, (dconv, _tensor((B, k2, H, W), dt, spec['layout'], who == 'x')), \
        {spec['declined']: (0, k2, n, _s0(spec['stride']))}


METAS = {'cif3x2': ('cif', 3, 2), 'caf2x1': ('caf', 2, 1), 'cifdet4x2': ('cifdet', 4, 2), 'cif3x3': ('cif', 3, 3), 'cif4x2': ('cif', 4, 2)}


@functools.lru_cache(maxsize=None)
def _meta(name):
    return hc.meta(*METAS[name])


def _head(spec, dt):
    k, who = spec['channels'], spec['who']
    meta = _meta(spec['meta'])
    n = 60 if spec['nout'] == 'cif3x2' else meta.n_fields * hc.n_components(meta) * meta.upsample_stride ** 2
    bias_dt = {'same': None, 'f32': F32, 'other16': _other16(dt)}[spec['bias']]
    conv = _conv_of(spec, dt, k, n, wgrad=who == 'weight', bgrad=who == 'bias', bias_dt=bias_dt)
    return fused.head_conv_fields16_supported, (conv, _tensor((B, k, H, W), dt, spec['layout'], who == 'x'), meta, spec['training']), \
        {spec['declined']: (k, n, meta.upsample_stride)}


BUILT = [('built', (True, False))]
# predicate -> (the route's own switches, the builder of a case, its axes in the order whose neighbours are crossed)
PREDICATES = {
    'conv1x1_supported': (('F16',), _conv1x1, COMMON + [
        ('who', ('nobody', 'x', 'weight', 'bias', 'third', 'abias')), ('channels', (64, 128, 96, 72, 32)), ('nout', (128, 64, 96, 72)),
        ('bias', VECTOR_FORMS), ('abias', ('none',) + tuple(f for f in VECTOR_FORMS if f != 'none')), ('layout', LAYOUTS), ('third', THIRD)]),
    'conv3x3_bf16_supported': (('CONV3_BF16', 'F16'), _conv3, COMMON + [
        ('who', ('nobody', 'x', 'weight', 'bias', 'third'))] + _geometry(3) + [
        ('channels', (64, 128, 96, 72)), ('nout', (128, 64, 96, 72)), ('bias', VECTOR_FORMS), ('layout', LAYOUTS), ('third', THIRD)] + BUILT),
    'gconv3x3_bf16_supported': (('GCONV_BF16', 'GCONV_F16', 'F16'), _gconv, COMMON + [
        ('who', ('nobody', 'x', 'weight', 'bias'))] + _geometry(3, groups=(32, 2, 1)) + [
        ('channels', (128, 64, 96, 72)), ('nout', ('same', 256)), ('bias', VECTOR_FORMS), ('layout', LAYOUTS),
        ('declined', ('none', 'GCONV_BF16_DECLINED', 'GCONV_F16_DECLINED'))] + BUILT),
    'stem7x7_bf16_supported': (('STEM7_BF16', 'STEM7_F16', 'F16'), _stem, COMMON + [
        ('who', ('nobody', 'x', 'weight', 'bias'))] + _geometry(7, groups=(1, 3)) + [
        ('cin', (3, 4)), ('nout', (64, 128, 96, 72)), ('bias', VECTOR_FORMS), ('layout', LAYOUTS + ('expanded',)),
        ('declined', ('none', 'STEM7_F16_DECLINED')), ('pooled', (False, True))] + BUILT),
    'pair_bf16_supported': (('PAIR_BF16', 'F16'), _pair, COMMON + [
        ('who', ('nobody', 'x', 'weight', 'dweight', 'bias', 'abias', 'third')), ('conv', tuple(CONV_FORMS))] + _geometry(1) + [
        ('channels', (64, 128, 96, 72)), ('k2', (128, 64, 96, 72)), ('nout', (128, 64, 96, 72)), ('bias', VECTOR_FORMS),
        ('abias', ('none',) + tuple(f for f in VECTOR_FORMS if f != 'none')), ('layout', LAYOUTS), ('third', THIRD[1:]),
        ('declined', ('none', 'PAIR_BF16_DECLINED'))] + BUILT),
    'conv1x1_strided_bf16_supported': (('PAIR_BF16', 'F16'), _strided, COMMON + [
        ('who', ('nobody', 'x', 'weight'))] + _geometry(1) + [
        ('channels', (64, 128, 96, 72)), ('nout', (128, 64, 96, 72)), ('layout', LAYOUTS), ('declined', ('none', 'PAIR_BF16_DECLINED'))] + BUILT),
    'head_conv_fields16_supported': (('HEAD16', 'F16'), _head, COMMON + [
        ('who', ('nobody', 'x', 'weight', 'bias')), ('training', (False, True))] + _geometry(1, own_bias=(True, False)) + [
        ('channels', (64, 128, 96, 72)), ('nout', ('meta', 'cif3x2')), ('meta', tuple(METAS)), ('bias', ('same', 'f32', 'other16')),
        ('layout', LAYOUTS), ('declined', ('none', 'HEAD16_DECLINED'))] + BUILT),
}


def specs(axes):
    """The base case, every single deviation, every pair of deviations on neighbouring axes."""
    base = {name: values[0] for name, values in axes}
    yield base
    for name, values in axes:
        for v in values[1:]:
            yield dict(base, **{name: v})
    for (n1, v1), (n2, v2) in zip(axes, axes[1:]):
        for a, b in itertools.product(v1[1:], v2[1:]):
            yield dict(base, **{n1: a, n2: b})


def settings(own):
    """Every on/off combination of the route's own switches, every other 16-bit switch off, then on."""
    for others in (False, True):
        for values in itertools.product((False, True), repeat=len(own)):
            yield dict({name: others for name in SWITCHES16}, **dict(zip(own, values)))


def _setting_name(own, setting):
    others = next(v for name, v in setting.items() if name not in own)
    return ','.join('%s=%d' % (name, setting[name]) for name in own) + ',others=%d' % others


@contextlib.contextmanager
def _patched(targets):
    """``[(object, attribute, value)]`` set for the block and put back after it."""
    saved = [(obj, name, getattr(obj, name)) for obj, name, _ in targets]
    try:
        for obj, name, value in targets:
            setattr(obj, name, value)
        yield
    finally:
        for obj, name, value in reversed(saved):
            setattr(obj, name, value)


def _answer(fn, args, legend):
    try:
        return '1' if fn(*args) else '0'
    except Exception as e:                      # noqa: BLE001 -- the type of whatever is raised IS the record
        name = 'raises:' + type(e).__name__
        if name not in legend:
            legend[name] = 'ABCDEFGHIJKLMNOPQRSTUVWXYZ'[len(legend)]
        return legend[name]


def record():
    """-> the document of ``routes16_truth.json``."""
    legend, answers, grid, total = {}, {}, {}, 0
    for predicate, (own, build, axes) in PREDICATES.items():
        labels = []
        rows = {_setting_name(own, s): [] for s in settings(own)}
        for dt in DTYPES:
            for spec in specs(axes):
                labels.append(str(dt) + ' ' + ' '.join('%s=%s' % kv for kv in spec.items()))
                environment = [(_lib, 'available', lambda built=spec.get('built', True): built)]
                if spec['autocast']:
                    environment.append((torch, 'is_autocast_enabled', lambda *a: True))
                with torch.set_grad_enabled(spec['grad']), _patched(environment):
                    try:
                        fn, args, declined = build(spec, dt)
                    except _Unbuildable:
                        fn = None
                    for setting in settings(own):
                        if fn is None:
                            rows[_setting_name(own, setting)].append('-')
                            continue
                        sets = [(fused, name, frozenset({declined[name]} if name in declined else ())) for name in DECLINED_SETS]
                        with _patched([(fused, name, value) for name, value in setting.items()] + sets):
                            rows[_setting_name(own, setting)].append(_answer(fn, args, legend))
        answers[predicate] = {name: ''.join(row) for name, row in rows.items()}
        grid[predicate] = {'cases': len(labels), 'labels_sha1': hashlib.sha1('\n'.join(labels).encode()).hexdigest()}
        total += len(labels) * len(rows)
    return {'about': 'tests/test_routes16_truth_host.py: %d answers of %d predicates (cases x switch settings); written by '
                     'tests/golden/make_golden_routes16.py' % (total, len(PREDICATES)),
            'legend': dict({'1': True, '0': False, '-': 'torch cannot build the module'}, **{v: k for k, v in legend.items()}),
            'grid': grid, 'answers': answers}


def test_every_predicate_answers_what_it_answered_before_the_rearrangement():
    with open(GOLDEN) as f:
        golden = json.load(f)
    got = json.loads(json.dumps(record()))
    assert got['grid'] == golden['grid'], 'the grid itself changed: the golden file pins the answers of the grid it was written from'
    for predicate, rows in golden['answers'].items():
        for setting, want in rows.items():
            have = got['answers'][predicate][setting]
            differing = [i for i, (a, b) in enumerate(zip(have, want)) if a != b]
            assert have == want, (predicate, setting, 'cases', differing[:10], [(have[i], want[i]) for i in differing[:10]])
    assert got['legend'] == golden['legend'] and got['about'] == golden['about']
    # the grid shows something: every predicate says yes somewhere, and no somewhere with every switch on
    for predicate, rows in golden['answers'].items():
        assert any('1' in row for row in rows.values()) and all('0' in row for row in rows.values()), predicate
