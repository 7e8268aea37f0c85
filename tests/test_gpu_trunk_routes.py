"""Every dispatch route of the fused trunk, one MODULE at a time, against the float64 module (real kernels, MI355X).

The module is built unfused, in ``eval()``, with random BatchNorm statistics (``trunk_common.randomize_``: the folded biases are of
the activations' size).  ``ref64`` is its ``double()`` copy applied to ``x.double()``; ``e0`` is the error of the SAME unfused module
in the test's dtype (PyTorch / MIOpen) against ``ref64`` (the median of nine calls, ``_median_error``); the module under test is its folded + ``enable_fused_()`` copy,
channels_last.  ``err = max |got - ref64| / max |ref64|`` and the same as an rms, three seeds.  Per route:

1. ``err <= K[family] * e0`` (max and rms), never looser than the sum of the single-kernel bars on the route
   (``2e-6 * sqrt(K)`` per float32 GEMM, ``2e-5`` per Winograd launch; a MIOpen step counts ``e0``).  ``K`` was chosen from
   ``profiles/trunk_routes/route_errors.log`` as the smallest of 2, 4, 8 that holds for every seed of the family.
2. the first call equals the second bit for bit, and the second call's LAUNCH TRACE (recorded at the Python launchers and by a
   forward hook on every ``nn.Conv2d``) is the route that was asked for -- a forced route that fell back to MIOpen fails here.
   One of MIOpen's own solvers adds partial sums with atomics and does not repeat (fixture ``rec``): a route THROUGH a MIOpen
   convolution that is seen to differ between two calls is compared at ``K * e0`` instead (max 1.7 e0 seen: one float32 ulp of the
   head's largest outputs); a route of the project's kernels alone has to repeat bit for bit;
3. the input is bit-identical after the forward, and a forward on a fresh clone of it gives the same bits;
4. (captured) the replayed graph equals the eager run with the remembered choices, bit for bit.

Decision value -> tests that run it (bottleneck shapes ``a``: identity 256->64, ``b``: downsample stride 1 128->64, ``c``: downsample
stride 2 256->64, H odd; ``n32`` / ``n48``: planes 32 / 48; every listed test runs seeds 0, 1, 2):

====================================  ==============================================================================
conv1 ``gemm`` / ``gemm3`` / ``conv``   test_bottleneck_conv1_routes[*]  (no residual, no a_bias); rotated through
                                      test_bottleneck_float32_matrix[*] as well
conv2 Winograd variant 4 / variant 2  test_bottleneck_float32_matrix[a|b-wino4|wino2-*]  x every tail
conv2 ``pick('conv3')`` x3 / conv     test_bottleneck_float32_matrix[a|b|c-conv3:x3|conv3:conv-*]  x every tail
conv2 raw MIOpen, bias deferred       test_bottleneck_float32_matrix[a|b|c-raw-*], test_bottleneck_bfloat16[*],
                                      test_widths_the_kernels_must_decline[*]
tail ``pick('pair')`` x3              ...matrix[b|c-*-pair] (a_bias applied: conv2 != raw; deferred: conv2 = raw),
                                      test_widths...[n32] (deferred, K1 = 32)
tail ``gemm`` / ``gemm3`` / ``conv``    ...matrix[*-gemm|gemm3|conv] (residual; applied and deferred); bfloat16: gemm, conv (deferred)
tail ``pass+gemm``                    ...matrix[a|b|c-raw-pass+gemm], test_bottleneck_bfloat16[*-pass+gemm]  (deferred only)
conv2 x tail, every adjacent pair     the full product in test_bottleneck_float32_matrix
``X3_TERMS`` 9 / ``X3_PAIR`` off        test_nine_terms_and_the_pair_switch
timed first call                      test_timed_first_call[c-deferred|c-auto|b-auto], test_timed_pair_with_the_inner_choice_pinned
                                      [pass+gemm|conv|gemm|gemm3], test_stem[timed-*], test_head[timed-*]
first call under capture              test_first_call_under_capture[small|large] (-> conv / x3 by size),
                                      test_stem[captured-*], test_head[captured-*]
``_BasicBlock``                       test_basic_block[*]  (Winograd variant 4 / 2 / MIOpen; identity and downsample residual)
``_InvertedResidualK``                test_inverted_residual[*]  (one route: dwconv + interleave; float32, bfloat16)
stem ``pick('stem')`` x3 / conv / off test_stem[forced:x3|forced:conv|terms9|off-*]
head ``pick('head')`` x3 / conv / off test_head[forced:x3|forced:conv|terms9|off-cif|caf]
operands after a parameter event      test_forward_after_a_parameter_event[*]  (``winograd.X3`` on and off)
====================================  ==============================================================================
"""
import copy
import functools
import math

import pytest
import torch
from torch import nn

from openpifpaf_amd import fused, headmeta, network, winograd

import trunk_common as tc

pytestmark = pytest.mark.gpu

SEEDS = (0, 1, 2)
# the smallest of 2, 4, 8 that holds for every seed of every route of the family (profiles/trunk_routes/route_errors.log)
K = {'float32': 2, 'winograd': 2, 'bfloat16': 2}
CL = torch.channels_last

_LAUNCHERS = {(fused, 'conv1x1_bias_act'): 'gemm', (fused, 'conv1x1_bias_act_x3'): 'gemm3', (fused, 'conv1x1_pair_bias_act_x3'): 'pair',
              (fused, 'conv3x3_bias_act_x3'): 'conv3x3_x3', (fused, 'stem7x7_bias_act_x3'): 'stem_x3', (fused, 'head_conv_x3'): 'head_x3',
              (fused, 'bias_act_'): 'bias_act', (fused, 'head_epilogue'): 'head_epilogue', (fused, 'dwconv_bias_act'): 'dwconv',
              (fused, 'channel_interleave'): 'interleave', (winograd, 'conv3x3'): 'wino2', (winograd, 'conv3x3_x3'): 'wino4'}
_SWITCHES = [(fused, 'FORCE_PICK'), (fused, 'X3_TERMS'), (fused, 'X3_PAIR'), (fused, 'X3_CONV3'), (fused, 'X3_STEM'), (fused, 'X3_HEAD'),
             (winograd, 'X3')]


class _Recorder:
    def __init__(self):
        self.trace = []
        self.timed = 0
        self.log = []
        self.case = None          # (e0, max |ref64|, dtype) of the case in hand

    def watch(self, module):
        """MIOpen's convolutions: every ``nn.Conv2d`` of ``module`` that is CALLED (the kernels read ``conv.weight`` instead)."""
        for name, m in module.named_modules():
            if isinstance(m, nn.Conv2d):
                m.register_forward_hook(lambda mod, args, out, name=name: self.trace.append('miopen:' + name))
        return module


@pytest.fixture
def rec(monkeypatch):
    """Launch recorder + every switch and the choice table saved and restored; the table starts EMPTY, nothing forced.

    MIOpen runs as the product runs it.  Its ConvAsmImplicitGemmGTCDynamicFwdXdlopsNHWC solver splits K across workgroups for
    some shapes (kernels ``igemm_fwd_gtcx35_nhwc_*_gkgs``: the 1x1 convolutions with 256 input channels here, float32 and
    bfloat16) and adds the parts with atomics: ten calls of one convolution gave eight to ten different outputs.  A route through
    a MIOpen convolution may therefore differ between two calls, by at most the family's ``K * e0`` (``_same``); a route of the
    project's kernels alone may not differ at all.  (``torch.backends.cudnn.deterministic`` is no way out: the solver it selects
    here is MIOpen's naive one, which ``MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_FWD=0`` -- set by ``bench.py`` on import -- removes.)"""
    r = _Recorder()
    for (mod, attr), label in _LAUNCHERS.items():
        real = getattr(mod, attr)

        def wrapper(*args, _real=real, _label=label, **kwargs):
            r.trace.append(_label)
            return _real(*args, **kwargs)
        monkeypatch.setattr(mod, attr, wrapper)
    real_time = fused._time_ms

    def time_ms(fn, reps=3):
        r.timed += 1
        return real_time(fn, reps)
    monkeypatch.setattr(fused, '_time_ms', time_ms)
    for mod, attr in _SWITCHES:
        monkeypatch.setattr(mod, attr, getattr(mod, attr))
    monkeypatch.setattr(fused, 'FORCE_PICK', None)
    monkeypatch.setattr(fused, 'X3_TERMS', 6)
    for attr in ('X3_PAIR', 'X3_CONV3', 'X3_STEM', 'X3_HEAD'):
        monkeypatch.setattr(fused, attr, True)
    monkeypatch.setattr(winograd, 'X3', True)
    monkeypatch.delenv('OPA_CONV1X1', raising=False)
    saved, mode = fused.choices(), winograd.get_mode()
    fused.set_choices({}, replace=True)
    winograd.reset_flop_counter()
    yield r
    fused.set_choices(saved, replace=True)
    winograd.set_mode(mode)
    if r.log:
        print('\n' + '\n'.join(r.log))


def _family(dtype, trace):
    if dtype == torch.bfloat16:
        return 'bfloat16'
    return 'winograd' if any(t in ('wino2', 'wino4') for t in trace) else 'float32'


def _bars(trace, gemm_k):
    """Sum of the single-kernel bars on a float32 route whose every compute launch has one (``gemm_k``: the K of its GEMM
    launches in order)."""
    ks = iter(gemm_k)
    total = 0.0
    for t in trace:
        if t in ('gemm', 'gemm3', 'pair', 'conv3x3_x3', 'stem_x3'):
            total += 2e-6 * math.sqrt(next(ks))
        elif t in ('wino2', 'wino4'):
            total += 2e-5
        elif t.startswith('miopen:') or t == 'dwconv':
            return float('inf')                                    # (a step without a bar of its own: K * e0 alone)
    return total


def _same(a, b, rec, trace, what):
    """Bit for bit -- or, with a convolution of MIOpen's on the route, at ``e0`` (see ``rec``): the two differ by
    no more than the family's ``K * e0``, max and rms (with K = 2 that is the sum of two errors of ``e0`` each; ``1 * e0`` is below
    one float32 ulp of the head's largest outputs, the smallest difference two calls can have there)."""
    if torch.equal(a, b):
        return
    e0, scale, dtype = rec.case
    d = a.double() - b.double()
    delta = (d.abs().max().item() / scale, d.pow(2).mean().sqrt().item() / scale)
    assert any(t.startswith('miopen:') for t in trace), '%s: max |delta| %.3g of max |ref|' % (what, delta[0])
    k = K[_family(dtype, trace)]
    rec.log.append('NOREPEAT %s %s | %s | delta max %.3e rms %.3e | delta/e0 max %.2f rms %.2f' % (
        what, str(dtype).replace('torch.', ''), ' '.join(trace), delta[0], delta[1], delta[0] / e0[0], delta[1] / e0[1]))
    assert delta[0] <= k * e0[0] and delta[1] <= k * e0[1], '%s: delta %s, e0 %s' % (what, delta, e0)


def _forward_checks(opt, x, rec):
    """Assertions 2 and 3 -> (output of the first call, launch trace of the second)."""
    x0 = x.clone()
    with torch.no_grad():
        first = opt(x)
        rec.trace.clear()
        second = opt(x)
        trace = list(rec.trace)
        assert torch.equal(x, x0), 'the forward wrote into its input'
        third = opt(x0.clone(memory_format=torch.preserve_format))
    assert first.isfinite().all()
    _same(first, second, rec, trace, 'first call != second call')
    _same(first, third, rec, trace, 'a fresh clone of the input gives other bits')
    return first, trace


class _Judge:
    """Collects (e0, err) of every seed of one route, prints them, then asserts bound 1 for all of them."""

    def __init__(self, rec, module, dtype, decided):
        self.rec, self.dtype, self.rows = rec, dtype, []
        self.head = '%s %s %s' % (module, str(dtype).replace('torch.', ''), decided)

    def add(self, seed, trace, got, ref64, e0, gemm_k=()):
        err = tc.errors(got, ref64)
        family = _family(self.dtype, trace)
        bound = [K[family] * e0[0], K[family] * e0[1]]
        if self.dtype == torch.float32 and gemm_k is not None:
            bound[0] = min(bound[0], _bars(trace, gemm_k))
        self.rows.append((seed, err, bound))
        self.rec.log.append('ROUTE %s | %s | seed %d | e0 max %.3e rms %.3e | err max %.3e rms %.3e | err/e0 max %.2f rms %.2f | %s k=%d'
                            % (self.head, ' '.join(trace), seed, e0[0], e0[1], err[0], err[1], err[0] / e0[0], err[1] / e0[1],
                               family, K[family]))

    def verdict(self):
        assert len(self.rows) >= 3
        bad = [(seed, err, bound) for seed, err, bound in self.rows if err[0] > bound[0] or err[1] > bound[1]]
        assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------ modules
def _median_error(plain, x, ref64, calls=9):
    """``e0``: MIOpen does not repeat (see ``rec``), and the LARGEST error of a float32 bottleneck moved between 0.7 and
    1.3 of its median over 30 calls -- so ``e0`` is the median (max and rms each) of nine calls of the unfused module."""
    errs = [tc.errors(plain(x), ref64) for _ in range(calls)]
    return tuple(sorted(e[i] for e in errs)[calls // 2] for i in (0, 1))


@functools.lru_cache(maxsize=None)
def _reference(make, shape, dtype, seed, relu_input=True):
    """-> (the unfused module on the CPU, x, ref64, e0).  ``make(seed)`` builds the unfused module."""
    module = make(seed)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(1000 + seed))
    if relu_input:
        x = x.relu()
    x = x.cuda().to(dtype).contiguous(memory_format=CL)
    with torch.no_grad():
        ref64 = copy.deepcopy(module).double().cuda()(x.double())
        plain = copy.deepcopy(module).cuda().to(dtype).to(memory_format=CL)
        e0 = _median_error(plain, x, ref64)
    assert e0[0] > 0 and ref64.isfinite().all()
    return module, x, ref64, e0


def _case(rec, *args):
    module, x, ref64, e0 = _reference(*args)
    rec.case = (e0, ref64.abs().max().item(), x.dtype)
    return module, x, ref64, e0


def _optimized(module, dtype, rec):
    return rec.watch(tc.optimized(module).cuda().to(dtype).to(memory_format=CL))


class _BSpec:
    """One bottleneck shape: the keys of its decisions and the launch trace of a route."""

    def __init__(self, name, inplanes, planes, stride, downsample, hw, batch=3):
        self.name, self.inplanes, self.planes, self.stride, self.downsample = name, inplanes, planes, stride, downsample
        self.shape = (batch, inplanes) + tuple(hw)
        self.m_in = batch * hw[0] * hw[1]
        self.m_out = batch * ((hw[0] - 1) // stride + 1) * ((hw[1] - 1) // stride + 1)
        self.make = functools.partial(tc.bottleneck, inplanes, planes, stride, downsample)

    def keys(self, dtype, deferred):
        dt, p = str(dtype), self.planes
        return {'conv1': (dt, self.m_in, self.inplanes, p, False, False),
                'conv3': ('torch.float32/conv3', self.m_out, 9 * p, p, self.stride > 1, False),
                'pair': ('torch.float32/pair', self.m_out, p + self.inplanes, 4 * p, self.stride > 1, deferred),
                'tail': (dt, self.m_out, p, 4 * p, True, deferred)}

    def force(self, dtype, conv1, conv2, tail):
        """Sets every switch and the whole table for one route -> the table."""
        winograd.set_mode('winograd' if conv2 in ('wino4', 'wino2') else 'conv')
        winograd.X3 = conv2 != 'wino2'
        fused.X3_CONV3 = conv2.startswith('conv3:')
        keys = self.keys(dtype, conv2 == 'raw')
        table = {keys['conv1']: conv1, keys['conv3']: 'x3' if conv2 == 'conv3:x3' else 'conv',
                 keys['pair']: 'x3' if tail == 'pair' else 'conv'}
        if tail != 'pair':
            table[keys['tail']] = tail
        fused.set_choices(table, replace=True)
        return table

    def trace(self, conv1, conv2, tail):
        t = {'gemm': ['gemm'], 'gemm3': ['gemm3'], 'conv': ['miopen:conv1', 'bias_act']}[conv1]
        t += {'wino4': ['wino4'], 'wino2': ['wino2'], 'conv3:x3': ['conv3x3_x3'], 'conv3:conv': ['miopen:conv2', 'bias_act'],
              'raw': ['miopen:conv2']}[conv2]
        if tail == 'pair':
            return t + ['pair']
        if self.downsample:
            t += ['miopen:downsample.0']
        deferred = ['bias_act'] if conv2 == 'raw' else []
        return t + {'gemm': ['gemm'], 'gemm3': ['gemm3'], 'pass+gemm': ['bias_act', 'gemm'],
                    'conv': deferred + ['miopen:conv3', 'bias_act']}[tail]

    def gemm_k(self, conv1, conv2, tail):
        """K of the route's float32 GEMM launches, in launch order (for their single-kernel bars)."""
        return ([self.inplanes] if conv1 != 'conv' else []) + ([9 * self.planes] if conv2 == 'conv3:x3' else []) + \
            [self.planes + self.inplanes if tail == 'pair' else self.planes]

    def routes_from_choices(self, dtype, deferred, conv3_on):
        """What the product decided by itself (timing, capture): read back from ``fused.choices()``."""
        table, keys = fused.choices(), self.keys(dtype, deferred)
        conv2 = 'raw' if deferred else ('conv3:' + table[keys['conv3']] if conv3_on else None)
        tail = 'pair' if table.get(keys['pair']) == 'x3' else table[keys['tail']]
        return table[keys['conv1']], conv2, tail


BLOCKS = {'a': _BSpec('bottleneck-a', 256, 64, 1, False, (13, 11)), 'b': _BSpec('bottleneck-b', 128, 64, 1, True, (13, 11)),
          'c': _BSpec('bottleneck-c', 256, 64, 2, True, (15, 11))}
assert (15 - 1) // 2 + 1 != 15 // 2


def _matrix():
    cases = []
    for b, spec in BLOCKS.items():
        conv2s = (('wino4', 'wino2') if spec.stride == 1 else ()) + ('conv3:x3', 'conv3:conv', 'raw')
        for conv2 in conv2s:
            tails = (('pair',) if spec.downsample else ()) + ('gemm', 'gemm3', 'conv') + (('pass+gemm',) if conv2 == 'raw' else ())
            for tail in tails:
                cases.append((b, conv2, tail))
    return cases


def _run_bottleneck_route(rec, spec, dtype, conv1, conv2, tail, decided='forced'):
    judge = _Judge(rec, spec.name, dtype, decided)
    for seed in SEEDS:
        module, x, ref64, e0 = _case(rec, spec.make, spec.shape, dtype, seed)
        opt = _optimized(module, dtype, rec)
        table = spec.force(dtype, conv1, conv2, tail)
        flops = winograd.direct_flops()
        got, trace = _forward_checks(opt, x, rec)
        assert trace == spec.trace(conv1, conv2, tail), (trace, spec.trace(conv1, conv2, tail))
        assert (winograd.direct_flops() > flops) == (conv2 in ('wino4', 'wino2'))
        assert fused.choices() == table and rec.timed == 0        # nothing was decided behind the table's back
        judge.add(seed, trace, got, ref64, e0, spec.gemm_k(conv1, conv2, tail))
    judge.verdict()


@pytest.mark.parametrize('block,conv2,tail', _matrix(), ids=lambda v: v)
def test_bottleneck_float32_matrix(rec, block, conv2, tail):
    """conv2 route x tail route, the full product of what each block can reach; conv1's three choices rotate through it."""
    index = _matrix().index((block, conv2, tail))
    _run_bottleneck_route(rec, BLOCKS[block], torch.float32, ('gemm', 'gemm3', 'conv')[index % 3], conv2, tail)


@pytest.mark.parametrize('conv1', ['gemm', 'gemm3', 'conv'])
@pytest.mark.parametrize('block', list(BLOCKS))
def test_bottleneck_conv1_routes(rec, block, conv1):
    spec = BLOCKS[block]
    _run_bottleneck_route(rec, spec, torch.float32, conv1, 'wino4' if spec.stride == 1 else 'conv3:x3', 'pair' if spec.downsample else 'gemm3')


@pytest.mark.parametrize('tail', ['gemm', 'pass+gemm', 'conv'])
@pytest.mark.parametrize('conv1', ['gemm', 'conv'])
@pytest.mark.parametrize('block', list(BLOCKS))
def test_bottleneck_bfloat16(rec, block, conv1, tail):
    """bfloat16: conv2 is MIOpen's raw output and its bias + ReLU are always left to the tail; no split-operand kernel may run."""
    _run_bottleneck_route(rec, BLOCKS[block], torch.bfloat16, conv1, 'raw', tail)


def test_nine_terms_and_the_pair_switch(rec):
    """``X3_TERMS = 9`` on every split-operand kernel of a block, and ``X3_PAIR`` off: the pair product is declined by
    ``pair_supported`` (two launches, no 'pair' entry asked for or made)."""
    spec = BLOCKS['b']
    fused.X3_TERMS = 9
    _run_bottleneck_route(rec, spec, torch.float32, 'gemm3', 'conv3:x3', 'pair', 'forced-terms9')
    _run_bottleneck_route(rec, spec, torch.float32, 'gemm3', 'wino4', 'gemm3', 'forced-terms9')
    fused.X3_TERMS = 6
    fused.X3_PAIR = False
    judge = _Judge(rec, spec.name, torch.float32, 'forced-pair-off')
    for seed in SEEDS:
        module, x, ref64, e0 = _case(rec, spec.make, spec.shape, torch.float32, seed)
        opt = _optimized(module, torch.float32, rec)
        table = spec.force(torch.float32, 'gemm', 'raw', 'gemm3')
        del table[spec.keys(torch.float32, True)['pair']]
        fused.set_choices(table, replace=True)
        got, trace = _forward_checks(opt, x, rec)
        assert trace == spec.trace('gemm', 'raw', 'gemm3') and fused.choices() == table and rec.timed == 0
        judge.add(seed, trace, got, ref64, e0, spec.gemm_k('gemm', 'raw', 'gemm3'))
    judge.verdict()


NARROW = {'n32': (_BSpec('bottleneck-n32', 96, 32, 2, True, (15, 11)),
                  # conv1: N = 32 is no multiple of 64 -> MIOpen; conv2: 32 channels -> raw; tail: the pair product takes K1 = 32
                  {torch.float32: ['miopen:conv1', 'bias_act', 'miopen:conv2', 'pair'],
                   torch.bfloat16: ['miopen:conv1', 'bias_act', 'miopen:conv2', 'miopen:downsample.0', 'bias_act', 'miopen:conv3', 'bias_act']}),
          'n48': (_BSpec('bottleneck-n48', 192, 48, 1, False, (13, 11)),
                  # K = 48 is no multiple of 32 (64 for bfloat16): every GEMM is declined, the deferred bias is applied by its own pass
                  {dt: ['miopen:conv1', 'bias_act', 'miopen:conv2', 'bias_act', 'miopen:conv3', 'bias_act']
                   for dt in (torch.float32, torch.bfloat16)})}


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['float32', 'bfloat16'])
@pytest.mark.parametrize('width', list(NARROW))
def test_widths_the_kernels_must_decline(rec, width, dtype):
    """Widths that are no multiple of 64, Winograd FORCED on: the ``*_supported`` predicates decline (nothing is mis-run), the
    only table entry that may appear is the pair product's (forced here: planes 32 + inplanes 96 is a multiple of 64)."""
    spec, traces = NARROW[width]
    judge = _Judge(rec, spec.name, dtype, 'forced')
    for seed in SEEDS:
        module, x, ref64, e0 = _case(rec, spec.make, spec.shape, dtype, seed)
        opt = _optimized(module, dtype, rec)
        winograd.set_mode('winograd')
        fused.FORCE_PICK = 'x3'
        got, trace = _forward_checks(opt, x, rec)
        assert trace == traces[dtype], trace
        assert fused.choices() == {} and winograd.direct_flops() == 0 and rec.timed == 0
        judge.add(seed, trace, got, ref64, e0, [spec.planes + spec.inplanes])
    judge.verdict()


# ------------------------------------------------------------------------------------------------- timed and captured blocks
def _set_conv2(spec, how):
    """'deferred': conv2 raw (MIOpen, bias left to the tail); 'auto': whatever the block does by default at this size."""
    winograd.set_mode('conv' if how == 'deferred' else 'winograd')
    fused.X3_CONV3 = how != 'deferred'


@pytest.mark.parametrize('block,how', [('c', 'deferred'), ('c', 'auto'), ('b', 'auto')], ids=['c-deferred', 'c-auto', 'b-auto'])
def test_timed_first_call(rec, block, how):
    """Empty table, nothing forced: the product's own first-call timing decides.  The first call must compute what every later
    call computes (timing runs each candidate seven times; the two-launch tail writes its operand in place)."""
    spec = BLOCKS[block]
    judge = _Judge(rec, spec.name, torch.float32, 'timed-' + how)
    for seed in SEEDS:
        module, x, ref64, e0 = _case(rec, spec.make, spec.shape, torch.float32, seed)
        opt = _optimized(module, torch.float32, rec)
        _set_conv2(spec, how)
        fused.set_choices({}, replace=True)
        rec.timed = 0
        got, trace = _forward_checks(opt, x, rec)
        assert rec.timed >= 4                                      # conv1's candidates and both sides of the pair, at least
        deferred = how == 'deferred'
        keys = spec.keys(torch.float32, deferred)
        assert keys['pair'] in fused.choices() and keys['conv1'] in fused.choices()
        if fused.choices()[keys['pair']] == 'x3':                  # (the inner choice is made while the other side is timed)
            assert keys['tail'] in fused.choices()
        conv1, conv2, tail = spec.routes_from_choices(torch.float32, deferred, spec.stride > 1)
        conv2 = conv2 or 'wino4'
        assert trace == spec.trace(conv1, conv2, tail), (trace, fused.choices())
        judge.add(seed, trace, got, ref64, e0, spec.gemm_k(conv1, conv2, tail))
    judge.verdict()


@pytest.mark.parametrize('inner', ['pass+gemm', 'conv', 'gemm', 'gemm3'])
def test_timed_pair_with_the_inner_choice_pinned(rec, inner):
    """The timed ``pick('pair')`` with deferred ``a_bias`` while the two-launch side's own choice is pinned: ``pass+gemm`` and
    ``conv`` apply ``relu(out + fb2)`` IN PLACE on the block's ``out`` -- seven times during the timing unless ``pick`` puts the
    operand back.  Whoever wins, the first call equals the second and the float64 block."""
    spec = BLOCKS['c']
    judge = _Judge(rec, spec.name, torch.float32, 'timed-pair/inner=' + inner)
    for seed in SEEDS:
        module, x, ref64, e0 = _case(rec, spec.make, spec.shape, torch.float32, seed)
        opt = _optimized(module, torch.float32, rec)
        _set_conv2(spec, 'deferred')
        keys = spec.keys(torch.float32, True)
        fused.set_choices({keys['conv1']: 'gemm', keys['tail']: inner}, replace=True)
        rec.timed = 0
        got, trace = _forward_checks(opt, x, rec)
        assert rec.timed == 2 and fused.choices()[keys['tail']] == inner
        tail = 'pair' if fused.choices()[keys['pair']] == 'x3' else inner
        assert trace == spec.trace('gemm', 'raw', tail), trace
        judge.add(seed, trace, got, ref64, e0, spec.gemm_k('gemm', 'raw', tail))
        # ... and the side that lost the clock, from the same state: the timing left nothing behind for it either
        table = fused.choices()
        table[keys['pair']] = 'conv' if tail == 'pair' else 'x3'
        fused.set_choices(table, replace=True)
        other, trace = _forward_checks(opt, x, rec)
        judge.add(seed, trace, other, ref64, e0, spec.gemm_k('gemm', 'raw', 'pair' if tail != 'pair' else inner))
    judge.verdict()


def _capture_first_call(opt, x):
    """The FIRST call of ``opt`` on this shape inside a stream capture, replayed -> (replayed output, the graph, its output)."""
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        with torch.no_grad():
            y = opt(x)
    graph.replay()
    torch.cuda.synchronize()
    return y.clone(), graph, y


def _captured_checks(opt, x, rec):
    x0 = x.clone()
    rec.trace.clear()
    got, graph, y = _capture_first_call(opt, x)
    trace = list(rec.trace)
    with torch.no_grad():
        eager = opt(x)                                             # the choices the capture made are remembered
    torch.cuda.synchronize()
    _same(got, eager, rec, trace, 'replay != eager run with the remembered choices')
    graph.replay()
    torch.cuda.synchronize()
    _same(y, got, rec, trace, 'second replay != first replay')
    assert torch.equal(x, x0)
    assert got.isfinite().all()
    return got, trace


CAPTURED_BLOCKS = {'small': (BLOCKS['c'], 'conv'), 'large': (_BSpec('bottleneck-c-large', 128, 64, 2, True, (149, 151)), 'x3')}


@pytest.mark.parametrize('size', list(CAPTURED_BLOCKS))
def test_first_call_under_capture(rec, size):
    """No timing inside a capture: ``conv_bias_act`` takes 'gemm', ``pick`` decides by size (x3 from 16384 output pixels), both
    remembered.  Strided block with downsample, conv2 raw, bias deferred; the large one is over the size rule's line."""
    spec, side = CAPTURED_BLOCKS[size]
    assert (spec.m_out >= 16384) == (side == 'x3')
    judge = _Judge(rec, spec.name, torch.float32, 'captured')
    for seed in SEEDS:
        module, x, ref64, e0 = _case(rec, spec.make, spec.shape, torch.float32, seed)
        opt = _optimized(module, torch.float32, rec)
        _set_conv2(spec, 'deferred')
        fused.set_choices({}, replace=True)
        got, trace = _captured_checks(opt, x, rec)
        keys = spec.keys(torch.float32, True)
        want = {keys['conv1']: 'gemm', keys['pair']: side}
        if side == 'conv':
            want[keys['tail']] = 'gemm'
        assert fused.choices() == want and rec.timed == 0, fused.choices()
        assert trace == spec.trace('gemm', 'raw', 'pair' if side == 'x3' else 'gemm'), trace
        judge.add(seed, trace, got, ref64, e0, spec.gemm_k('gemm', 'raw', 'pair' if side == 'x3' else 'gemm'))
    judge.verdict()


# ------------------------------------------------------------------------------------------------------------ other modules
BASIC = {'identity': (functools.partial(tc.basic_block, 64, 64, 1, False), (3, 64, 13, 11)),
         'downsample': (functools.partial(tc.basic_block, 64, 128, 2, True), (3, 64, 15, 11))}


@pytest.mark.parametrize('conv', ['wino4', 'wino2', 'miopen'])
@pytest.mark.parametrize('block', list(BASIC))
def test_basic_block(rec, block, conv):
    make, shape = BASIC[block]
    strided = block == 'downsample'
    first = ['miopen:conv1', 'bias_act'] if conv == 'miopen' or strided else [conv]
    want = (['miopen:downsample.0'] if strided else []) + first + (['miopen:conv2'] if conv == 'miopen' else [conv]) + ['bias_act']
    judge = _Judge(rec, 'basicblock-' + block, torch.float32, 'forced')
    for seed in SEEDS:
        module, x, ref64, e0 = _case(rec, make, shape, torch.float32, seed)
        opt = _optimized(module, torch.float32, rec)
        winograd.set_mode('conv' if conv == 'miopen' else 'winograd')
        winograd.X3 = conv != 'wino2'
        got, trace = _forward_checks(opt, x, rec)
        assert trace == want, trace
        judge.add(seed, trace, got, ref64, e0)
    judge.verdict()


def _unit(first, seed):
    return tc.randomize_(network._InvertedResidualK(32, 64, True, stride=2, kernel_size=5) if first
                         else network._InvertedResidualK(64, 64, False, stride=1, kernel_size=5), seed)


UNITS = {'first-stride2': functools.partial(_unit, True), 'split-stride1': functools.partial(_unit, False)}


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['float32', 'bfloat16'])
@pytest.mark.parametrize('unit', list(UNITS))
def test_inverted_residual(rec, unit, dtype):
    first = unit == 'first-stride2'
    want = (['dwconv', 'miopen:branch1.2'] if first else []) + ['miopen:branch2.0', 'dwconv', 'miopen:branch2.5', 'interleave']
    judge = _Judge(rec, 'invertedresidual-' + unit, dtype, 'only')
    for seed in SEEDS:
        module, x, ref64, e0 = _case(rec, UNITS[unit], (3, 32 if first else 64, 15, 11), dtype, seed)
        opt = _optimized(module, dtype, rec)
        got, trace = _forward_checks(opt, x, rec)
        assert trace == want, trace
        judge.add(seed, trace, got, ref64, e0)
    judge.verdict()


def _decide(rec, how, key_of, small):
    """Applies one way of deciding a ``pick`` -> (runner, the side it must take or None where the clock decides)."""
    if how.startswith('forced:'):
        fused.set_choices({key_of: how[7:]}, replace=True)
        return _forward_checks, how[7:]
    if how == 'terms9':
        fused.X3_TERMS = 9
        fused.FORCE_PICK = 'x3'
        return _forward_checks, 'x3'
    if how == 'captured':
        return _captured_checks, 'conv' if small else 'x3'
    return _forward_checks, None                                   # 'timed', 'off'


def _stem(seed):
    net = network.Resnet('resnet18')
    net.block2 = net.block3 = net.block4 = net.block5 = nn.Identity()
    return tc.randomize_(net, seed)


STEM_SIZES = {'97x65': (3, 3, 97, 65), '161x163': (3, 3, 161, 163)}


@pytest.mark.parametrize('size', list(STEM_SIZES))
@pytest.mark.parametrize('how', ['forced:x3', 'forced:conv', 'terms9', 'off', 'timed', 'captured'])
def test_stem(rec, how, size):
    shape = STEM_SIZES[size]
    m = shape[0] * ((shape[2] - 1) // 2 + 1) * ((shape[3] - 1) // 2 + 1)
    key = ('torch.float32/stem', m, 256, 64, True, False)
    assert (m < 16384) == (size == '97x65')
    judge = _Judge(rec, 'stem-' + size, torch.float32, how)
    for seed in SEEDS:
        module, x, ref64, e0 = _case(rec, _stem, shape, torch.float32, seed, False)
        opt = _optimized(module, torch.float32, rec)
        fused.set_choices({}, replace=True)
        rec.timed = 0
        fused.X3_STEM = how != 'off'
        run, side = _decide(rec, how, key, m < 16384)
        got, trace = run(opt, x, rec)
        if how == 'off':
            side, want = 'conv', {}
        elif how == 'terms9':
            want = {}
        else:
            assert key in fused.choices()
            side = side or fused.choices()[key]
            want = {key: side}
        assert fused.choices() == want and rec.timed == (2 if how == 'timed' else 0), fused.choices()
        assert trace == (['stem_x3'] if side == 'x3' else ['miopen:input_block.0', 'bias_act']), trace
        judge.add(seed, trace, got, ref64, e0, [147])
    judge.verdict()


def _head_ref64(head, x):
    """``CompositeField4.forward`` (inference) restated in float64."""
    m, us = head.meta, head.meta.upsample_stride
    y = nn.functional.conv2d(x.double(), head.conv.weight.double(), head.conv.bias.double())
    if us > 1:
        y = nn.functional.pixel_shuffle(y, us)
        low, high = (us - 1) // 2, math.ceil((us - 1) / 2.0)
        y = y[:, :, low:y.shape[2] - high, low:y.shape[3] - high]
    B, _, H, W = y.shape
    y = y.reshape(B, m.n_fields, head.n_components, H, W).clone()
    nc = m.n_confidences
    y[:, :, 1:1 + nc] = y[:, :, 1:1 + nc].sigmoid()
    ii = torch.arange(W, device=y.device, dtype=y.dtype)
    jj = torch.arange(H, device=y.device, dtype=y.dtype).unsqueeze(1)
    for i, do_offset in enumerate(m.vector_offsets):
        if do_offset:
            y[:, :, 1 + nc + 2 * i] += ii
            y[:, :, 1 + nc + 2 * i + 1] += jj
    s0 = 1 + nc + m.n_vectors * 2
    y[:, :, s0:s0 + m.n_scales] = nn.functional.softplus(y[:, :, s0:s0 + m.n_scales])
    return y


@functools.lru_cache(maxsize=None)
def _head_reference(which, hw, seed):
    meta = headmeta.cocokp_metas()[0 if which == 'cif' else 1]
    head = tc.randomize_(network.CompositeField4(meta, 256), seed)
    x = torch.randn((3, 256) + hw, generator=torch.Generator().manual_seed(2000 + seed)).relu().cuda().contiguous(memory_format=CL)
    with torch.no_grad():
        ref64 = _head_ref64(copy.deepcopy(head).cuda(), x)
        plain = copy.deepcopy(head).cuda().to(memory_format=CL)
        plain.fused_epilogue = False
        old, fused.X3_HEAD = fused.X3_HEAD, False
        try:
            e0 = _median_error(plain, x, ref64)
        finally:
            fused.X3_HEAD = old
    assert e0[0] > 0 and ref64.isfinite().all()
    return head, x, ref64, e0


@pytest.mark.parametrize('which', ['cif', 'caf'])
@pytest.mark.parametrize('how', ['forced:x3', 'forced:conv', 'terms9', 'off', 'timed', 'captured', 'captured-large'])
def test_head(rec, how, which):
    """``CompositeField4`` with ``fused_epilogue`` on: 340 (CIF) / 684 (CAF) output channels, no multiple of 64."""
    hw = (75, 77) if how == 'captured-large' else (21, 19)
    m = 3 * hw[0] * hw[1]
    judge = _Judge(rec, 'head-' + which, torch.float32, how)
    for seed in SEEDS:
        head, x, ref64, e0 = _head_reference(which, hw, seed)
        rec.case = (e0, ref64.abs().max().item(), torch.float32)
        assert head.conv.out_channels % 64 != 0 and head.fused_epilogue
        key = ('torch.float32/head', m, 256, head.conv.out_channels, False, False)
        opt = rec.watch(copy.deepcopy(head).cuda().to(memory_format=CL))
        fused.set_choices({}, replace=True)
        rec.timed = 0
        fused.X3_HEAD = how != 'off'
        run, side = _decide(rec, how.replace('-large', ''), key, m < 16384)
        got, trace = run(opt, x, rec)
        if how == 'off':
            side, want = 'conv', {}
        elif how == 'terms9':
            want = {}
        else:
            assert key in fused.choices()
            side = side or fused.choices()[key]
            want = {key: side}
        assert fused.choices() == want and rec.timed == (2 if how == 'timed' else 0), fused.choices()
        assert trace == (['head_x3', 'gemm3'] if side == 'x3' else ['miopen:conv']) + ['head_epilogue'], trace
        judge.add(seed, trace, got, ref64, e0, None)
    judge.verdict()


# ------------------------------------------------------------------------------------------ operands after a parameter event
def _event(opt, other, name):
    with torch.no_grad():
        if name == 'load_state_dict':
            opt.load_state_dict(other.state_dict(), strict=True)
        elif name == 'in_place':
            for p in opt.parameters():
                p.mul_(1.25)
        elif name == 'bfloat16_round_trip':
            opt.to(torch.bfloat16).float()
        else:
            conv = opt.conv
            new = nn.Parameter(other.conv.bias.detach().clone())
            while new._version < conv.bias._version:
                new.add_(0.0)
            conv.bias = new


EVENT_MODULES = {'bottleneck': (lambda seed: tc.bottleneck(256, 64, 1, False, seed), (3, 256, 13, 11)),
                 'bottleneck-pair': (lambda seed: tc.bottleneck(128, 64, 2, True, seed), (3, 128, 15, 11)),
                 'basicblock': (lambda seed: tc.basic_block(64, 64, 1, False, seed), (3, 64, 13, 11)),
                 'invertedresidual': (lambda seed: _unit(True, seed), (3, 32, 15, 11)),
                 'stem': (_stem, (3, 3, 97, 65)),
                 'head': (lambda seed: tc.randomize_(network.CompositeField4(headmeta.cocokp_metas()[0], 256), seed), (3, 256, 21, 19))}


@pytest.mark.parametrize('module,event', [(m, e) for m in EVENT_MODULES for e in ('load_state_dict', 'in_place', 'bfloat16_round_trip')]
                         + [('head', 'bias_replaced')])     # (only the head's convolution has a bias Parameter)
def test_forward_after_a_parameter_event(rec, monkeypatch, module, event):
    """A forward (which fills every operand cache), the event, a forward: bit for bit the output of a freshly optimized module
    that holds the same parameters, on the kernels' routes, with ``winograd.X3`` on and off -- and within 1e-4 (the bar the
    trunk tests hold Winograd against MIOpen to) of the same module on MIOpen's routes, which derive nothing."""
    monkeypatch.setenv('OPA_CONV1X1', 'gemm')                      # (the 1x1 convolutions on the kernel: no MIOpen step that does not repeat)
    make, shape = EVENT_MODULES[module]
    x = torch.randn(shape, generator=torch.Generator().manual_seed(5)).relu().cuda().contiguous(memory_format=CL)
    fresh_of = (lambda m: copy.deepcopy(m)) if module == 'head' else tc.optimized
    for x3 in (True, False):
        winograd.set_mode('winograd')
        winograd.X3 = x3
        fused.FORCE_PICK = 'x3'
        fused.set_choices({}, replace=True)
        opt = fresh_of(make(0)).cuda().to(memory_format=CL)
        other = fresh_of(make(1)).cuda().to(memory_format=CL)
        with torch.no_grad():
            before = opt(x)
            _event(opt, other, event)
            after = opt(x)
            fresh = fresh_of(make(0)).cuda().to(memory_format=CL)
            fresh.load_state_dict(opt.state_dict(), strict=True)
            for name, p in opt.named_parameters():                 # (a replaced Parameter: the state dict carries its values)
                assert torch.equal(p, fresh.get_parameter(name))
            want = fresh(x)
            assert not torch.equal(before, after)
            stale = (after - want).abs().max().item()
            # (the unit's 1x1 convolutions are MIOpen's: should one of them not repeat, float32 rounding level; a stale w_taps is order one)
            assert torch.equal(after, want) or (module == 'invertedresidual' and stale <= 1e-5 * want.abs().max().item()), \
                '%s: stale operand, max |delta| %.3g of %.3g' % (module, stale, want.abs().max().item())
            winograd.set_mode('conv')
            fused.FORCE_PICK = 'conv'
            plain = fresh(x)
        assert not torch.equal(plain, want) or module == 'invertedresidual'          # (it did take other kernels)
        assert (plain - want).abs().max().item() <= 1e-4 * plain.abs().max().item()
