"""The host state around the kernels while a stream is being captured into a HIP graph, without a GPU: ``fused.derived`` (every
operand derived from a parameter), ``fused._gn_workspace`` (the GroupNorm workspace kept per stream) and the depthwise taps buffer of
``network._InvertedResidualK.taps_of``.  A graph bakes the ADDRESS of whatever a launch was handed, so

* nothing made inside a capture is kept (it lives in the graph's pool and holds nothing until the first replay), and a capturing
  call is not handed a kept tensor that an eager call may free (the workspace);
* a kept operand whose sources changed in place is overwritten in place -- same ``data_ptr()``, new values --, and replaced only
  where a source was replaced.

"Capturing" is ``torch.cuda.is_initialized`` and ``torch.cuda.is_current_stream_capturing`` answering True (``test_unit_gemm_host.py``
does the same to the decision); the tensors are the CPU's.  The same rules on real graphs: ``test_gpu_graph_replay.py``."""
import pytest
import torch
from torch import nn

from openpifpaf_amd import fused, network, winograd


@pytest.fixture
def capture(monkeypatch):
    """-> ``set(on)``: from then on the current stream is (not) being captured, as far as ``fused`` can tell."""
    state = {'on': False}
    monkeypatch.setattr(torch.cuda, 'is_initialized', lambda: True)
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: state['on'])

    def set_(on):
        state['on'] = bool(on)
    return set_


def _conv(k=24, n=40, bias=True, size=1, seed=0):
    torch.manual_seed(seed)
    return nn.Conv2d(k, n, size, padding=size // 2, bias=bias).requires_grad_(False)


class _Counted:
    """``make`` for ``derived``: twice the weight and the bias as it is (None without one), and how often it ran."""

    def __init__(self, conv):
        self.conv, self.calls = conv, 0

    def __call__(self):
        self.calls += 1
        c = self.conv
        return c.weight.detach() * 2.0, None if c.bias is None else c.bias.detach().clone()


# ---- derived: while capturing ----------------------------------------------------------------------------------------------------

def test_without_a_gpu_nothing_is_capturing():
    assert fused._capturing() is False                                 # (asking torch itself would raise on a machine without one)


def test_an_operand_made_while_capturing_is_not_kept(capture):
    conv = _conv()
    make = _Counted(conv)
    capture(True)
    first = fused.derived(conv, '_opa_t', (conv.weight, conv.bias), make)
    assert not hasattr(conv, '_opa_t') and make.calls == 1
    assert torch.equal(first[0], conv.weight * 2.0) and torch.equal(first[1], conv.bias)
    second = fused.derived(conv, '_opa_t', (conv.weight, conv.bias), make)           # (every capturing call makes its own)
    assert not hasattr(conv, '_opa_t') and make.calls == 2 and second[0] is not first[0]
    capture(False)
    eager = fused.derived(conv, '_opa_t', (conv.weight, conv.bias), make)            # an eager call makes and keeps its own
    assert make.calls == 3 and eager[0] is not first[0] and eager[0] is not second[0]
    assert conv._opa_t[1] is eager and fused.derived(conv, '_opa_t', (conv.weight, conv.bias), make) is eager and make.calls == 3


def test_a_current_entry_is_what_a_capturing_call_gets(capture):
    """The warm-up case: the graph bakes the kept operand's address, and rule (ii) keeps that address valid."""
    conv = _conv()
    make = _Counted(conv)
    eager = fused.derived(conv, '_opa_t', (conv.weight, conv.bias), make)
    capture(True)
    assert fused.derived(conv, '_opa_t', (conv.weight, conv.bias), make) is eager and make.calls == 1


def test_a_stale_entry_met_while_capturing_is_left_alone(capture):
    conv = _conv()
    make = _Counted(conv)
    eager = fused.derived(conv, '_opa_t', (conv.weight, conv.bias), make)
    entry, old = conv._opa_t, eager[0].clone()
    conv.weight.mul_(3.0)
    capture(True)
    got = fused.derived(conv, '_opa_t', (conv.weight, conv.bias), make)
    assert got[0] is not eager[0] and torch.equal(got[0], conv.weight * 2.0)         # the capturing call: the current weights, its own
    assert conv._opa_t is entry and torch.equal(eager[0], old)                       # nothing recorded into the kept tensors
    capture(False)
    after = fused.derived(conv, '_opa_t', (conv.weight, conv.bias), make)
    assert after[0] is eager[0] and torch.equal(eager[0], conv.weight * 2.0)         # the next eager call refreshes them in place


# ---- derived: after an in-place change, after a replaced source ----------------------------------------------------------------------

def test_an_in_place_change_refreshes_the_kept_tensors_in_place():
    conv = _conv()
    make = _Counted(conv)
    w2, b = fused.derived(conv, '_opa_t', (conv.weight, conv.bias), make)
    ptrs = (w2.data_ptr(), b.data_ptr())
    other = _conv(seed=1)
    conv.load_state_dict(other.state_dict())                           # copy_: the pointers stay, the versions rise
    got = fused.derived(conv, '_opa_t', (conv.weight, conv.bias), make)
    assert got[0] is w2 and got[1] is b and (w2.data_ptr(), b.data_ptr()) == ptrs
    assert torch.equal(w2, other.weight * 2.0) and torch.equal(b, other.bias) and make.calls == 2
    conv.weight.mul_(1.25)
    conv.bias.add_(1.0)
    got = fused.derived(conv, '_opa_t', (conv.weight, conv.bias), make)
    assert got[0] is w2 and (w2.data_ptr(), b.data_ptr()) == ptrs
    assert torch.equal(w2, other.weight * 1.25 * 2.0) and torch.equal(b, other.bias + 1.0) and make.calls == 3
    assert fused.derived(conv, '_opa_t', (conv.weight, conv.bias), make) is got and make.calls == 3


def test_a_replaced_source_replaces_the_entry():
    conv = _conv()
    make = _Counted(conv)
    w2, b = fused.derived(conv, '_opa_t', (conv.weight, conv.bias), make)
    old = w2.clone()
    conv.to(torch.float64)                                             # a new dtype (and new storage)
    got = fused.derived(conv, '_opa_t', (conv.weight, conv.bias), make)
    assert got[0] is not w2 and got[1] is not b and got[0].dtype == torch.float64
    assert torch.equal(w2, old)                                        # what a graph over the old parameters reads stays what it was
    w2, b = got
    new = nn.Parameter(torch.ones(40, dtype=torch.float64), requires_grad=False)
    with torch.no_grad():
        while new._version < conv.bias._version:                       # (the version alone would not tell)
            new.add_(0.0)
    conv.bias = new                                                    # a new pointer, same dtype and shape
    got = fused.derived(conv, '_opa_t', (conv.weight, conv.bias), make)
    assert got[0] is not w2 and got[1] is not b and torch.equal(got[1], torch.ones(40, dtype=torch.float64))
    w2 = got[0]
    conv.weight = nn.Parameter(conv.weight[:, :12].clone().contiguous(), requires_grad=False)          # another shape
    got = fused.derived(conv, '_opa_t', (conv.weight, conv.bias), make)
    assert got[0] is not w2 and tuple(got[0].shape) == (40, 12, 1, 1)


def test_a_tuple_with_none_is_handled():
    conv = _conv(bias=False)
    make = _Counted(conv)
    w2, b = fused.derived(conv, '_opa_t', (conv.weight, conv.bias), make)
    assert b is None
    conv.weight.mul_(0.5)
    got = fused.derived(conv, '_opa_t', (conv.weight, conv.bias), make)
    assert got[0] is w2 and got[1] is None and torch.equal(w2, conv.weight * 2.0) and make.calls == 2
    conv.bias = nn.Parameter(torch.ones(40), requires_grad=False)      # None -> a tensor: a source replaced
    got = fused.derived(conv, '_opa_t', (conv.weight, conv.bias), make)
    assert got[0] is not w2 and torch.equal(got[1], torch.ones(40))
    w2 = got[0]
    conv.bias = None                                                   # ... and back
    got = fused.derived(conv, '_opa_t', (conv.weight, conv.bias), make)
    assert got[0] is not w2 and got[1] is None


def test_an_operand_of_another_layout_replaces_the_entry():
    """``make`` decides the operand's shape; should it ever give another one for the same sources, nothing is written across."""
    conv = _conv()
    shapes = [(40, 24), (24, 40)]
    first = fused.derived(conv, '_opa_t', (conv.weight,), lambda: conv.weight.detach().reshape(shapes[0]).clone())
    conv.weight.mul_(2.0)
    second = fused.derived(conv, '_opa_t', (conv.weight,), lambda: conv.weight.detach().reshape(40, 24).t().contiguous())
    assert second is not first and tuple(second.shape) == shapes[1] and tuple(first.shape) == shapes[0]


# ---- derived: the operands of the routes ---------------------------------------------------------------------------------------------

def _pair():
    return _conv(16, 32, bias=False), _conv(8, 32, bias=False, seed=1), torch.arange(16.0)


OPERANDS = {
    'split weight': (lambda: _conv(64, 64, bias=False), lambda c: fused._split_weight_of(c, c.weight.view(64, 64))),
    'split 3x3': (lambda: _conv(16, 32, bias=False, size=3), fused._split_weight_3x3_of),
    'stem 7x7': (lambda: _conv(3, 64, bias=False, size=7), fused._stem_weight_of),
    'unit': (lambda: _conv(24, 40), fused._unit_weight_of),
    'unit bf16': (lambda: _conv(24, 40).to(torch.bfloat16), fused._unit_weight_bf16_of),
    'head16': (lambda: _conv(64, 40).to(torch.float16), fused.head16_operands_of),
    'grouped': (lambda: nn.Conv2d(64, 64, 3, padding=1, groups=4, bias=False).requires_grad_(False), fused.gconv_weight_of),
    'winograd': (lambda: _conv(16, 64, bias=False, size=3), winograd.filter_of),
    'winograd split': (lambda: _conv(16, 64, bias=False, size=3), winograd.split_filter_of),
    'stem 3x3': (lambda: _conv(3, 24, bias=False, size=3), fused.stem_weight_of),
}


def _flat(operand):
    return [t for t in (operand if isinstance(operand, (tuple, list)) else (operand,)) if t is not None]


@pytest.mark.parametrize('name', list(OPERANDS))
def test_the_routes_operands_obey_the_contract(capture, name):
    """Not kept while capturing; after an in-place change the same tensors with what a fresh module derives, bit for bit; new
    tensors after a cast."""
    build, of = OPERANDS[name]
    conv = build()
    capture(True)
    attrs = set(vars(conv))
    made = _flat(of(conv))
    assert set(vars(conv)) == attrs, set(vars(conv)) - attrs           # nothing left on the module
    capture(False)
    kept = _flat(of(conv))
    assert len(set(vars(conv)) - attrs) == 1
    assert all(k is not m and torch.equal(k, m) for k, m in zip(kept, made))
    ptrs = [t.data_ptr() for t in kept]
    with torch.no_grad():
        for p in conv.parameters():
            p.mul_(1.25)
    again = _flat(of(conv))
    assert all(a is k for a, k in zip(again, kept)) and [t.data_ptr() for t in again] == ptrs
    fresh = build()
    fresh.load_state_dict(conv.state_dict())
    assert all(torch.equal(a, f) for a, f in zip(again, _flat(of(fresh))))
    assert not all(torch.equal(a, m) for a, m in zip(again, made))     # (the change did change them)
    dtype = conv.weight.dtype
    conv.to(torch.float64).to(dtype)                                   # a round trip: new tensors with the same values
    replaced = _flat(of(conv))
    assert all(r is not k and torch.equal(r, k) for r, k in zip(replaced, kept))


def test_the_pair_operands_follow_both_convolutions_and_the_bias(capture):
    conv, dconv, a_bias = _pair()
    w3, ab = fused._pair_weight_of(conv, dconv, a_bias)
    ptrs = (w3.data_ptr(), ab.data_ptr())
    with torch.no_grad():
        dconv.weight.mul_(2.0)
        a_bias.add_(1.0)
    w3b, abb = fused._pair_weight_of(conv, dconv, a_bias)
    assert w3b is w3 and abb is ab and (w3.data_ptr(), ab.data_ptr()) == ptrs
    both = torch.cat((conv.weight.flatten(1), dconv.weight.flatten(1)), dim=1)
    assert torch.equal(w3, fused.split_weight(both)) and torch.equal(ab, torch.cat((a_bias, torch.zeros(8))))
    w3c, abc = fused._pair_weight_of(conv, dconv, None)               # the bias gone: a source replaced
    assert w3c is not w3 and abc is None
    capture(True)
    entry = conv._opa_w3_pair
    w3d, _ = fused._pair_weight_of(conv, dconv, a_bias)
    assert conv._opa_w3_pair is entry and w3d is not w3c and torch.equal(w3d, w3)


# ---- the depthwise taps: a buffer that is the kept operand ---------------------------------------------------------------------------

def _unit():
    torch.manual_seed(3)
    unit = network._InvertedResidualK(24, 48, True, stride=2).eval().requires_grad_(False)
    return network.optimize_for_inference_(unit)


def _depthwise(unit):
    convs = [m for m in unit.modules() if isinstance(m, nn.Conv2d) and hasattr(m, 'w_taps')]
    assert convs
    return convs


def test_the_taps_buffer_is_the_kept_operand_and_is_refreshed_in_place():
    unit = _unit()
    taps_of = network._InvertedResidualK.taps_of
    for conv in _depthwise(unit):
        taps = taps_of(conv)
        assert conv.w_taps is taps and torch.equal(taps, fused.depthwise_taps(conv.weight))
        assert any(v is taps for v in conv._buffers.values())          # still a buffer: part of the state dict
        ptr = taps.data_ptr()
        conv.weight.mul_(1.5)
        assert taps_of(conv) is taps and conv.w_taps is taps and taps.data_ptr() == ptr
        assert torch.equal(taps, fused.depthwise_taps(conv.weight))
        conv.to(torch.float64)
        new = taps_of(conv)
        assert new is not taps and conv.w_taps is new and new.dtype == torch.float64 and torch.equal(new, fused.depthwise_taps(conv.weight))


def test_the_taps_buffer_is_not_replaced_while_capturing(capture):
    unit = _unit()
    taps_of = network._InvertedResidualK.taps_of
    for conv in _depthwise(unit):
        buffer = conv.w_taps
        capture(True)
        first = taps_of(conv)                                          # the FIRST call, inside a capture
        assert conv.w_taps is buffer and first is not buffer and not hasattr(conv, '_opa_taps')
        assert torch.equal(first, fused.depthwise_taps(conv.weight))
        capture(False)
        kept = taps_of(conv)
        assert kept is not first and conv.w_taps is kept
        conv.weight.mul_(2.0)
        capture(True)
        stale = taps_of(conv)                                          # a stale entry met while capturing
        assert stale is not kept and conv.w_taps is kept and torch.equal(stale, fused.depthwise_taps(conv.weight))
        assert not torch.equal(kept, stale)
        capture(False)
        assert taps_of(conv) is kept and torch.equal(kept, stale)


# ---- the GroupNorm workspace ---------------------------------------------------------------------------------------------------------

@pytest.fixture
def workspaces(monkeypatch):
    monkeypatch.setattr(fused, '_GN_WORKSPACE', {})
    monkeypatch.setattr(fused, '_stream', lambda: 7)
    return fused._GN_WORKSPACE


def test_not_capturing_the_workspace_is_kept_and_grows(capture, workspaces):
    x = torch.zeros(1)
    ws = fused._gn_workspace(x, 1000)
    assert ws.dtype == torch.float64 and ws.numel() * 8 >= 1000 and list(workspaces.values()) == [ws] and list(workspaces) == [('cpu', 7)]
    assert fused._gn_workspace(x, 1000) is ws and fused._gn_workspace(x, 8) is ws        # a smaller call keeps it
    grown = fused._gn_workspace(x, 4096)
    assert grown is not ws and grown.numel() * 8 >= 4096 and list(workspaces.values()) == [grown]
    assert fused._gn_workspace(x, 1000) is grown


@pytest.mark.parametrize('cached', ['none', 'large enough', 'too small'])
def test_capturing_the_workspace_is_the_calls_own_and_nothing_is_stored(capture, workspaces, cached):
    x = torch.zeros(1)
    kept = None if cached == 'none' else fused._gn_workspace(x, 4096 if cached == 'large enough' else 64)
    before = dict(workspaces)
    capture(True)
    ws = fused._gn_workspace(x, 1000)
    again = fused._gn_workspace(x, 1000)
    assert ws is not kept and again is not kept and again is not ws and ws.dtype == torch.float64 and ws.numel() * 8 >= 1000
    if kept is not None:
        assert ws.data_ptr() != kept.data_ptr()
    assert workspaces == before and all(workspaces[k] is before[k] for k in before)      # the table as it was
    capture(False)
    if cached == 'large enough':
        assert fused._gn_workspace(x, 1000) is kept
