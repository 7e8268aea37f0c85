"""The 128 x 256 tile of the split-operand GEMM (csrc/gemm_f32x3.hip, ``gemm_f32x3_wide_kernel``) against the 128-wide tile it
stands in for, through the Python launchers.  ``OPA_X3_TILE`` -- read by ``launch_x3`` on every launch -- chooses the tile inside
one process: ``256`` takes the wide tile wherever it has an instantiation (not UNIT, six terms, N a multiple of 256) whatever the
size of the launch, ``128`` never.

* exact: integer operands against an int64 product, every RES / RELU / PRO leaf of the plain mode, the pair at stride 1 and 2, the
  3x3 taps at stride and dilation 1 and 2 -- after asserting that the variants' expectations differ;
* bit identity: on N(0, 1) data every such launch is ``torch.equal`` under both tiles (the wave tile, the MFMA order and the
  epilogue are the 128-wide tile's: every element sees the same additions in the same order);
* guards: the output as an interior view of a NaN-filled buffer -- rows past M and the surroundings keep their bits -- and one
  NaN and one Inf in A: their rows are NaN, every other element is the clean run's (the contract of csrc/split_bf16.hpp);
* dispatch: N = 128 and nine terms under ``OPA_X3_TILE=256`` still run, on the 128-wide tile.

M in {1, 128, 129, 257}: one row, one full tile, a tile and a one-row tile, two tiles and a one-row tile (rows of both M halves of
the workgroup and rows past M in every wave); N in {256, 512}: one and two N-tiles; K in {64, 128, 192}: the two peeled K-steps
alone, one and two passes of the loop in front of them."""
import functools
import itertools

import pytest

torch = pytest.importorskip('torch')

import x3_common as xc  # noqa: E402

gpu = pytest.mark.gpu
CL = torch.channels_last
MS, NS, KS = (1, 128, 129, 257), (256, 512), (64, 128, 192)
FLAGS = list(itertools.product((False, True), repeat=3))                    # (res, relu, pro)
PAIR_HW = (3, 43)                                                           # the pair's output pixels
TAPS_IN = (2, 64, 9, 15)                                                    # the taps' input: C = 64, M = 270 at stride 1, 80 at stride 2
NAN_BITS = 0x7fc0beef                                                       # a quiet NaN with a payload of its own
GUARD = 4096                                                                # floats on either side (16 KB: more than a tile's rows past M would need)


def _tile(monkeypatch, tile):
    monkeypatch.setenv('OPA_X3_TILE', str(tile))


def _product(a, w, bias, res=None, a_bias=None):
    a = a.long()
    if a_bias is not None:
        a = (a + a_bias.long()).clamp_min(0)
    out = a @ w.long().t() + bias.long()
    return out if res is None else out + res.long()


def _all_different(tensors, what):
    for (i, s), (j, t) in itertools.combinations(enumerate(tensors), 2):
        assert not torch.equal(s, t), '%s: variants %d and %d expect the same tensor' % (what, i, j)


def _expect(pre, relu):
    want = (pre.clamp_min(0) if relu else pre).double()
    assert torch.equal(want.float().double(), want), 'the expectation is not a float32 number'
    return want.float()


def _image(rows, b, h, w):
    return xc.image_of(rows, b, h, w).cuda().contiguous(memory_format=CL)


def _rows(out):
    torch.cuda.synchronize()
    assert out.is_contiguous(memory_format=CL)
    return xc.rows_of(out.cpu())


def _conv(w4d, stride=1, padding=0, dilation=1):
    n, c, k, _ = w4d.shape
    conv = torch.nn.Conv2d(c, n, k, stride, padding, dilation, bias=False).cuda().requires_grad_(False)
    conv.weight.copy_(w4d)
    return conv


# ---- the three modes: operands (integers or N(0, 1)) and one function that launches a variant -----------------------------------------------

@functools.lru_cache(maxsize=None)
def _plain_operands(m, n, k, kind):
    """-> (a, w, bias, res, a_bias) on the CPU: ``xc.integer_problem``'s budget (9-bit operands, 32 weights per row, below 2^24) or
    unit-scale normal numbers."""
    g = xc.gen(1000 * m + 10 * n + k + (kind == 'randn'))
    if kind == 'int':
        a, w = xc.integers((m, k), g, 9), xc.sparse_integer_weight(n, k, g)
        bias, res, a_bias = xc.integers((n,), g, 20), xc.integers((m, n), g, 20), xc.integers((k,), g, 8)
    else:
        a, w = torch.randn((m, k), generator=g), torch.randn((n, k), generator=g) * (2.0 / k) ** 0.5
        bias, res, a_bias = torch.randn((n,), generator=g), torch.randn((m, n), generator=g), torch.randn((k,), generator=g) * 0.3
    assert bool(res.any()) and bool(a_bias.any())
    return a, w, bias, res, a_bias


def _plain_runner(m, n, k, kind):
    """-> run(res, relu, pro) -> rows [M, N] on the CPU; the operands are uploaded once."""
    from openpifpaf_amd import fused
    a, w, bias, res, a_bias = _plain_operands(m, n, k, kind)
    x, r_d = _image(a, 1, 1, m), _image(res, 1, 1, m)
    w_d, bias_d, ab_d = w.cuda(), bias.cuda(), a_bias.cuda()
    w3 = fused.split_weight(w_d)
    assert fused.conv1x1_supported(x, w_d, bias_d, r_d, ab_d)

    def run(with_res, relu, pro):
        with torch.no_grad():
            return _rows(fused.conv1x1_bias_act_x3(x, w3, bias_d, r_d if with_res else None, relu, ab_d if pro else None, 6))
    return run


@functools.lru_cache(maxsize=None)
def _pair_operands(n, k, stride, kind, pro):
    spec = ('pair', k // 2, k // 2, n, stride)
    h_in = ((PAIR_HW[0] - 1) * stride + 1, (PAIR_HW[1] - 1) * stride + 1)
    g = xc.gen(77 + n + k + stride + 2 * pro + (kind == 'randn'))
    draw = (lambda s: xc.integers(s, g, 9)) if kind == 'int' else (lambda s: torch.randn(s, generator=g))
    x = draw((1, k // 2) + h_in)
    h = draw((1, k // 2) + PAIR_HW)
    if pro:                                                                 # (the second activation meets max(x + 0, 0))
        x = x.abs()
    if kind == 'int':
        w, bias, a_bias = xc.sparse_integer_weight(n, k, g), xc.integers((n,), g, 20), xc.integers((k // 2,), g, 8)
    else:
        w, bias, a_bias = torch.randn((n, k), generator=g) * (2.0 / k) ** 0.5, torch.randn((n,), generator=g), torch.randn((k // 2,), generator=g) * 0.3
    a = torch.cat((xc.rows_of(h), xc.rows_of(x[:, :, ::stride, ::stride])), dim=1)
    return spec, h, x, a, w, bias, (a_bias if pro else None)


def _pair_runner(n, k, stride, kind, pro):
    from openpifpaf_amd import fused
    spec, h, x, _, w, bias, a_bias = _pair_operands(n, k, stride, kind, pro)
    k1 = k // 2
    conv, dconv = _conv(w[:, :k1].reshape(n, k1, 1, 1)), _conv(w[:, k1:].reshape(n, k - k1, 1, 1), stride)
    h_d, x_d, bias_d = h.cuda().contiguous(memory_format=CL), x.cuda().contiguous(memory_format=CL), bias.cuda()
    ab = None if a_bias is None else a_bias.cuda()
    assert fused.X3_TERMS == 6 and fused.pair_supported(conv, dconv, h_d, x_d, bias_d, ab)

    def run(relu):
        with torch.no_grad():
            return _rows(fused.conv1x1_pair_bias_act_x3(conv, dconv, h_d, x_d, bias_d, relu, ab))
    return run


@functools.lru_cache(maxsize=None)
def _taps_operands(n, stride, dilation, kind):
    g = xc.gen(55 + n + 2 * stride + dilation + (kind == 'randn'))
    c = TAPS_IN[1]
    if kind == 'int':
        x, w4d = xc.integers(TAPS_IN, g, 9), xc.sparse_integer_weight(n, 9 * c, g).reshape(n, c, 3, 3)
        bias = xc.integers((n,), g, 20)
    else:
        x, w4d = torch.randn(TAPS_IN, generator=g), (torch.randn((n, 9 * c), generator=g) * (2.0 / (9 * c)) ** 0.5).reshape(n, c, 3, 3)
        bias = torch.randn((n,), generator=g)
    return x, w4d, bias


def _taps_runner(n, stride, dilation, kind):
    from openpifpaf_amd import fused
    x, w4d, bias = _taps_operands(n, stride, dilation, kind)
    conv, bias_d, x_d = _conv(w4d, stride, dilation, dilation), bias.cuda(), x.cuda().contiguous(memory_format=CL)
    supported, launch = ((fused.conv3x3_x3_supported, fused.conv3x3_bias_act_x3) if dilation == 1 else
                         (fused.conv3x3_dilated_x3_supported, fused.conv3x3_dilated_bias_act_x3))
    assert fused.X3_TERMS == 6 and supported(conv, x_d, bias_d)

    def run(relu):
        with torch.no_grad():
            return _rows(launch(conv, x_d, bias_d, relu))
    return run


# ---- exact ---------------------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('n', NS)
@pytest.mark.parametrize('m', MS)
def test_plain_exact(monkeypatch, m, n, k):
    a, w, bias, res, a_bias = _plain_operands(m, n, k, 'int')
    pres = [_product(a, w, bias, res if r else None, a_bias if p else None) for r, _, p in FLAGS]
    wants = [_expect(pre, relu) for pre, (_, relu, _) in zip(pres, FLAGS)]
    assert all(bool((pre < 0).any()) and bool((pre > 0).any()) for pre in pres)
    _all_different(wants, 'plain')
    _tile(monkeypatch, 256)
    run = _plain_runner(m, n, k, 'int')
    for flags, want in zip(FLAGS, wants):
        got = run(*flags)
        assert torch.equal(got, want), 'M %d N %d K %d res %d relu %d pro %d: %d elements differ' % ((m, n, k) + flags + (int((got != want).sum()),))


@gpu
@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('n', NS)
@pytest.mark.parametrize('stride', [1, 2])
def test_pair_exact(monkeypatch, stride, n, k):
    variants = list(itertools.product((False, True), repeat=2))             # (relu, pro)
    wants = []
    for relu, pro in variants:
        spec, _, _, a, w, bias, a_bias = _pair_operands(n, k, stride, 'int', pro)
        assert a.shape[0] == PAIR_HW[0] * PAIR_HW[1]
        pre = _product(a, w, bias, None, None if a_bias is None else xc.prologue_bias(spec, a_bias))
        assert bool((pre < 0).any()) and bool((pre > 0).any())
        wants.append(_expect(pre, relu))
    _all_different(wants, 'pair')
    _tile(monkeypatch, 256)
    for (relu, pro), want in zip(variants, wants):
        got = _pair_runner(n, k, stride, 'int', pro)(relu)
        assert torch.equal(got, want), 'pair stride %d N %d K %d relu %d pro %d: %d elements differ' % (stride, n, k, relu, pro, int((got != want).sum()))


@gpu
@pytest.mark.parametrize('n', NS)
@pytest.mark.parametrize('dilation', [1, 2])
@pytest.mark.parametrize('stride', [1, 2])
def test_taps_exact(monkeypatch, stride, dilation, n):
    x, w4d, bias = _taps_operands(n, stride, dilation, 'int')
    cols = torch.nn.functional.unfold(x, 3, dilation, dilation, stride)     # [B, 9 C, pixels], zeros in the padding
    pre = _product(cols.transpose(1, 2).reshape(-1, cols.shape[1]), w4d.reshape(n, -1), bias)
    assert bool((pre < 0).any()) and bool((pre > 0).any())
    wants = [_expect(pre, relu) for relu in (False, True)]
    _all_different(wants, 'taps')
    _tile(monkeypatch, 256)
    run = _taps_runner(n, stride, dilation, 'int')
    for relu, want in zip((False, True), wants):
        got = run(relu)
        assert got.shape == want.shape
        assert torch.equal(got, want), 'taps stride %d dilation %d N %d relu %d: %d elements differ' % (stride, dilation, n, relu, int((got != want).sum()))


# ---- bit identity with the 128-wide tile -----------------------------------------------------------------------------------------------------

def _both_tiles(monkeypatch, launch):
    outs = []
    for tile in (128, 256):
        _tile(monkeypatch, tile)
        outs.append(launch())
    return outs


@gpu
@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('n', NS)
@pytest.mark.parametrize('m', MS)
def test_plain_bit_identity(monkeypatch, m, n, k):
    run = _plain_runner(m, n, k, 'randn')
    for flags in FLAGS:
        narrow, wide = _both_tiles(monkeypatch, lambda: run(*flags))
        assert bool(narrow.isfinite().all()) and bool(narrow.any())
        assert torch.equal(narrow.view(torch.int32), wide.view(torch.int32)), 'M %d N %d K %d res %d relu %d pro %d' % ((m, n, k) + flags)


@gpu
@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('n', NS)
@pytest.mark.parametrize('stride', [1, 2])
def test_pair_bit_identity(monkeypatch, stride, n, k):
    for relu, pro in itertools.product((False, True), repeat=2):
        run = _pair_runner(n, k, stride, 'randn', pro)
        narrow, wide = _both_tiles(monkeypatch, lambda: run(relu))
        assert bool(narrow.isfinite().all()) and bool(narrow.any())
        assert torch.equal(narrow.view(torch.int32), wide.view(torch.int32)), 'pair stride %d N %d K %d relu %d pro %d' % (stride, n, k, relu, pro)


@gpu
@pytest.mark.parametrize('n', NS)
@pytest.mark.parametrize('dilation', [1, 2])
@pytest.mark.parametrize('stride', [1, 2])
def test_taps_bit_identity(monkeypatch, stride, dilation, n):
    run = _taps_runner(n, stride, dilation, 'randn')
    for relu in (False, True):
        narrow, wide = _both_tiles(monkeypatch, lambda: run(relu))
        assert bool(narrow.isfinite().all()) and bool(narrow.any())
        assert torch.equal(narrow.view(torch.int32), wide.view(torch.int32)), 'taps stride %d dilation %d N %d relu %d' % (stride, dilation, n, relu)


# ---- guards: nothing written outside the M x N rows, a non-finite value stays in its row ----------------------------------------------------

def _launch_plain(a_d, w3, bias_d, res_d, out_view, m, n, k, relu):
    from openpifpaf_amd import fused
    fused._launch('opa_gemm_bias_act_f32x3', a_d.data_ptr(), None, w3.data_ptr(), bias_d.data_ptr(),
                  None if res_d is None else res_d.data_ptr(), out_view.data_ptr(), m, n, k, int(relu), 6)
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize('with_res', [False, True])
@pytest.mark.parametrize('n', NS)
@pytest.mark.parametrize('m', [129, 257])
def test_guards_and_nonfinite_rows(monkeypatch, m, n, with_res):
    from openpifpaf_amd import fused
    k = 192
    a, w, bias, res, _ = _plain_operands(m, n, k, 'randn')
    _tile(monkeypatch, 256)
    # the operand is an interior view as well: NaN on either side of it would reach the rows that read it
    abuf = torch.full((m * k + 2 * GUARD,), float('nan'), device='cuda')
    a_d = abuf[GUARD:GUARD + m * k].view(m, k)
    w3, bias_d = fused.split_weight(w.cuda()), bias.cuda()
    res_d = res.cuda() if with_res else None
    nan_row, inf_row = 5, m - 1                                            # a row of the first tile, the last row that exists
    outs = {}
    for name, places in (('clean', ()), ('planted', (((nan_row, 3), float('nan')), ((inf_row, k - 1), float('inf'))))):
        a_d.copy_(xc.plant(a, places))
        obuf = torch.full((m * n + 2 * GUARD,), NAN_BITS, dtype=torch.int32, device='cuda')
        _launch_plain(a_d, w3, bias_d, res_d, obuf[GUARD:GUARD + m * n], m, n, k, False)
        assert bool((obuf[:GUARD] == NAN_BITS).all()), name + ': written in front of the output'
        assert bool((obuf[GUARD + m * n:] == NAN_BITS).all()), name + ': written behind row M - 1 (rows past M, or beyond)'
        outs[name] = obuf[GUARD:GUARD + m * n].view(torch.float32).view(m, n).cpu()
    clean, planted = outs['clean'], outs['planted']
    assert bool(clean.isfinite().all())
    assert bool(planted[nan_row].isnan().all()) and bool(planted[inf_row].isnan().all()), 'a non-finite operand does not make its row NaN'
    others = torch.ones(m, dtype=torch.bool)
    others[[nan_row, inf_row]] = False
    assert torch.equal(planted[others].view(torch.int32), clean[others].view(torch.int32)), 'a non-finite value leaked out of its row'


# ---- dispatch: what the wide tile has no instantiation for stays on the 128-wide tile -------------------------------------------------------

@gpu
@pytest.mark.parametrize('n,terms', [(128, 6), (256, 9), (64, 6)])
def test_forced_wide_tile_leaves_other_launches_alone(monkeypatch, n, terms):
    from openpifpaf_amd import fused
    m, k = 257, 128
    a, w, bias, res, _ = _plain_operands(m, n, k, 'randn')
    x, r_d, w_d, bias_d = _image(a, 1, 1, m), _image(res, 1, 1, m), w.cuda(), bias.cuda()
    w3 = fused.split_weight(w_d)
    with torch.no_grad():
        narrow, wide = _both_tiles(monkeypatch, lambda: _rows(fused.conv1x1_bias_act_x3(x, w3, bias_d, r_d, True, None, terms)))
    assert bool(narrow.isfinite().all()) and bool(narrow.any())
    assert torch.equal(narrow.view(torch.int32), wide.view(torch.int32))
    # ... and it is the product: K additions of leading products, the join, bias and residual, each within 2^-24 of a running sum
    # that S = sum |a||w| + |bias| + |res| bounds, and up to 8 K additions of corrections whose sums 2^-7 S bounds -- the textbook
    # worst case -- plus what six terms leave out
    bound = (k + 3 + 8 * k / 128) * 2.0 ** -24 + xc.EXTRA[terms]
    assert xc.err_c(wide, xc.ref64(a, w, bias, res, None, True), xc.scale_of(a, w, bias, res)) <= bound
