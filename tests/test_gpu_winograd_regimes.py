"""Every variant of csrc/winograd.hip (0-3 through ``winograd.conv3x3``, 4 and 5 through ``winograd.conv3x3_x3``) in both workgroup
orders at ``winograd_common.WINO_REGIMES`` -- small shapes that together reach every regime of the launch: the three cases of the
XCD remap, a last tile block of 1 / 32 / 33 / 64 tiles, H and W of 1, 2, odd and even, blocks that hold many images, waves without a
border tile, 1 / 2 / 3 / 16 / 32 K-chunks, and variant 3 walking a second tile block.  tests/test_winograd_cases.py says which shape
reaches what, checks the bit budget of the integer case and shows mutants of the walk failing it.
Variant 5 (``winograd_f23_w8x3w_kernel``, 32 tiles x 128 channels) runs at ``winograd_common.WIDE_REGIMES``, the same classes for
its own blocks (a last block of 1 / 31 / 32 tiles, eight images to a block, an odd count of channel blocks).  Variant 4 would take
that kernel by the launcher's rule where it pays (``WALK``); every test here holds it to its 64-channel kernel with
``OPA_WINO_X3_BN=64``, so that the kernel that runs is the one ``winograd_common`` models for the variant, whatever the rule says.
  (a) known answer: dense integer operands inside the budget in which float32 is exact -- the float64 convolution, bit for bit;
  (b) the same through interior views of NaN-filled buffers: nothing read that is not selected away, nothing written outside;
  (c) invariances on N(0, 1) data, bit for bit: relaunch, workgroup order, an image alone, the batch reversed, variant 3 = variant 2;
  (d) NaN and +-Inf in the operands of the float32 variants stay in their windows and channels;
  (e) accuracy on N(0, 1) data in the componentwise measure: a hard bound on the maximum from the count of roundings, and the rms
      against a float32 restatement on the CPU.  Every case prints a ``WINOREG`` line (``pytest -s``); the lines of a run are kept
      in ``profiles/winograd_regimes/errors.log``."""
import functools

import pytest

torch = pytest.importorskip('torch')

import winograd_common as wc  # noqa: E402
import x3_common as xc  # noqa: E402

pytestmark = pytest.mark.gpu

CL = torch.channels_last
NAN, INF = float('nan'), float('inf')
GUARD = 4096                                            # floats on either side of x and of the output (16 KB: more than one output row
                                                        # of any shape here, which is what a dropped ``oh >= H`` mask would write past the end)
PATTERN = 0x7FC0BEEF                                    # a NaN the kernels never produce

CASES = [pytest.param(v, s, id='v%d-%s' % (v, 'x'.join(map(str, s)))) for v in wc.VARIANTS for s in wc.shapes_of(v)]


@pytest.fixture(autouse=True)
def _variant_4_on_its_64_channel_kernel(monkeypatch):
    """The launcher reads the variable on every launch; variant 5 is the 128-channel kernel whatever it says."""
    monkeypatch.setenv('OPA_WINO_X3_BN', '64')


def _cl(t):
    return t.cuda().contiguous(memory_format=CL)


@functools.lru_cache(maxsize=None)
def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _filter(f, variant):
    from openpifpaf_amd import winograd
    f = f.cuda()
    return winograd.split_filter(f) if variant >= 4 else winograd.transform_filter(f, variant)


def _launch(x_dev, u, c_out, variant, order, bias=None, relu=False, out=None):
    """One launch on operands already on the device -> the device tensor."""
    from openpifpaf_amd import winograd
    with torch.no_grad():
        if variant >= 4:
            return winograd.conv3x3_x3(x_dev, u, c_out, bias=bias, relu=relu, variant=variant, order=order, out=out)
        return winograd.conv3x3(x_dev, u, c_out, bias=bias, relu=relu, variant=variant, order=order, out=out)


def _run(x, f, variant, order, bias=None, relu=False):
    """CPU operands -> the result on the CPU, standard layout."""
    out = _launch(_cl(x), _filter(f, variant), f.shape[0], variant, order, None if bias is None else bias.cuda(), relu)
    torch.cuda.synchronize()
    assert out.shape == (x.shape[0], f.shape[0]) + tuple(x.shape[2:]) and out.is_contiguous(memory_format=CL)
    return out.cpu().contiguous()


def _premise(variant, shape):
    """The regime a shape is in the list for must be the one this device gives it: variant 3's walk depends on the compute units."""
    if variant == 3 and shape == wc.WALK:
        geo = wc.wino_geometry(shape, 3, 0, _cus())
        assert geo['n_tb'] > geo['G'] and wc.walks_a_second_block(shape, geo), (_cus(), geo['n_tb'], geo['G'])


def _with_bias(want, bias, relu):
    out = want + bias.double()[None, :, None, None]
    return out.clamp_min(0) if relu else out


# ---- (a) known answer ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('order', [0, 1])
@pytest.mark.parametrize('variant,shape', CASES)
def test_dense_integer_case_is_returned_bit_for_bit(variant, shape, order):
    """Integer inputs, a dense filter of integers in [-4, 4]: every partial sum of every variant, in any order, is a float32 number
    (test_winograd_cases.py), so the result is the float64 convolution exactly -- variant 4's too, whose U is one bfloat16 piece
    and whose V needs two.  Without bias, and with an integer bias and ReLU."""
    _premise(variant, shape)
    x, f, bias, want = wc.winograd_dense_integer_case(shape)
    got = _run(x, f, variant, order)
    assert torch.equal(got.double(), want), int((got.double() != want).sum())
    got = _run(x, f, variant, order, bias, True)
    assert torch.equal(got.double(), _with_bias(want, bias, True)), int((got.double() != _with_bias(want, bias, True)).sum())


# ---- (b) guard bands ----------------------------------------------------------------------------------------------------------------------

def _interior_nhwc(buf, b, c, h, w):
    """The [B, C, H, W] channels-last view of ``buf[GUARD:GUARD + B H W C]``."""
    view = buf[GUARD:GUARD + b * h * w * c].view(b, h, w, c).permute(0, 3, 1, 2)
    assert view.is_contiguous(memory_format=CL) and view.data_ptr() % 16 == 0
    return view


@pytest.mark.parametrize('order', [0, 1])
@pytest.mark.parametrize('variant,shape', CASES)
def test_nothing_is_read_or_written_outside_the_operands(variant, shape, order):
    """(a) with x and the output as 16-byte-aligned interior views of larger buffers: 16 KB of NaN on either side of x, the output
    buffer filled with a NaN bit pattern.  The result is still exact (a pixel loaded outside x and not replaced by the padding's
    zero would show as NaN; an output the kernel does not write keeps the pattern), the output's surroundings keep their bits and
    x is unchanged."""
    _premise(variant, shape)
    x, f, bias, want = wc.winograd_dense_integer_case(shape)
    B, C, O, H, W = shape
    xbuf = torch.full((B * H * W * C + 2 * GUARD,), NAN, device='cuda')
    xv = _interior_nhwc(xbuf, B, C, H, W)
    xv.copy_(x.cuda())
    x_before = xbuf.view(torch.int32).clone()
    n_out = B * H * W * O
    obuf = torch.full((n_out + 2 * GUARD,), PATTERN, dtype=torch.int32, device='cuda')
    ov = _interior_nhwc(obuf.view(torch.float32), B, O, H, W)
    out = _launch(xv, _filter(f, variant), O, variant, order, bias.cuda(), True, out=ov)
    torch.cuda.synchronize()
    assert out.data_ptr() == ov.data_ptr()
    assert torch.equal(ov.cpu().contiguous().double(), _with_bias(want, bias, True))
    assert bool((obuf[:GUARD] == PATTERN).all()) and bool((obuf[GUARD + n_out:] == PATTERN).all())
    assert torch.equal(xbuf.view(torch.int32), x_before)


# ---- (c) invariances ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('variant,shape', CASES)
def test_relaunch_order_single_image_and_reversed_batch_are_bit_identical(variant, shape):
    """N(0, 1) data with bias.  A second launch equals the first; ``order=1`` equals ``order=0`` (only the map from workgroups to
    tiles differs); image b of the batch equals the same image run alone, and the batch with its images reversed gives the reversed
    result (a tile's arithmetic does not depend on its place in a block, a wave or the launch)."""
    _premise(variant, shape)
    x, f, bias, _, _ = wc.winograd_randn_case(shape)
    x_dev, u, b_dev, O = _cl(x), _filter(f, variant), bias.cuda(), shape[2]
    first = _launch(x_dev, u, O, variant, 0, b_dev)
    assert bool(first.isfinite().all())
    assert torch.equal(_launch(x_dev, u, O, variant, 0, b_dev), first)
    assert torch.equal(_launch(x_dev, u, O, variant, 1, b_dev), first)
    for b in sorted({0, shape[0] // 2, shape[0] - 1}):
        alone = _launch(_cl(x[b:b + 1]), u, O, variant, 0, b_dev)
        assert torch.equal(alone[0], first[b]), b
    if shape[0] > 1:
        assert torch.equal(_launch(_cl(x.flip(0)), u, O, variant, 0, b_dev), first.flip(0))


@pytest.mark.parametrize('shape', wc.shapes_of(3), ids=str)
def test_variant_3_equals_variant_2_bit_for_bit(shape):
    """Read off the two kernels: variant 3 forms V with the same additions (its zero selects are unconditional, variant 2's are
    skipped where every pixel is valid -- the same values), issues the same MFMAs in the same order on the same filter layout
    into accumulators zeroed per block, and its output transform is variant 2's text.  Only which workgroup computes a block, and
    when its pixels are fetched, differ: the results are equal bit for bit, with and without bias and ReLU."""
    _premise(3, shape)
    x, f, bias, _, _ = wc.winograd_randn_case(shape)
    x_dev, u, b_dev = _cl(x), _filter(f, 2), bias.cuda()
    for b, relu in ((None, False), (b_dev, True)):
        assert torch.equal(_launch(x_dev, u, shape[2], 3, 0, b, relu), _launch(x_dev, u, shape[2], 2, 0, b, relu))


# ---- (d) non-finite operands, variants 0-3 --------------------------------------------------------------------------------------------------

def _check(what, got, clean, cls, relu):
    bad = xc.nonfinite_violations(got, clean, cls, relu)
    assert not any(bad.values()), (what, bad)


@pytest.mark.parametrize('order', [0, 1])
@pytest.mark.parametrize('variant', [0, 1, 2, 3])
def test_non_finite_inputs_stay_in_their_windows(variant, order):
    """The places of ``test_winograd_non_finite_inputs_stay_in_their_windows`` (test_gpu_x3_edges.py) for the float32 MFMA variants.
    The contract, from the code: ``B^T d B`` and ``A^T M A`` only add and subtract, the MFMA multiplies a tile's V by finite U and
    adds along K within one (tile, channel) element, and the LDS round trips move whole elements -- so an output whose 3x3
    window holds no planted pixel never meets one (rows 0-2 of the tile feed output row 0, rows 1-3 row 1, columns alike) and is
    bit for bit the clean run's, in the same tile too.  Inside a window a NaN pixel gives NaN.  An infinite pixel enters V with
    both signs (d1 + d2 and d2 - d1), reaches the accumulators as +-Inf -- the float32 MFMA keeps an infinity, where variant 4's
    split turns it into NaN before the product -- and the output transform then adds infinities of either sign: the result is
    NaN wherever two of them disagree, and otherwise the infinity of the true sum's sign (the infinite terms that agree in sign
    are the terms of w x Inf taken apart).  So: NaN -> NaN; +-Inf -> that infinity or NaN; with ReLU NaN, 0 or +Inf -- the same
    classes as variant 4, with the infinity possible where variant 4 always gives NaN."""
    x, f, bias = xc.winograd_randn_case(wc.NONFINITE_SHAPE, 15)
    B, C, H, W = x.shape
    places = [((0, 3, 0, 0), NAN), ((0, C - 1, H - 1, W - 1), INF), ((1, 0, 3, 4), -INF)]
    x_bad = xc.plant(x, places)
    cls = xc.nonfinite_class(torch.nn.functional.conv2d(x_bad, f, bias, padding=1))
    window = torch.zeros((B, 1, H, W), dtype=torch.bool)
    for (b, _, y, xx), _ in places:
        window[b, 0, max(y - 1, 0):y + 2, max(xx - 1, 0):xx + 2] = True
    assert torch.equal(cls != xc.FINITE, window.expand(B, f.shape[0], H, W))
    for relu in (False, True):
        clean = _run(x, f, variant, order, bias, relu)
        got = _run(x_bad, f, variant, order, bias, relu)
        assert bool(clean.isfinite().all())
        _check((variant, relu), got, clean, cls, relu)


@pytest.mark.parametrize('order', [0, 1])
@pytest.mark.parametrize('variant', [0, 1, 2, 3])
def test_non_finite_filter_and_bias_stay_in_their_channels(variant, order):
    """The places of ``test_winograd_non_finite_filter_and_bias_stay_in_their_channels``.  ``G g G^T`` (float64, on the host) spreads
    a non-finite tap over the sixteen positions of its (c_out, c_in) pair -- an infinite tap as NaN too, 0 x Inf among the
    products of G's zeros -- and an MFMA column belongs to one output channel: that CHANNEL is NaN (allowed where the reference has
    an infinity), an infinite bias gives its infinity, and every other channel is bit for bit the clean run's."""
    x, f, bias = xc.winograd_randn_case(wc.NONFINITE_SHAPE, 16)
    B, C, H, W = x.shape
    O = f.shape[0]
    f_bad = xc.plant(f, [((1, 0, 0, 0), NAN), ((O // 2, C - 1, 1, 1), INF), ((O - 1, 5, 2, 2), -INF)])
    bias_bad = xc.plant(bias, [((3,), INF)])
    ref32 = xc.ref32(xc.im2col_3x3(x, 1), xc.weight_rows(f_bad), bias_bad)
    cls = xc.nonfinite_class(xc.image_of(ref32, B, H, W))
    assert sorted(set((cls != xc.FINITE).any(0).any(1).any(1).nonzero().flatten().tolist())) == sorted({1, 3, O // 2, O - 1})
    for relu in (False, True):
        clean = _run(x, f, variant, order, bias, relu)
        got = _run(x, f_bad, variant, order, bias_bad, relu)
        assert bool(clean.isfinite().all())
        _check((variant, 'filter', relu), got, clean, cls, relu)
        assert bool((got[:, 3] == INF).all())


# ---- (e) accuracy -------------------------------------------------------------------------------------------------------------------------

ROUNDINGS = 9


@pytest.mark.parametrize('order', [0, 1])
@pytest.mark.parametrize('variant,shape', CASES)
def test_accuracy_in_the_componentwise_measure(variant, shape, order):
    """N(0, 1) data with bias against the float64 convolution, ``x3_common.err_c`` with S = ``winograd_scale`` + |bias|.
    (i) ``err_c <= (R + C_in) 2^-24`` (+ 2^-23 for variant 4's three dropped products; variant 5 promises variant 4's bits and
        takes its bars unchanged).  C_in = nchunks x KC roundings in the
        channel sum (one per fma of the MFMA's k-ordered chain), and outside it, counted from the kernels, R = 9: two in
        ``B^T d B`` (one addition per pass and element), one of U (float64 -> float32, once), two in the nu-sum (variant 0:
        (m0 + m1) + m2 in registers; variants 2-4: ma + mb in the wave, the wave pair's halves added from LDS), two in the
        xi-sum ((P0 + P1) + P2), one adding the bias -- eight, each at most 2^-24 of the magnitudes it adds, which S sums up --
        and one for every second-order term ((R + C_in)^2 2^-48 / 2 < 2^-24 up to C_in = 5000).
    (ii) the rms of the same ratio is at most 2 x the rms of a float32 restatement on the CPU (``winograd_common.model_f32``:
        transforms in float32, U rounded once, channels added in k order; ``winograd_model_f32`` for variants 4 and 5) -- 2 is what
        ``trunk_common.report`` grants another summation order.  Where C_out > 192 both are taken over every eighth channel."""
    _premise(variant, shape)
    x, f, bias, ref, S = wc.winograd_randn_case(shape)
    got = _run(x, f, variant, order, bias)
    assert bool(got.isfinite().all())
    ch = wc.sampled_channels(shape)
    k_max, _ = wc.max_rms(got, ref, S)
    _, k_rms = wc.max_rms(got[:, ch], ref[:, ch], S[:, ch])
    m_max, m_rms = wc.max_rms(wc.model_f32(shape, variant >= 4), ref[:, ch], S[:, ch])
    bound = (ROUNDINGS + shape[1]) * 2.0 ** -24 + (xc.EXTRA[6] if variant >= 4 else 0.0)
    print('WINOREG v%d order %d %-18s | model max %.3e rms %.3e | kernel max %.3e rms %.3e | rms ratio %.2f | bound %.3e %s'
          % (variant, order, 'x'.join(map(str, shape)), m_max, m_rms, k_max, k_rms, k_rms / max(m_rms, 1e-30), bound,
             'ok' if k_max <= bound and k_rms <= 2 * m_rms else 'ABOVE'))
    assert k_max <= bound, (k_max, bound)
    assert k_rms <= 2 * m_rms, (k_rms, m_rms)
