"""The cases of tests/test_gpu_winograd_regimes.py, checked on the CPU (winograd_common.py): that the shapes reach every regime of
the launch of every variant of csrc/winograd.hip, that the dense integer case stays inside the budget in which float32 is exact, and
that the case is telling -- nine mutants of the kernels' walk over tile blocks each change the expected output.

Which shape (B x C_in x C_out x H x W) reaches which class; ``test_every_class_is_reached`` derives the same table from
``wino_geometry`` (``pytest -s`` prints it).  Variants 0, 2, 3, 4 (K-chunks of 16, 64 output channels per workgroup) share every
entry; variant 1 (chunks of 8, 32 channels) has its own where it differs.  Compute units: 256.

  class                                  variants 0, 2, 3, 4                    variant 1
  nwg = 1                                1x16x64x1x1 (and six more)             1x8x32x2x3
  nwg < 8, 2+ tile x 2+ channel blocks   3x48x192x9x11 (2 x 3)                  3x24x64x9x11 (2 x 2), 17x16x64x3x3, 1x16x64x6x80
  nwg = 8q + r                           5x48x192x16x13 (15 = 8 + 7)            5x48x192x16x13 (30), 3x48x192x9x11 (12)
  nwg = 8q                               1x32x512x96x97 (296; variant 3: 256)   1x32x512x96x97 (592)
  T % 64 = 1 / 32 / 33 / 0               1x16x64x1x1 / 2x32x64x8x7 / 3x16x64x2x21 / 4x32x64x8x7         (all variants)
  H odd, W odd                           2x32x64x7x9, 3x48x192x9x11, 17x16x64x3x3, 1x512x64x5x5          (all variants)
  H even / W even                        5x48x192x16x13, 1x256x128x6x6 / 2x32x64x1x6, 1x16x64x6x80       (all variants)
  H = 1 / W = 1 / H = 2                  2x32x64x1x6, 1x16x64x1x1 / 2x16x128x5x1 / 3x16x64x2x21          (all variants)
  3 x 3 images, 17 of them               17x16x64x3x3: block 0 holds 16 images, block 1 the last          (all variants)
  3+ images in a block                   3x48x192x9x11, 3x16x64x2x21, 4x32x64x8x7                         (all variants)
  a wave without a border tile           1x16x64x6x80 (tiles 48..63), 1x32x512x96x97                      (all variants; only
                                         variants 2 and 4 branch on it: ``wave_inside``)
  1 chunk                                1x16x64x1x1, 17x16x64x3x3, ...         1x8x32x2x3
  2 chunks                               2x32x64x7x9, 4x32x64x8x7, ...          1x16x64x1x1, 1x16x64x6x80, ...
  3 chunks                               3x48x192x9x11, 5x48x192x16x13          3x24x64x9x11
  32 chunks                              1x512x64x5x5                           1x256x128x6x6
  16 chunks x 2+ channel blocks          1x256x128x6x6                          1x128x64x3x4
  variant 3 walks a second block         1x32x512x96x97: n_tb = 37 > G = 32; workgroups 0..4 of every channel block walk two
                                         blocks, the last of them the partial block 36 (48 tiles), the other 27 walk one

Variant 5 (``winograd_f23_w8x3w_kernel``: K-chunks of 16, 32 tiles x 128 output channels per workgroup, a wave stages 4 tiles) has
a shape list of its own, ``WIDE_REGIMES``, and its own class table (tile counts modulo 32):

  class                                  variant 5
  nwg = 1                                1x16x128x1x1 (and five more)
  nwg < 8, 2+ tile x 2+ channel blocks   2x32x256x7x9 (2 x 2)
  nwg = 8q + r                           3x48x384x9x11 (9 = 8 + 1), 5x48x384x16x13 (27 = 24 + 3)
  nwg = 8q                               1x32x512x96x97 (74 x 4 = 296 = 8 x 37)
  T % 32 = 1 / 31 / 0                    1x16x128x1x1, 3x16x128x2x21 (T = 33) / 1x16x128x2x62 / 2x32x128x8x7
  H odd, W odd                           2x32x128x7x9, 3x48x384x9x11, 9x16x128x3x3, 1x512x128x5x5
  H even / W even                        5x48x384x16x13, 1x256x256x6x6 / 1x16x128x2x62, 2x32x128x1x6, 1x16x128x6x80
  H = 1 / W = 1 / H = 2                  2x32x128x1x6, 1x16x128x1x1 / 2x16x128x5x1 / 3x16x128x2x21, 1x16x128x2x62
  3 x 3 images, 9 of them                9x16x128x3x3: block 0 holds 8 images, block 1 the last
  3+ images in a block                   3x16x128x2x21 (11 tiles per image), 9x16x128x3x3
  a wave without a border tile           1x16x128x6x80 (tiles 44..47), 5x48x384x16x13, 1x32x512x96x97 (the kernel does not branch
                                         on it: its padding costs no select)
  an odd number of channel blocks        3x48x384x9x11, 5x48x384x16x13 (3 blocks of 128: the filter's 64-channel blocks 4, 5)
  1 / 2 / 3 chunks                       1x16x128x1x1 / 2x32x128x7x9, 1x32x512x96x97 / 3x48x384x9x11
  32 chunks                              1x512x128x5x5
  16 chunks x 2+ channel blocks          1x256x256x6x6"""
import pytest

torch = pytest.importorskip('torch')

import winograd_common as wc  # noqa: E402
import x3_common as xc  # noqa: E402


def _sid(shape):
    return 'x'.join(str(v) for v in shape)


# ---- the launch model ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('variant', wc.VARIANTS)
def test_every_class_is_reached(variant):
    table = wc.reached(variant)
    for name, shapes in table.items():
        print('WINOCASE variant %d | %-44s | %s' % (variant, name, ' '.join(_sid(s) for s in shapes) or 'NOT REACHED'))
    assert not [name for name, shapes in table.items() if not shapes]


def test_the_docstring_names_a_shape_that_reaches_each_class():
    """The table above is written by hand: every class's line names at least one shape that ``reached`` lists for it."""
    text = ' '.join(__doc__.split())
    for variant in wc.VARIANTS:
        for name, shapes in wc.reached(variant).items():
            assert any(_sid(s) in text for s in shapes), (variant, name)


def test_geometry_of_the_shapes_the_issue_names():
    g = wc.wino_geometry((3, 48, 192, 9, 11), 2)
    assert (g['T'], g['n_tb'], g['n_nb'], g['nwg'], g['xcd'], g['t_mod'], g['nchunks']) == (90, 2, 3, 6, wc.BELOW8, 26, 3)
    g = wc.wino_geometry((5, 48, 192, 16, 13), 4)
    assert (g['T'], g['n_tb'], g['nwg'], g['xcd']) == (280, 5, 15, wc.MIXED)
    g = wc.wino_geometry(wc.WALK, 3)
    assert (g['T'], g['n_tb'], g['n_nb'], g['G'], g['nwg'], g['longest_walk'], g['shortest_walk']) == (2352, 37, 8, 32, 256, 2, 1)
    assert wc.wino_geometry(wc.WALK, 2)['nwg'] == 296 and wc.wino_geometry(wc.WALK, 1)['nwg'] == 592
    assert wc.wino_geometry(wc.WALK, 3, cus=304)['G'] == 37 and not wc.walks_a_second_block(wc.WALK, wc.wino_geometry(wc.WALK, 3, cus=304))
    g = wc.wino_geometry((1, 16, 64, 6, 80), 2)
    assert g['interior_wave'] and not wc.wino_geometry((2, 32, 64, 7, 9), 2)['interior_wave']
    assert wc.wino_geometry((17, 16, 64, 3, 3), 0)['images_per_block'] == 16


def test_geometry_of_the_wide_shapes_the_issue_names():
    """Variant 5's launch, worked out by hand from ``launch_wino_w8x3w``: ceil(T / 32) tile blocks x C_out / 128 channel blocks."""
    def geo(shape):
        g = wc.wino_geometry(shape, 5)
        return g['T'], g['n_tb'], g['n_nb'], g['nwg'], g['xcd'], g['t_mod'], g['nchunks']
    assert geo((1, 16, 128, 1, 1)) == (1, 1, 1, 1, wc.ONE, 1, 1)
    assert geo((2, 32, 128, 8, 7)) == (32, 1, 1, 1, wc.ONE, 0, 2)
    assert geo((3, 16, 128, 2, 21)) == (33, 2, 1, 2, wc.BELOW8, 1, 1)
    assert geo((1, 16, 128, 2, 62)) == (31, 1, 1, 1, wc.ONE, 31, 1)
    assert geo((2, 32, 256, 7, 9)) == (40, 2, 2, 4, wc.BELOW8, 8, 2)
    assert geo((3, 48, 384, 9, 11)) == (90, 3, 3, 9, wc.MIXED, 26, 3)
    assert geo((5, 48, 384, 16, 13)) == (280, 9, 3, 27, wc.MIXED, 24, 3)
    assert geo(wc.WALK) == (2352, 74, 4, 296, wc.MULTIPLE8, 16, 2)
    assert geo((1, 512, 128, 5, 5))[6] == 32 and geo((1, 256, 256, 6, 6))[2::4] == (2, 16)
    assert wc.wino_geometry((9, 16, 128, 3, 3), 5)['images_per_block'] == 8
    assert wc.wino_geometry((3, 16, 128, 2, 21), 5)['images_per_block'] == 3
    assert wc.wino_geometry((1, 16, 128, 6, 80), 5)['interior_wave'] and not wc.wino_geometry((2, 32, 128, 7, 9), 5)['interior_wave']
    # the shapes variant 4's rule hands to this kernel are pinned narrow in the GPU tests: WALK is one (296 >= 256 wide workgroups)
    assert wc.wino_geometry(wc.WALK, 4)['nwg'] == 296 and wc.wino_geometry(wc.WALK, 4)['n_tb'] == 37


@pytest.mark.parametrize('order', [0, 1])
@pytest.mark.parametrize('variant', wc.VARIANTS)
def test_every_tile_block_and_channel_block_is_computed_once(variant, order):
    """The XCD remap is a permutation of the logical workgroups in all three of its cases, so the (channel block, tile block) pairs
    of a launch are each computed exactly once -- by walks, for variant 3."""
    for shape in wc.shapes_of(variant):
        g = wc.wino_geometry(shape, variant, order)
        assert sorted(wc.logical_of(b, g['nwg']) for b in range(g['nwg'])) == list(range(g['nwg']))
        pairs = sorted((nb, tb) for nb, walk in g['blocks'] for tb in walk)
        assert pairs == [(nb, tb) for nb in range(g['n_nb']) for tb in range(g['n_tb'])], shape


# ---- the dense integer case ---------------------------------------------------------------------------------------------------------------

def _is_multiple(t, unit):
    return bool(((t / unit).round() * unit == t).all())


@pytest.mark.parametrize('shape', wc.WINO_REGIMES + [s for s in wc.WIDE_REGIMES if s not in wc.WINO_REGIMES], ids=_sid)
def test_dense_integer_case_stays_inside_its_bit_budget(shape):
    """Every intermediate of F(2x2, 3x3) on the case -- both passes of the input transform, U, every partial sum over the channels
    in any order (bounded by ``m_abs``) and of the output transform (``y_abs``), the output plus the bias -- is a multiple of 1/4
    below 2^22, i.e. a float32 number: every variant must return the float64 convolution bit for bit.  U is one bfloat16 piece and
    V needs two, so variant 4's second piece is at work in a dense sum.  The bit count is the largest one up to 12 that fits."""
    from openpifpaf_amd import winograd
    x, f, bias, want = wc.winograd_dense_integer_case(shape)
    half, v, u, m_abs, m, y_abs = xc.winograd_intermediates(x, f)
    for t in (half, v, u, m_abs, m, y_abs):
        assert _is_multiple(t, 0.25) and float(t.abs().max()) < wc.BUDGET
    used = wc.budget_used(x, f)
    print('WINOCASE budget %-18s | %2d bits | %.0f %% used' % (_sid(shape), wc.BITS[shape], 100 * used))
    assert float((want.abs() + bias.abs()[None, :, None, None]).max()) < 2.0 ** 24
    if wc.BITS[shape] < wc.MAX_BITS:
        assert wc.budget_used(*wc.dense_integer_operands(shape, 21, wc.BITS[shape] + 1)[:2]) >= 1.0
    assert bool((f != 0).flatten(2).any(2).all()) and float((f == 0).float().mean()) < 0.2         # dense: one weight in nine is 0
    pv, pu = xc.split3(v.float()), xc.split3(u.float())
    assert torch.equal(u.float().double(), u) and bool((pu[1:] == 0).all())
    assert bool((pv[1] != 0).any()) and wc.BITS[shape] >= 9
    assert torch.equal(winograd.reference_f23(x, f), want)


@pytest.mark.parametrize('variant', wc.VARIANTS)
def test_the_tile_walk_is_the_convolution(variant):
    """The float64 restatement of the kernels' walk (clamped tiles, clamped offsets and zero selects, chunks, output halves, masks)
    returns the expected output of every shape in both workgroup orders: the mutants below damage a correct model."""
    for shape in wc.shapes_of(variant):
        x, f, _, want = wc.winograd_dense_integer_case(shape)
        for order in (0, 1):
            assert torch.equal(wc.tile_walk(x, f, variant, order), want), (shape, order)


@pytest.mark.parametrize('mutant', wc.MUTANTS)
def test_mutants_of_the_walk_change_the_expected_output(mutant):
    """Each mutant changes the dense integer case's output at EVERY shape at which the mutated path runs at all (variant 2's
    geometry; variant 1's for its own shapes; variant 3's for the walk; variant 5's on its own list) -- the known-answer test of
    any such shape fails it.  Every mutant but the walk's (variant 3 alone walks) and the padding select (variant 5 has none: the
    offset mutant stands in for it) runs at one wide shape or more."""
    ran = {2: 0, 1: 0, 3: 0, 5: 0}
    for variant in ran:
        for shape in wc.shapes_of(variant):
            if (variant == 1 and wc.supports(2, shape)) or (variant == 3) != (mutant == wc.MUTANTS[6]):
                continue
            if not wc.mutant_applies(mutant, shape, wc.wino_geometry(shape, variant), variant):
                continue
            x, f, _, want = wc.winograd_dense_integer_case(shape)
            got = wc.tile_walk(x, f, variant, 0, mutant=mutant)
            wrong = int((~(got == want)).sum())
            print('WINOCASE mutant %-50s | variant %d %-18s | %d of %d outputs differ' % (mutant, variant, _sid(shape), wrong, want.numel()))
            assert wrong > 0, (shape, variant)
            ran[variant] += 1
    assert sum(ran.values()) >= 1
    assert ran[5] >= 1 or mutant in (wc.MUTANTS[5], wc.MUTANTS[6])


def test_the_walk_mutant_needs_more_tile_blocks_than_workgroups():
    """On a part with 304 compute units variant 3 walks one block per workgroup at WALK and the mutant is the kernel itself: the
    GPU test asserts its premise (``n_tb > G``) from the device's own count."""
    x, f, _, want = wc.winograd_dense_integer_case(wc.WALK)
    assert torch.equal(wc.tile_walk(x, f, 3, 0, cus=304, mutant=wc.MUTANTS[6]), want)


# ---- the float32 restatement ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', [(2, 32, 64, 7, 9), (1, 512, 64, 5, 5)], ids=_sid)
def test_float32_restatement_is_exact_on_the_integer_case_and_inside_the_hard_bound(shape):
    """``model_plain_f32`` returns the dense integer case bit for bit (it is the algorithm), and on the N(0, 1) case its error in the
    componentwise measure is below the hard bound the GPU test sets, (R + C_in) 2^-24 with R = 9."""
    x, f, _, want = wc.winograd_dense_integer_case(shape)
    assert torch.equal(wc.model_plain_f32(x, f).double(), want)
    x, f, bias, ref, S = wc.winograd_randn_case(shape)
    for x3 in (False, True):
        e_max, e_rms = wc.max_rms(wc.model_f32(shape, x3), ref, S)
        print('WINOCASE model %-14s %s | max %.3e rms %.3e' % (_sid(shape), 'variant 4' if x3 else 'variants 0-3', e_max, e_rms))
        assert e_max <= (9 + shape[1]) * 2.0 ** -24 + (xc.EXTRA[6] if x3 else 0.0)
