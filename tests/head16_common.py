"""What the tests of the 16-bit head route (``fused.HEAD16``: ``csrc/head16.hip``) share: head metas with a field count set by hand
and the launch geometries that the store plan's stand-alone checker (``tests/host/head16_plan_main.cpp``) runs too."""
from openpifpaf_amd import headmeta

# (B, hc, wc, F, C, us) of tests/host/head16_plan_main.cpp: a partial row tile; three row tiles whose 32-row blocks cross image rows
# and images; no upsampling; one pixel with three of its four sub-pixels cropped; M = 128 exactly with 20 live columns in the last N-tile
GEOMETRIES = ((2, 5, 7, 2, 5, 2), (3, 9, 11, 3, 8, 2), (1, 33, 4, 13, 6, 1), (1, 1, 1, 1, 5, 2), (1, 8, 16, 17, 5, 2))
KIND_OF_COMPONENTS = {5: 'cif', 8: 'caf', 6: 'cifdet'}


def meta(kind, n_fields, upsample):
    """A Cif (5 components), Caf (8) or CifDet (6: no scales, the offset on the first vector alone) meta of ``n_fields`` fields."""
    if kind == 'cif':
        m = headmeta.Cif('cif', 'head16', keypoints=['k%d' % i for i in range(n_fields)])
    elif kind == 'caf':
        m = headmeta.Caf('caf', 'head16', skeleton=[(1, 2)] * n_fields)
    else:
        assert kind == 'cifdet', kind
        m = headmeta.CifDet('cifdet', 'head16', categories=['c%d' % i for i in range(n_fields)])
    m.upsample_stride = upsample
    assert m.n_fields == n_fields
    return m


def n_components(m):
    return 1 + m.n_confidences + 2 * m.n_vectors + m.n_scales


def offset_mask(m):
    return sum(1 << i for i, on in enumerate(m.vector_offsets) if on)
