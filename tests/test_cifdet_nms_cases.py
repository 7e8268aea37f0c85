"""CifDet NMS on the device, CPU side: the case list the GPU test runs reaches every regime it claims; ``decoder.CifDet._post``
-- the standard the kernel is held to -- equals a float64 brute-force greedy NMS written here from the definition on every
case; no case has a pair whose IoU is within 1e-6 of the threshold (the host's coordinate-offset trick and a category test
differ by rounding at the 1e-13 level, float32 and float64 IoUs by 1e-7: with that margin the keep set is unambiguous); and
the new surface is declared, bound and offered (these three fail without the feature)."""
import os
import re

import numpy as np
import pytest

import cifdet_nms_common as cn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [c[0] for c in cn.CASES]


@pytest.fixture(scope='module')
def facts():
    """Per case: the inputs, the brute-force outcome and what regime they are in."""
    out = {}
    for case in cn.CASES:
        cat, sc, bx = cn.candidates(case)
        post = cn.settings(case)
        kept, survivors = cn.brute_force(cat, sc, bx, **post)
        n = len(sc)
        suppressed = sc[~kept] * np.float32(post['suppression'])
        thr = np.float32(post['instance_threshold'])
        iou = cn.iou_matrix(bx) if n else np.zeros((0, 0))
        off = ~np.eye(n, dtype=bool)
        area = np.maximum(0, bx[:, 2] - bx[:, 0]) * np.maximum(0, bx[:, 3] - bx[:, 1]) if n else np.zeros(0)
        inside = (bx[:, None, 0] <= bx[None, :, 0]) & (bx[:, None, 1] <= bx[None, :, 1]) & \
                 (bx[:, None, 2] >= bx[None, :, 2]) & (bx[:, None, 3] >= bx[None, :, 3]) if n else np.zeros((0, 0), dtype=bool)
        out[case[0]] = dict(
            case=case, inputs=(cat, sc, bx), post=post, kept=kept, survivors=survivors, n=n,
            equal_scores=n > 1 and len(np.unique(sc)) < n,
            unsorted=n > 1 and bool((np.diff(sc) > 0).any()),
            identical_boxes=n > 1 and bool((iou[off] == 1.0).any()) and len(np.unique(bx, axis=0)) < n,
            zero_area=bool((area == 0).any()),
            nested=bool((inside & off & (area[:, None] > area[None, :])).any()) if n else False,
            one_category=n > 1 and len(np.unique(cat)) == 1,
            all_different=n > 1 and len(np.unique(cat)) == n,
            all_suppressed=n > 1 and int(kept.sum()) == 1,
            none_suppressed=n > 1 and bool(kept.all()),
            suppressed_above=bool((suppressed > thr).any()), suppressed_below=bool((suppressed <= thr).any()),
            by_category=post['by_category'],
            other_thresholds=(post['iou_threshold'], post['suppression'], post['instance_threshold']) != (0.5, 0.1, 0.15),
            oracle=case[1] == 'oracle')
    return out


def test_case_list_reaches_every_regime(facts):
    sizes = {f['n'] for f in facts.values()}
    assert {0, 1, 2, 63, 64, 65, 120, 121, 1024} <= sizes, sorted(sizes)
    for regime in ('equal_scores', 'unsorted', 'identical_boxes', 'zero_area', 'nested', 'one_category', 'all_different',
                   'all_suppressed', 'none_suppressed', 'by_category', 'other_thresholds', 'oracle'):
        assert any(f[regime] for f in facts.values()), regime
    assert any(not f['by_category'] for f in facts.values())
    # suppressed scores on both sides of the instance threshold, in ONE case
    assert any(f['suppressed_above'] and f['suppressed_below'] for f in facts.values())
    # the categories only matter where boxes of different categories overlap: a by_category case and its twin without differ
    a, b = facts['all_different'], facts['all_different_any_category']
    assert a['none_suppressed'] and not b['none_suppressed']
    # real decode output: non-increasing scores, the reference's cap of 120 candidates reached
    assert all(not f['unsorted'] for f in facts.values() if f['oracle'])
    assert any(f['oracle'] and f['n'] == 120 for f in facts.values())
    assert all(f['n'] <= 1024 for f in facts.values())


@pytest.mark.parametrize('name', IDS)
def test_margin_condition(facts, name):
    f = facts[name]
    cat, sc, bx = f['inputs']
    m = cn.margin(cat, bx, f['post']['by_category'], f['post']['iou_threshold'])
    print('%s: n = %d, min |IoU - threshold| = %.3g' % (name, f['n'], m))
    assert m >= cn.MARGIN, (name, m)
    assert np.isfinite(bx).all() and np.isfinite(sc).all()


@pytest.mark.parametrize('name', IDS)
def test_post_equals_the_brute_force_model(facts, name):
    f = facts[name]
    got = cn.post_arrays(*f['inputs'], **f['post'])
    assert cn.same_bits(got, f['survivors']), name
    assert len(got[0]) <= f['n']


def test_brute_force_model_on_a_hand_made_case():
    """The model itself, on numbers worked out by hand."""
    cat = np.array([1, 1, 2, 1], dtype=np.int64)
    sc = np.array([0.9, 0.8, 0.7, 0.95], dtype=np.float32)
    bx = np.array([[0, 0, 10, 10], [1, 1, 11, 11], [0, 0, 10, 10], [0, 0, 10, 10.5]], dtype=np.float32)
    # 3 (0.95) first: suppresses 0 (IoU 100/105) and 1 (85.5 / (100 + 105 - 85.5) = 0.715); 2 is another category
    kept, (c, s, b) = cn.brute_force(cat, sc, bx, **cn.DEFAULTS)
    assert kept.tolist() == [False, False, True, True]
    assert c.tolist() == [2, 1] and s.tolist() == [np.float32(0.7), np.float32(0.95)]      # 0.09 and 0.08 fall below 0.15
    assert b.tolist() == [[0, 0, 10, 10], [0, 0, 10, 10.5]]
    kept, (c, s, b) = cn.brute_force(cat, sc, bx, iou_threshold=0.5, suppression=0.5, instance_threshold=0.42, by_category=False)
    assert kept.tolist() == [False, False, False, True]
    assert c.tolist() == [1, 1] and s.tolist() == [np.float32(0.9) * np.float32(0.5), np.float32(0.95)]
    assert abs(cn.iou64(bx[1], bx[3]) - 85.5 / 119.5) < 1e-15


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, 'include', 'openpifpaf_amd.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in ('opa_cifdet_nms', 'opa_cifdet_decode_nms', 'opa_det_post_bytes'):
        assert re.search(r'\b%s\s*\(' % name, code), name
    assert re.search(r'typedef struct opa_det_post \{[^}]*iou_threshold[^}]*suppression[^}]*instance_threshold[^}]*by_category',
                     code, re.S)
    assert 'opa_cifdet_decode(' in code and 'typedef struct opa_det_shape' in code         # and the old ones stay
    assert 'host-side Python in the reference too' not in text


def test_ctypes_table_binds_them():
    import ctypes
    from openpifpaf_amd import _lib
    for name in ('opa_cifdet_nms', 'opa_cifdet_decode_nms', 'opa_det_post_bytes'):
        assert name in _lib.SYMBOLS, name
    L = _lib.lib()
    assert L.opa_det_post_bytes() == ctypes.sizeof(_lib.DetPost) == 32
    post = _lib.DetPost()
    L.opa_default_det_post(ctypes.byref(post))
    assert (post.iou_threshold, post.suppression, post.instance_threshold, post.by_category) == (0.5, 0.1, 0.15, 1)
    # the capacity is refused on the host, before anything touches a device: no GPU is needed to see it
    assert L.opa_cifdet_nms(None, 1, _lib.CIFDET_NMS_MAX + 1, 8, 8, 8, 8, 8, 8, 8, 8, None) == 1
    assert b'OPA_CIFDET_NMS_MAX' in L.opa_last_error()
    shape = _lib.DetShape(1, 8, 41, 41, 8, 2000)
    assert L.opa_cifdet_decode_nms(ctypes.byref(shape), None, None, 8, 8, 1 << 30, 8, 8, 8, 8, None) == 1
    assert L.opa_cifdet_nms(None, 1, 120, None, 8, 8, 8, 8, 8, 8, 8, None) == 1                 # null pointer


def test_decoder_offers_the_asynchronous_path():
    from openpifpaf_amd import decoder, native
    assert hasattr(decoder.CifDet, 'batch_async')
    assert not getattr(decoder.CifDet, 'supports_device_inverse', False)      # boxes are transformed back on the host
    assert hasattr(native.CifDet, 'nms') and hasattr(native.CifDet, 'call_batch_nms')
    multi = decoder.Multi([cn.post_model(**cn.DEFAULTS)])
    assert multi.pipeline_depth == decoder.CifDet.decoder_workers >= 1
