"""Shared by the CifDet NMS tests: the case list (plain tuples, seeded), the candidate generators, a from-scratch float64
greedy NMS (the model that pins ``decoder.CifDet._post``), and ``_post`` itself as the standard the kernel is held to."""
import numpy as np

# reference decoder/cifdet.py:17-20
DEFAULTS = dict(iou_threshold=0.5, suppression=0.1, instance_threshold=0.15, by_category=True)
MARGIN = 1e-6            # min |IoU - iou_threshold| over pairs that may suppress each other: asserted on every case

# (name, kind, n, seed, overrides of DEFAULTS as a tuple of (key, value))
#   kinds: see candidates(); 'oracle': n = objects of synth.synth_det_field(seed, n, height=H, width=W), the oracle's candidates
CASES = [
    ('empty', 'random', 0, 100, ()),
    ('one', 'random', 1, 101, ()),
    ('two', 'random', 2, 102, ()),
    ('n63', 'random', 63, 103, ()),
    ('n64', 'random', 64, 104, ()),
    ('n65', 'random', 65, 105, ()),
    ('n120', 'random', 120, 106, ()),
    ('n121', 'random', 121, 107, ()),
    ('n300', 'random', 300, 108, ()),
    ('n1024', 'random', 1024, 109, ()),
    ('n1024_any_category', 'random', 1024, 110, (('by_category', False),)),
    ('sorted', 'sorted', 120, 111, ()),
    ('equal_scores', 'equal', 90, 112, ()),
    ('few_score_values', 'few_scores', 130, 113, ()),
    ('identical_boxes', 'identical', 70, 114, ()),
    ('zero_area', 'zero_area', 66, 115, ()),
    ('nested', 'nested', 48, 116, ()),
    ('nested_low_iou', 'nested', 48, 117, (('iou_threshold', 0.3),)),
    ('one_category', 'one_category', 120, 118, ()),
    ('all_different', 'all_different', 100, 119, ()),
    ('all_different_any_category', 'all_different', 100, 119, (('by_category', False),)),
    ('all_suppressed', 'pile', 64, 120, ()),
    ('all_suppressed_129', 'pile', 129, 121, ()),
    ('none_suppressed', 'grid', 120, 122, ()),
    ('both_sides_of_threshold', 'random', 120, 123, (('instance_threshold', 0.05),)),
    ('any_category', 'random', 120, 124, (('by_category', False),)),
    ('other_thresholds', 'random', 120, 125, (('iou_threshold', 0.3), ('suppression', 0.5), ('instance_threshold', 0.3))),
    ('high_iou', 'random', 200, 126, (('iou_threshold', 0.75), ('suppression', 0.25), ('instance_threshold', 0.1))),
    ('oracle_1', 'oracle', 1, 0, (('field', (41, 41)),)),
    ('oracle_5', 'oracle', 5, 1, (('field', (41, 41)),)),
    ('oracle_12', 'oracle', 12, 2, (('field', (33, 49)),)),
    ('oracle_30', 'oracle', 30, 3, (('field', (81, 81)),)),
    ('oracle_150', 'oracle', 150, 4, (('field', (81, 81)),)),
    ('oracle_60_any_category', 'oracle', 60, 7, (('field', (81, 81)), ('by_category', False))),
]


def settings(case):
    out = dict(DEFAULTS)
    out.update({k: v for k, v in case[4] if k != 'field'})
    return out


def _boxes(rng, n, lo=8.0, hi=150.0, extent=400.0):
    w, h = rng.uniform(lo, hi, n), rng.uniform(lo, hi, n)
    cx, cy = rng.uniform(0.5 * w, extent), rng.uniform(0.5 * h, extent)      # (coordinates stay non-negative)
    return np.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], axis=1)


def candidates(case):
    """-> (categories int64 [n], scores float32 [n], boxes float32 [n,4] as x0 y0 x1 y1)."""
    name, kind, n, seed, extra = case
    if kind == 'oracle':
        from openpifpaf_amd import synth
        from oracle import port
        H, W = dict(extra)['field']
        cat, sc, bx = port.cifdet_decode(synth.synth_det_field(seed, n, height=H, width=W), 8)
        return np.asarray(cat, dtype=np.int64), np.asarray(sc, dtype=np.float32), np.asarray(bx, dtype=np.float32)
    rng = np.random.default_rng(seed)
    cat = rng.integers(1, 5, n)
    sc = rng.uniform(0.16, 1.0, n)
    bx = _boxes(rng, n)
    if kind == 'sorted':
        sc = np.sort(sc)[::-1]
    elif kind == 'equal':
        sc = np.full(n, 0.625)
    elif kind == 'few_scores':
        sc = rng.choice([0.25, 0.5, 0.75], n)
    elif kind == 'identical':
        bx = bx[rng.integers(0, 9, n)]                   # nine distinct boxes, each many times
    elif kind == 'zero_area':
        flat = rng.integers(0, 3, n)
        bx[flat == 0, 2] = bx[flat == 0, 0]              # no width
        bx[flat == 1, 3] = bx[flat == 1, 1]              # no height
        bx[: n // 6] = bx[0]                             # and identical ones among them
    elif kind == 'nested':
        centre = rng.uniform(150.0, 250.0, (n // 12 + 1, 2))[rng.integers(0, n // 12 + 1, n)]
        half = rng.uniform(3.0, 120.0, (n, 2))
        bx = np.concatenate([centre - half, centre + half], axis=1)
        cat[:] = 2
    elif kind == 'one_category':
        cat[:] = 3
    elif kind == 'all_different':
        cat = rng.permutation(n) + 1
        bx = _boxes(rng, n, 100.0, 150.0, 200.0)         # heavy overlap that only counts without by_category
    elif kind == 'pile':
        base = np.array([100.0, 120.0, 260.0, 300.0])
        bx = base[None] + rng.uniform(-3.0, 3.0, (n, 4))
        cat[:] = 1
    elif kind == 'grid':
        i = np.arange(n)
        x0, y0 = 30.0 * (i % 12), 30.0 * (i // 12)
        bx = np.stack([x0, y0, x0 + rng.uniform(10.0, 29.0, n), y0 + rng.uniform(10.0, 29.0, n)], axis=1)
    elif kind != 'random':
        raise KeyError(kind)
    return cat.astype(np.int64), sc.astype(np.float32), bx.astype(np.float32)


def iou64(p, q):
    """IoU of two (x0, y0, x1, y1) boxes in float64 (Python floats)."""
    p, q = [float(v) for v in p], [float(v) for v in q]
    area_p = max(0.0, p[2] - p[0]) * max(0.0, p[3] - p[1])
    area_q = max(0.0, q[2] - q[0]) * max(0.0, q[3] - q[1])
    inter = max(0.0, min(p[2], q[2]) - max(p[0], q[0])) * max(0.0, min(p[3], q[3]) - max(p[1], q[1]))
    return inter / max(area_p + area_q - inter, 1e-12)


def iou_matrix(bx):
    """The same for all pairs at once (float64 numpy), [n, n]."""
    b = np.asarray(bx, dtype=np.float64)
    area = np.maximum(0.0, b[:, 2] - b[:, 0]) * np.maximum(0.0, b[:, 3] - b[:, 1])
    w = np.maximum(0.0, np.minimum(b[:, None, 2], b[None, :, 2]) - np.maximum(b[:, None, 0], b[None, :, 0]))
    h = np.maximum(0.0, np.minimum(b[:, None, 3], b[None, :, 3]) - np.maximum(b[:, None, 1], b[None, :, 1]))
    inter = w * h
    return inter / np.maximum(area[:, None] + area[None, :] - inter, 1e-12)


def may_suppress(cat, by_category):
    """[n, n] bool: pairs of DISTINCT candidates that can suppress each other."""
    n = len(cat)
    pairs = ~np.eye(n, dtype=bool)
    if by_category:
        pairs &= cat[:, None] == cat[None, :]
    return pairs


def margin(cat, bx, by_category, iou_threshold):
    """min |IoU - iou_threshold| over the pairs that may suppress each other (inf when there is none)."""
    pairs = may_suppress(cat, by_category)
    if not pairs.any():
        return float('inf')
    return float(np.abs(iou_matrix(bx) - iou_threshold)[pairs].min())


def brute_force(cat, sc, bx, *, iou_threshold, suppression, instance_threshold, by_category):
    """Greedy NMS written from its definition, float64 IoU, one pair at a time -> (kept [n] bool, survivors as
    (categories, scores float32, boxes float32 x y w h) in candidate order).  Score and box arithmetic is float32, as in the
    reference's arrays."""
    n = len(sc)
    order = sorted(range(n), key=lambda i: (-float(sc[i]), i))               # stable, descending
    iou = iou_matrix(bx) if n > 200 else None                                # (the pairwise loop is O(n^2) Python calls)
    alive, kept = [True] * n, np.zeros(n, dtype=bool)
    for i in order:
        if not alive[i]:
            continue
        kept[i] = True
        for j in range(n):
            if j == i or not alive[j] or (by_category and cat[i] != cat[j]):
                continue
            v = iou[i, j] if iou is not None else iou64(bx[i], bx[j])
            if v > iou_threshold:
                alive[j] = False
    new = np.where(kept, sc, sc * np.float32(suppression)).astype(np.float32)
    mask = new > np.float32(instance_threshold)
    xywh = np.concatenate([bx[:, :2], bx[:, 2:] - bx[:, :2]], axis=1).astype(np.float32)
    return kept, (cat[mask], new[mask], xywh[mask].reshape(-1, 4))


def post_model(**post):
    """A ``decoder.CifDet`` that can run ``_post`` without a device (its constructor builds a native decoder)."""
    from openpifpaf_amd import decoder, headmeta
    dec = object.__new__(decoder.CifDet)
    dec.metas = [headmeta.CifDet('cifdet', 'synthetic', categories=['c%d' % i for i in range(2048)])]
    dec.iou_threshold, dec.suppression = post['iou_threshold'], post['suppression']
    dec.instance_threshold, dec.nms_by_category = post['instance_threshold'], post['by_category']
    return dec


def post_arrays(cat, sc, bx, **post):
    """``decoder.CifDet._post`` -> (categories int64 [m], scores float32 [m], boxes float32 [m,4] x y w h)."""
    anns = post_model(**post)._post(cat, sc, bx)
    return (np.asarray([a.category_id for a in anns], dtype=np.int64),
            np.asarray([a.score for a in anns], dtype=np.float32),
            np.asarray([a.bbox for a in anns], dtype=np.float32).reshape(-1, 4))


def same_bits(got, want):
    """Count, order, categories and the bits of scores and boxes."""
    return (len(got[0]) == len(want[0]) and np.array_equal(np.asarray(got[0], dtype=np.int64), want[0])
            and np.array_equal(np.asarray(got[1], dtype=np.float32).view(np.uint32), want[1].view(np.uint32))
            and np.array_equal(np.asarray(got[2], dtype=np.float32).reshape(-1, 4).view(np.uint32), want[2].view(np.uint32)))
