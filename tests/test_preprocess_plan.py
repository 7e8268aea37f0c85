"""Host side of the preprocessing kernels (``csrc/preprocess.hip``): the plan ``preprocess_batch_device`` hands to
``opa_preprocess_u8`` -- geometry, metas, coefficient tables, offsets -- the 32-bit accumulator the kernels use, the
normalisation look-up table, the C ABI's bookkeeping and its argument checks, and the CLI switch.  No GPU is touched."""
import argparse
import ctypes
import os
import re

import numpy as np
import pytest

from openpifpaf_amd import _lib, predictor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(60, 80), (40, 30), (300, 180), (33, 400), (400, 25), (97, 97), (97, 60), (22, 28)]          # (h0, w0)
TARGETS = [(97, 72), (72, 97), (58, 97), (97, 8), (6, 97), (97, 97), (60, 97), (97, 76)]               # (tw, th) at long edge 97
RESIZES = [((2, 2), (7, 5)), ((37, 53), (37, 53)), ((48, 64), (48, 97)), ((150, 90), (97, 58)), ((33, 400), (8, 97)),
           ((9, 300), (3, 97)), ((131, 131), (97, 97))]                                                # ((h0, w0), (th, tw))


def frame(h, w, seed=0):
    return np.random.default_rng(1000 * h + w + seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def same_meta(a, b):
    assert set(a) == set(b)
    for key in ('offset', 'scale', 'valid_area', 'width_height'):
        assert np.array_equal(a[key], b[key]), (key, a[key], b[key])
    assert a['hflip'] == b['hflip'] and a['rotation'] == b['rotation']


@pytest.mark.parametrize('long_edge,batch_mode', [(97, True), (97, False), (None, False)])
def test_plan_geometry_and_metas_equal_preprocess_image(long_edge, batch_mode):
    for i, (h0, w0) in enumerate(SIZES):
        plan = predictor.preprocess_plan([(h0, w0)], long_edge=long_edge, batch_mode=batch_mode, fast=True)
        want, wmeta = predictor.preprocess_image(frame(h0, w0), long_edge=long_edge, batch_mode=batch_mode)
        assert plan['canvas'] == tuple(want.shape[1:])
        tw, th, left, top = plan['geometry'][0]
        if long_edge:
            assert (tw, th) == TARGETS[i]
        else:
            assert (tw, th) == (w0, h0) and plan['canvas'] == (-(-(h0 - 1) // 16) * 16 + 1, -(-(w0 - 1) // 16) * 16 + 1)
        assert (left, top) == (int((plan['canvas'][1] - tw) / 2.0), int((plan['canvas'][0] - th) / 2.0))
        same_meta(plan['metas'][0], wmeta)
        d = plan['images'][0]
        assert (d['h0'], d['w0'], d['th'], d['tw'], d['top'], d['left']) == (h0, w0, th, tw, top, left)


def test_plan_packs_a_mixed_batch():
    plan = predictor.preprocess_plan(SIZES, long_edge=97, batch_mode=True, fast=True)
    assert plan['canvas'] == (97, 97) and [g[:2] for g in plan['geometry']] == TARGETS
    images, src, mid = plan['images'], 0, 0
    for d, (h0, w0) in zip(images, SIZES):
        assert d['src_offset'] == src                                    # frames are packed without gaps
        src += h0 * w0 * 3
        for table, ksize, n_in, n_out in ((d['x_table'], d['x_ksize'], w0, d['tw']), (d['y_table'], d['y_ksize'], h0, d['th'])):
            first, fixed = predictor._pil_bilinear_coeffs(n_in, n_out)
            assert table % 4 == 0 and ksize == fixed.shape[1] >= 1
            got = plan['tables'][table:table + (1 + ksize) * n_out].reshape(1 + ksize, n_out)
            assert np.array_equal(got[0], first) and np.array_equal(got[1:], fixed.T)
        if d['tw'] != w0:
            assert d['mid_offset'] == mid and mid % 256 == 0
            mid += -(-h0 * (-(-3 * d['tw'] // 16) * 16) // 256) * 256
    assert plan['frames_bytes'] == -(-src // 16) * 16 and plan['workspace_bytes'] == mid
    assert plan['tables'].dtype == np.int32
    assert sorted({int(d['x_ksize']) for d in images} | {int(d['y_ksize']) for d in images}) == [3, 9, 11]
    # the library's own size of the intermediate agrees (no device: a host computation)
    ptr = images.ctypes.data_as(ctypes.POINTER(_lib.PreImage))
    assert _lib.lib().opa_preprocess_workspace_bytes(ptr, len(images), 0) == mid
    assert _lib.lib().opa_preprocess_workspace_bytes(ptr, len(images), 1) == 0
    precise = predictor.preprocess_plan(SIZES, long_edge=97, batch_mode=True, fast=False)
    assert precise['workspace_bytes'] == 0 and precise['geometry'] == plan['geometry']
    assert all(d['x_ksize'] == 2 and d['y_ksize'] == 2 and d['x_table'] % 4 == 0 for d in precise['images'])


def resample_int32(img, table, ksize, n_out, axis):
    """One pass of the kernels in numpy with an int32 accumulator: start at 2^21, shift right by 22, clamp, uint8."""
    tab = table[:(1 + ksize) * n_out].reshape(1 + ksize, n_out)
    n_in = img.shape[axis]
    shape = [1, 1, 1]
    shape[axis] = n_out
    acc = np.full([n_out if a == axis else img.shape[a] for a in range(3)], 1 << 21, dtype=np.int32)
    with np.errstate(over='raise'):
        for k in range(ksize):
            idx = np.minimum(tab[0] + k, n_in - 1)
            acc = acc + np.take(img, idx, axis=axis).astype(np.int32) * tab[1 + k].reshape(shape)
    assert acc.dtype == np.int32
    return np.clip(acc >> 22, 0, 255).astype(np.uint8)


def run_plan_int32(img, d, tables):
    if d['tw'] != d['w0']:
        img = resample_int32(img, tables[d['x_table']:], int(d['x_ksize']), int(d['tw']), 1)
    if d['th'] != d['h0']:
        img = resample_int32(img, tables[d['y_table']:], int(d['y_ksize']), int(d['th']), 0)
    return img


def test_int32_accumulator_equals_pillow():
    import PIL.Image
    bilinear = getattr(PIL.Image, 'Resampling', PIL.Image).BILINEAR
    cases = [((h0, w0), (th, tw)) for (h0, w0), (tw, th) in zip(SIZES, TARGETS)] + RESIZES
    ksizes = set()
    for (h0, w0), (th, tw) in cases:
        img = frame(h0, w0)
        xt, xk = predictor._axis_table(w0, tw, True)
        yt, yk = predictor._axis_table(h0, th, True)
        tables = np.concatenate([xt, yt])
        d = {'h0': h0, 'w0': w0, 'th': th, 'tw': tw, 'x_table': 0, 'x_ksize': xk, 'y_table': len(xt), 'y_ksize': yk}
        ksizes |= {xk, yk}
        got = run_plan_int32(img, d, tables)
        want = np.asarray(PIL.Image.fromarray(img).resize((tw, th), bilinear))
        assert np.array_equal(got, want), ((h0, w0), (th, tw), int((got != want).sum()))
        # the weights are non-negative and sum to about 2^22, so 255 * sum + 2^21 stays below 2^31
        for t, k, n in ((xt, xk, tw), (yt, yk, th)):
            w = t[:(1 + k) * n].reshape(1 + k, n)[1:].astype(np.int64)
            assert w.min() >= 0 and 255 * w.sum(axis=0).max() + (1 << 21) < 2 ** 31
    assert {3, 5, 7, 9, 11} <= ksizes
    # extreme values: an all-255 and an all-0 frame stay 255 and 0
    for value in (255, 0):
        img = np.full((33, 400, 3), value, np.uint8)
        xt, xk = predictor._axis_table(400, 97, True)
        assert np.all(resample_int32(img, xt, xk, 97, 1) == value)


def test_zoom_tables_equal_the_model():
    import torch
    for n_in, n_out in ((22, 76), (28, 97), (400, 97), (25, 6), (97, 97), (5, 1)):
        words, ksize = predictor._axis_table(n_in, n_out, False)
        assert ksize == 2 and len(words) % 4 == 0
        ints, dbl = words[:3 * n_out].reshape(3, n_out), words[(3 * n_out + 1) // 2 * 2:][:4 * n_out].view(np.float64).reshape(2, n_out)
        zoom = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0           # zoom_linear_u8.axis, in torch
        cc = torch.arange(n_out, dtype=torch.float64) * zoom
        start = torch.floor(cc)
        i0 = start.to(torch.int64).clamp_(0, n_in - 1)
        assert np.array_equal(ints[0], i0.numpy()) and np.array_equal(ints[1], (i0 + 1).clamp_(max=n_in - 1).numpy())
        assert np.array_equal(ints[2], (cc > (n_in - 1)).numpy())
        assert np.array_equal(dbl[0], (1.0 - (cc - start)).numpy()) and np.array_equal(dbl[1], (1.0 - ((start + 1.0) - cc)).numpy())
    # (22, 28) at long edge 97: the zoom's last row is rounded past the edge
    assert predictor._axis_table(22, 76, False)[0][2 * 76:3 * 76][-1] == 1


def test_normalisation_lut_is_the_host_expression():
    lut = predictor.normalisation_lut()
    assert lut.shape == (3, 256) and lut.dtype == np.float32
    x = np.asarray(np.arange(256, dtype=np.uint8).reshape(1, 256, 1).repeat(3, axis=2), dtype=np.float32) / 255.0
    x = (x - predictor.IMAGENET_MEAN) / predictor.IMAGENET_STD           # preprocess_image's two lines
    want = x.transpose(2, 0, 1)[:, 0, :]
    assert np.array_equal(lut.view(np.uint32), want.view(np.uint32))     # all 768 entries, bit for bit


def test_header_ctypes_and_abi_version():
    text = open(os.path.join(ROOT, 'include', 'openpifpaf_amd.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in ('opa_preprocess_u8', 'opa_preprocess_workspace_bytes', 'opa_pre_image_bytes'):
        assert re.search(r'\b%s\s*\(' % name, code) and name in _lib.SYMBOLS
    body = re.search(r'typedef struct opa_pre_image \{(.*?)\} opa_pre_image;', code, flags=re.S).group(1)
    ctype = {'int64_t': ctypes.c_int64, 'int32_t': ctypes.c_int32}
    fields = []
    for kind, names in re.findall(r'(int64_t|int32_t)\s+([^;]+);', body):
        fields += [(n.strip(), ctype[kind]) for n in names.split(',')]
    assert fields == list(_lib.PreImage._fields_)
    assert ctypes.sizeof(_lib.PreImage) == 56 == _lib.lib().opa_pre_image_bytes() == np.dtype(_lib.PreImage).itemsize
    assert re.search(r'#define OPA_ABI_VERSION 9\b', text)
    assert _lib.lib().opa_abi_version() == 9 == _lib.ABI_VERSION


def call_preprocess(images, **change):
    """``opa_preprocess_u8`` with pointers that are never read (validation comes before any device use)."""
    fake = 4096
    arr = (_lib.PreImage * max(len(images), 1))(*images)
    args = dict(images_host=arr, images_dev=fake, batch=len(images), frames_dev=fake, frames_bytes=1 << 20, tables_dev=fake,
                tables_words=1 << 16, workspace_dev=fake, workspace_bytes=1 << 20, lut_dev=fake, out_dev=fake, canvas_h=97,
                canvas_w=97, mode=0, channels_last=0, fill=0, stream=None)
    args.update(change)
    rc = _lib.lib().opa_preprocess_u8(*args.values())
    return rc, _lib.lib().opa_last_error().decode()


def good_image(**change):
    fields = dict(src_offset=0, mid_offset=0, h0=60, w0=80, th=72, tw=97, top=12, left=0, x_table=0, x_ksize=3, y_table=400, y_ksize=3)
    fields.update(change)
    return _lib.PreImage(**fields)


@pytest.mark.parametrize('image,change,named', [
    ({}, {'images_host': None}, 'images_host'), ({}, {'images_dev': None}, 'images_dev'),
    ({}, {'frames_dev': None}, 'frames_dev'), ({}, {'tables_dev': None}, 'tables_dev'),
    ({}, {'workspace_dev': None}, 'workspace_dev'), ({}, {'lut_dev': None}, 'lut_dev'), ({}, {'out_dev': None}, 'out_dev'),
    ({}, {'batch': 0}, 'batch'), ({}, {'batch': -3}, 'batch'),
    ({'th': 0}, {}, 'images[1].th'), ({'tw': 0}, {}, 'images[1].tw'), ({'h0': 0}, {}, 'images[1].h0'), ({'w0': -1}, {}, 'images[1].w0'),
    ({'top': 26}, {}, 'images[1].top'), ({'left': 1}, {}, 'images[1].top / left'), ({'top': -1}, {}, 'placement'),
    ({'x_ksize': 0}, {}, 'images[1].x_ksize'), ({'y_ksize': 0}, {}, 'images[1].y_ksize'),
    ({'src_offset': 1 << 20}, {}, 'images[1].src_offset'), ({'x_table': 1 << 16}, {}, 'images[1].x_table'),
    ({'y_table': 2}, {}, 'images[1].y_table'), ({'mid_offset': 8}, {}, 'images[1].mid_offset'),
    ({}, {'canvas_h': 0}, 'canvas_h'), ({}, {'canvas_w': 0}, 'canvas_w'), ({}, {'mode': 2}, 'mode'),
    ({}, {'frames_bytes': 100}, 'frames_bytes'), ({}, {'frames_dev': 4100}, '16-B aligned'),
    ({'w0': 40000, 'src_offset': 0, 'h0': 1}, {'frames_bytes': 1 << 24}, 'LDS'),
])
def test_invalid_arguments_are_refused_before_any_device_use(image, change, named):
    rc, text = call_preprocess([good_image(), good_image(**image)], **change)
    assert rc == 1 and _lib.ERROR_NAMES[rc] == 'INVALID_ARGUMENT'
    assert text.startswith('opa_preprocess_u8: ') and named in text, text


def test_small_workspace_is_refused():
    rc, text = call_preprocess([good_image()], workspace_bytes=1024)
    assert _lib.ERROR_NAMES[rc] == 'WORKSPACE' and 'workspace_bytes' in text
    assert _lib.lib().opa_preprocess_workspace_bytes(None, 1, 0) == 0 and b'images_host' in _lib.lib().opa_last_error()
    assert _lib.lib().opa_preprocess_workspace_bytes((_lib.PreImage * 1)(good_image(tw=0)), 1, 0) == 0
    assert b'images[0].tw' in _lib.lib().opa_last_error()


def test_a_target_side_of_zero_raises():
    assert predictor._target_size(3, 2000, 97) == (0, 97)
    with pytest.raises(ValueError, match='0 pixels'):
        predictor.preprocess_plan([(2000, 3)], long_edge=97, batch_mode=True)
    with pytest.raises(ValueError, match='0 pixels'):
        predictor.preprocess_plan([(3, 2000)], long_edge=97, batch_mode=False, fast=False)
    with pytest.raises(ValueError, match='one canvas'):
        predictor.preprocess_plan([(60, 80), (40, 30)], long_edge=97, batch_mode=False)


def test_cli_switch_sets_and_resets_the_class_attribute():
    from openpifpaf_amd import Predictor
    assert Predictor.device_preprocess is False
    parser = argparse.ArgumentParser()
    Predictor.cli(parser)
    before = (Predictor.batch_size, Predictor.long_edge, Predictor.fast_rescaling, Predictor.base_name)
    try:
        assert parser.parse_args([]).device_preprocess is False
        args = parser.parse_args(['--device-preprocess', '--long-edge', '97', '--batch-size', '2'])
        assert args.device_preprocess is True
        Predictor.configure(args)
        assert Predictor.device_preprocess is True
        Predictor.configure(parser.parse_args([]))
        assert Predictor.device_preprocess is False
        Predictor.device_preprocess = True                               # an argument set without the switch leaves it alone
        Predictor.configure(argparse.Namespace(batch_size=1, long_edge=None))
        assert Predictor.device_preprocess is True
    finally:
        Predictor.device_preprocess = False
        Predictor.batch_size, Predictor.long_edge, Predictor.fast_rescaling, Predictor.base_name = before
