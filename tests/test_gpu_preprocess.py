"""The preprocessing kernels (``csrc/preprocess.hip``) against the host path: ``preprocess_image`` is Pillow (``fast``) or
scipy's order-1 zoom (``fast=False``) itself, and the float32 batch the kernels write must EQUAL its output element for
element (``torch.equal``) -- both rescales, both memory formats, batch and single-image canvases."""
import numpy as np
import pytest
import torch

from openpifpaf_amd import predictor

pytestmark = pytest.mark.gpu

SIZES = [(60, 80), (40, 30), (300, 180), (33, 400), (400, 25), (97, 97), (97, 60), (22, 28)]          # (h0, w0)
_expected = {}


def frames_of(sizes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]


def expected(key, frames, **kwargs):
    """The host path's result, computed once per case and shared (never modified)."""
    if key not in _expected:
        items = [predictor.preprocess_image(f, **kwargs) for f in frames]
        _expected[key] = (torch.stack([t for t, _ in items]), [m for _, m in items])
    return _expected[key]


def check(frames, key, *, long_edge, fast, batch_mode=True, channels_last=False):
    got, metas = predictor.preprocess_batch_device(frames, long_edge=long_edge, device=torch.device('cuda'), fast=fast,
                                                   channels_last=channels_last, batch_mode=batch_mode)
    want, wmetas = expected((key, fast), frames, long_edge=long_edge, batch_mode=batch_mode, fast=fast)
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == want.shape
    host = got.cpu()
    for b in range(len(frames)):
        assert torch.equal(host[b], want[b]), 'image %d %s (fast=%s): %d values differ' % (
            b, frames[b].shape, fast, int((host[b] != want[b]).sum()))
    for m, w in zip(metas, wmetas):
        for name in ('offset', 'scale', 'valid_area', 'width_height'):
            assert np.array_equal(m[name], w[name])
    return got


@pytest.mark.parametrize('fast', [True, False])
def test_mixed_batch_equals_the_host_path(fast):
    """Upscale and downscale, both axes unchanged (97, 97), targets 6 and 8 pixels wide, source rows whose byte length is no
    multiple of 4 or 16, tap counts 3, 9 and 11, and (22, 28), whose zoom rounds its last row past the edge (zeros).  Frames
    with exactly ONE axis unchanged: ``test_one_axis_unchanged`` and ``test_vertical_pass_straight_from_the_frame``."""
    check(frames_of(SIZES, 11), 'mixed', long_edge=97, fast=fast)


@pytest.mark.parametrize('fast', [True, False])
def test_more_odd_sizes(fast):
    """Row lengths 3 * 53 and 3 * 131 bytes, a 2 x 2 frame, one axis upscaled only, a 9-row frame reduced to 3 rows."""
    check(frames_of([(37, 53), (131, 131), (2, 2), (48, 64), (9, 300), (150, 90)], 12), 'odd', long_edge=131, fast=fast)


@pytest.mark.parametrize('fast', [True, False])
def test_equal_frames_and_a_batch_of_one(fast):
    check(frames_of([(120, 160)] * 4, 13), 'equal', long_edge=193, fast=fast)
    check(frames_of([(120, 160)], 14), 'one', long_edge=193, fast=fast)


@pytest.mark.parametrize('fast', [True, False])
def test_canvas_and_target_wider_than_one_workgroup(fast):
    """A workgroup spans 256 columns (``kPreCols``).  ``long_edge = 321``: the canvas has two column chunks, the second of 65
    columns.  Targets: 321 wide (pass H and pass V both end with a 65-column chunk), 238 wide on columns 41..278 (begins in
    the first chunk, ends in the second), 161 wide on columns 80..240 (inside the first chunk: the second is all padding),
    and 321 wide again from a source wider than 256 pixels."""
    check(frames_of([(150, 250), (199, 148), (199, 100), (190, 259)], 15), 'wide', long_edge=321, fast=fast)


@pytest.mark.parametrize('fast', [True, False])
def test_channels_last_equals_nchw_and_is_not_copied_by_the_predictor(fast):
    frames = frames_of(SIZES, 11)
    nhwc = check(frames, 'mixed', long_edge=97, fast=fast, channels_last=True)
    assert nhwc.is_contiguous(memory_format=torch.channels_last) and nhwc.stride() == (3 * 97 * 97, 1, 3 * 97, 3)
    nchw = check(frames, 'mixed', long_edge=97, fast=fast)
    assert nchw.is_contiguous() and torch.equal(nhwc, nchw)
    assert nhwc.contiguous(memory_format=torch.channels_last).data_ptr() == nhwc.data_ptr()      # what Predictor._forward does


@pytest.mark.parametrize('fast', [True, False])
@pytest.mark.parametrize('size,long_edge,canvas', [((60, 80), 97, (81, 97)), ((150, 91), 97, (97, 65)),
                                                   ((60, 80), None, (65, 81)), ((150, 91), None, (161, 97))])
def test_single_image_canvas(size, long_edge, canvas, fast):
    got = check(frames_of([size], 16), ('single', size, long_edge), long_edge=long_edge, fast=fast, batch_mode=False)
    assert tuple(got.shape[2:]) == canvas


@pytest.mark.parametrize('channels_last', [False, True])
@pytest.mark.parametrize('fast', [True, False])
@pytest.mark.parametrize('sizes,long_edge', [([(96, 128), (128, 96), (97, 129), (129, 97)], 129), ([(480, 640), (640, 480)], 641)])
def test_one_axis_unchanged(sizes, long_edge, fast, channels_last):
    """``RescaleAbsolute`` truncates the short side, so the common frames keep one axis: 480 x 640 at 641 becomes 480 x 641.
    Landscape frames (96 x 128 -> 96 x 129, 480 x 640 -> 480 x 641): pass H, then pass V COPIES rows of the 16-B-pitched
    intermediate.  Portrait frames (128 x 96 -> 129 x 96, 640 x 480 -> 641 x 480): no pass H, pass V resamples vertically
    straight from the packed frame (rows of 3 * w0 bytes, every tap row with its own alignment).  In zoom mode the unchanged
    axis has zoom exactly 1.  (97, 129) and (129, 97) are the frames with both axes unchanged next to them."""
    for (h0, w0), (tw, th, _, _) in zip(sizes, predictor.preprocess_plan(sizes, long_edge=long_edge, batch_mode=True)['geometry']):
        assert (tw == w0) != (th == h0) or (h0, w0) in ((97, 129), (129, 97))
    got = check(frames_of(sizes, 17), ('one-axis', long_edge), long_edge=long_edge, fast=fast, channels_last=channels_last)
    assert got.is_contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)


def run_cases(frames, cases, canvas, fast, channels_last):
    """``opa_preprocess_u8`` on a hand-made plan: ``cases`` = (th, tw, top, left) per frame, any combination (the geometry
    ``preprocess_plan`` derives from a long edge never reduces one axis alone)."""
    from openpifpaf_amd import _lib
    images = np.zeros(len(frames), dtype=np.dtype(_lib.PreImage))
    tables, words, src, mid = [], 0, 0, 0
    for d, f, (th, tw, top, left) in zip(images, frames, cases):
        h0, w0 = f.shape[:2]
        d['h0'], d['w0'], d['th'], d['tw'], d['top'], d['left'], d['src_offset'] = h0, w0, th, tw, top, left, src
        src += f.size
        for name, n_in, n_out in (('x', w0, tw), ('y', h0, th)):
            t, ksize = predictor._axis_table(n_in, n_out, fast)
            d[name + '_table'], d[name + '_ksize'] = words, ksize
            tables.append(t)
            words += len(t)
        if fast and tw != w0:
            d['mid_offset'] = mid
            mid += -(-h0 * (-(-3 * tw // 16) * 16) // 256) * 256
    plan = {'canvas': canvas, 'images': images, 'tables': np.concatenate(tables), 'frames_bytes': -(-src // 16) * 16,
            'workspace_bytes': mid}
    return predictor._run_plan(frames, plan, device=torch.device('cuda'), fast=fast, channels_last=channels_last)


def host_cases(frames, cases, canvas, fast):
    """The same on the host: Pillow's resize (or the zoom ``preprocess_image`` calls), paste, ToTensor + Normalize as there."""
    import PIL.Image
    out = []
    for f, (th, tw, top, left) in zip(frames, cases):
        if fast:
            small = PIL.Image.fromarray(f).resize((tw, th), getattr(PIL.Image, 'Resampling', PIL.Image).BILINEAR)
        else:
            small = PIL.Image.fromarray(predictor.zoom_linear_u8(torch.from_numpy(f), th, tw).numpy())
        page = PIL.Image.new('RGB', (canvas[1], canvas[0]), predictor.FILL_RGB)
        page.paste(small, (left, top))
        x = np.asarray(page, dtype=np.float32) / 255.0
        x = (x - predictor.IMAGENET_MEAN) / predictor.IMAGENET_STD
        out.append(torch.from_numpy(np.ascontiguousarray(x.transpose(2, 0, 1))))
    return torch.stack(out)


@pytest.mark.parametrize('channels_last', [False, True])
@pytest.mark.parametrize('fast', [True, False])
def test_vertical_pass_straight_from_the_frame(fast, channels_last):
    """Width unchanged, height reduced, through the C entry with a hand-made plan: pass V resamples rows of the packed frame
    itself.  200 -> 40 rows and 131 -> 30 rows have 11 taps, so the second staging round of pass V (8 tap rows per round)
    runs, on rows of 159 and 231 bytes whose alignment changes from row to row; 300 x 259 -> 33 rows (21 taps, three rounds)
    is wider than one workgroup's 256 columns; 37 -> 80 rows is the upscale.  The last case reduces the width alone
    (pass H with 11 taps, then the copy out of the intermediate)."""
    frames = frames_of([(200, 53), (131, 77), (300, 259), (37, 53), (40, 300)], 18)
    cases = [(40, 53, 3, 100), (30, 77, 50, 0), (33, 259, 10, 1), (80, 53, 0, 207), (40, 60, 5, 30)]    # (th, tw, top, left)
    canvas = (83, 261)
    got = run_cases(frames, cases, canvas, fast, channels_last)
    want = host_cases(frames, cases, canvas, fast)
    assert got.shape == want.shape
    for b in range(len(frames)):
        assert torch.equal(got[b].cpu(), want[b]), 'case %d (fast=%s): %d values differ' % (b, fast, int((got[b].cpu() != want[b]).sum()))
    if fast:
        assert [int(k) for k in (predictor._axis_table(200, 40, True)[1], predictor._axis_table(300, 33, True)[1])] == [11, 21]


def test_back_to_back_batches_on_a_side_stream_keep_their_results():
    """Three different batches reuse the staging ring (two blocks) and the workspace; every result is read only after all
    three were queued."""
    batches = [(frames_of(SIZES, 21), 97), (frames_of([(120, 160), (150, 90), (61, 77)], 22), 193), (frames_of(SIZES[::-1], 23), 97)]
    stream = torch.cuda.Stream()
    results = []
    with torch.cuda.stream(stream):
        for fast in (True, False):
            for frames, long_edge in batches:
                results.append(predictor.preprocess_batch_device(frames, long_edge=long_edge, device=torch.device('cuda'),
                                                                 fast=fast)[0])
    stream.synchronize()
    i = 0
    for fast in (True, False):
        for n, (frames, long_edge) in enumerate(batches):
            want, _ = expected(('b2b', n, fast), frames, long_edge=long_edge, batch_mode=True, fast=fast)
            assert torch.equal(results[i].cpu(), want), (n, fast)
            i += 1


@pytest.mark.parametrize('fast', [True, False])
def test_launch_and_copy_counts_of_a_mixed_batch(fast):
    """At most two kernels -- pass H and pass V, or the zoom kernel alone -- and exactly one host-to-device copy per batch.
    Counting method: the kernels by the library's own launch counter (``opa_profile_begin`` / ``opa_profile_end``: one entry per
    operation the library queued on the stream; the library itself copies nothing); the copies by torch's host-side
    profiler, in which every transfer torch makes is one ``aten::copy_`` (filling the pinned block is numpy, no device
    transfer).  The device-to-host copy of the final comparison comes after the counted region."""
    from torch.profiler import ProfilerActivity, profile
    from openpifpaf_amd import _lib
    frames = frames_of(SIZES, 11)
    device = torch.device('cuda')
    for _ in range(2):                                                   # look-up table, workspace, staging ring, code objects
        predictor.preprocess_batch_device(frames, long_edge=97, device=device, fast=fast)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU]) as prof:
        _lib.profile_begin(torch.cuda.current_stream().cuda_stream)
        got, _ = predictor.preprocess_batch_device(frames, long_edge=97, device=device, fast=fast)
        launched = [name for name, _ in _lib.profile_end()]
    copies = [e for e in prof.events() if e.name == 'aten::copy_']
    print('launched:', launched, 'copies:', [(e.name, e.input_shapes) for e in copies])
    assert launched == (['preprocess_h_kernel', 'preprocess_v_kernel'] if fast else ['preprocess_zoom_kernel'])
    assert len(copies) == 1
    assert torch.equal(got.cpu(), expected(('mixed', fast), frames, long_edge=97, batch_mode=True, fast=fast)[0])


@pytest.mark.parametrize('batch_size', [2, 1])
def test_predictor_annotations_equal_the_host_preprocessing(batch_size):
    """Through the product: ``Predictor('resnet18')`` with ``device_preprocess`` on and off gives identical annotations, at
    batch size 2 (batch canvas) and 1 (single-image canvas)."""
    from openpifpaf_amd import Predictor
    rng = np.random.default_rng(1)
    images = [(rng.random((120, 160, 3)) * 255).astype(np.uint8), (rng.random((150, 90, 3)) * 255).astype(np.uint8)]
    results, fed = {}, {}
    for on_device in (True, False):
        Predictor.long_edge, Predictor.batch_size, Predictor.device_preprocess = 193, batch_size, on_device
        try:
            torch.manual_seed(7)                                         # the same randomly initialised network both times
            pred = Predictor('resnet18')
            fed[on_device] = []
            pred.model.register_forward_pre_hook(lambda module, args, store=fed[on_device]: store.append(args[0].clone()))
            results[on_device] = list(pred.numpy_images(images))
            assert len(results[on_device]) == 2 and pred.total_images == 2
        finally:
            Predictor.long_edge, Predictor.batch_size, Predictor.device_preprocess = None, 1, False
    # what the network was fed is the same tensor, batch for batch (the annotations of a randomly initialised network may
    # be few or none, so they alone would not show it)
    assert len(fed[True]) == len(fed[False]) == 2 // batch_size
    for x_d, x_h in zip(fed[True], fed[False]):
        assert x_d.shape == x_h.shape and torch.equal(x_d, x_h)
    for (pred_d, _, meta_d), (pred_h, _, meta_h) in zip(results[True], results[False]):
        assert np.array_equal(meta_d['offset'], meta_h['offset']) and np.array_equal(meta_d['scale'], meta_h['scale'])
        assert len(pred_d) == len(pred_h)
        for a_d, a_h in zip(pred_d, pred_h):
            assert np.array_equal(a_d.data, a_h.data)


def test_predictor_forward_takes_the_channels_last_batch_as_it_is():
    """``Predictor._preprocess`` asks for ``channels_last``; ``_forward``'s ``.contiguous(memory_format=...)`` is then a no-op:
    the model sees the very buffer the kernels wrote."""
    from openpifpaf_amd import Predictor
    frames = frames_of([(120, 160), (150, 90)], 31)
    seen = []

    class Model(torch.nn.Module):
        head_metas = None

        def forward(self, x):
            seen.append(x.data_ptr())
            return x

    Predictor.long_edge, Predictor.batch_size, Predictor.device_preprocess = 193, 2, True
    try:
        pred = Predictor.__new__(Predictor)
        pred.model = Model()
        assert pred.channels_last and pred.device.type == 'cuda'
        batch, _ = pred._preprocess(frames)
        torch.cuda.synchronize()
        assert batch.is_contiguous(memory_format=torch.channels_last)
        pred._forward(batch)
        assert seen == [batch.data_ptr()]
    finally:
        Predictor.long_edge, Predictor.batch_size, Predictor.device_preprocess = None, 1, False
