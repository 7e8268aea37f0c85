"""CifDet NMS, score filter and box conversion on the device (csrc/cifdet.hip: cifdet_nms_kernel) against
``decoder.CifDet._post``, which tests/test_cifdet_nms_cases.py pins to a float64 brute-force model on the same cases: count,
order, categories and the BITS of scores and boxes (the arithmetic is the same float32 / float64 operations: tolerance zero).
Then every layer above the kernel: the combined native call, ``decoder.CifDet`` without its host loop, the setting above the
kernel's capacity, the decode lanes, ``Predictor``, the TorchScript class and a captured graph."""
import numpy as np
import pytest

import cifdet_nms_common as cn

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

SENTINEL_CAT, SENTINEL = -7, -3.5


def capacity(n):
    """The reference's 120 candidates where the case fits; else exactly the case (121: 256 threads; 300, 1024: 1024 threads)."""
    return 120 if n <= 120 else n


def batch_of(case):
    """Three images: the case, an empty image, the case again -> padded arrays + counts."""
    cat, sc, bx = cn.candidates(case)
    n, M = len(sc), capacity(len(sc))
    rng = np.random.default_rng(1)
    cats = rng.integers(1, 5, (3, M)).astype(np.int64)              # (rows behind counts[b] hold other candidates: never read)
    scs = rng.uniform(0.2, 1.0, (3, M)).astype(np.float32)
    bxs = rng.uniform(0.0, 300.0, (3, M, 4)).astype(np.float32)
    for b in (0, 2):
        cats[b, :n], scs[b, :n], bxs[b, :n] = cat, sc, bx
    return (cat, sc, bx), (cats, scs, bxs, np.array([n, 0, n], dtype=np.int32))


def sentinels(B, M):
    return (torch.full((B, M), SENTINEL_CAT, dtype=torch.int64, device='cuda'),
            torch.full((B, M), SENTINEL, dtype=torch.float32, device='cuda'),
            torch.full((B, M, 4), SENTINEL, dtype=torch.float32, device='cuda'),
            torch.full((B,), -1, dtype=torch.int32, device='cuda'))


def rows(anns):
    return [(a.category_id, np.float32(a.score).tobytes(), np.asarray(a.bbox, dtype=np.float32).tobytes()) for a in anns]


def as_arrays(anns):
    return (np.asarray([a.category_id for a in anns], dtype=np.int64), np.asarray([a.score for a in anns], dtype=np.float32),
            np.asarray([a.bbox for a in anns], dtype=np.float32).reshape(-1, 4))


@pytest.mark.parametrize('case', cn.CASES, ids=[c[0] for c in cn.CASES])
def test_kernel_equals_post(case):
    from openpifpaf_amd import native
    post = cn.settings(case)
    (cat, sc, bx), (cats, scs, bxs, counts) = batch_of(case)
    want = cn.post_arrays(cat, sc, bx, **post)
    B, M = cats.shape
    dev = [torch.from_numpy(a).cuda() for a in (cats, scs, bxs, counts)]
    out = sentinels(B, M)
    det = native.CifDet()
    got = det.nms(*dev, out=out, **post)
    torch.cuda.synchronize()
    assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
    ocat, osc, obx, ocnt = (t.cpu().numpy() for t in got)
    print('%s: n = %d, capacity %d, survivors %d (want %d)' % (case[0], len(sc), M, int(ocnt[0]), len(want[0])))
    assert ocnt.tolist() == [len(want[0]), 0, len(want[0])]
    for b in range(3):
        m = int(ocnt[b])
        assert cn.same_bits((ocat[b, :m], osc[b, :m], obx[b, :m]), want if b != 1 else tuple(w[:0] for w in want)), (case[0], b)
        # the tails are untouched
        assert (ocat[b, m:] == SENTINEL_CAT).all() and (osc[b, m:] == SENTINEL).all() and (obx[b, m:] == SENTINEL).all()
    # the inputs were only read
    assert all(np.array_equal(t.cpu().numpy(), a) for t, a in zip(dev, (cats, scs, bxs, counts)))
    # in place (what the combined call does): the same survivors, the rows behind them keep the candidates
    same = det.nms(*dev, out=tuple(dev), **post)
    torch.cuda.synchronize()
    icat, isc, ibx, icnt = (t.cpu().numpy() for t in same)
    assert icnt.tolist() == ocnt.tolist()
    for b in range(3):
        m = int(icnt[b])
        assert np.array_equal(icat[b, :m], ocat[b, :m]) and np.array_equal(isc[b, :m], osc[b, :m]) and np.array_equal(ibx[b, :m], obx[b, :m])
        assert np.array_equal(isc[b, m:], scs[b, m:]) and np.array_equal(ibx[b, m:], bxs[b, m:])


def det_fields(n_images=6, seed0=50):
    from openpifpaf_amd import synth
    return np.stack([synth.synth_det_field(seed0 + b, 3 + 5 * b) for b in range(n_images)])


def oracle_post(fields, max_detections=120, **post):
    """Per image: ``_post`` of the oracle's candidates -> lists of AnnotationDet."""
    from oracle import port
    model = cn.post_model(**post)
    return [model._post(*port.cifdet_decode(f, 8, max_detections=max_detections)) for f in fields]


@pytest.mark.parametrize('post', [cn.DEFAULTS, dict(iou_threshold=0.3, suppression=0.5, instance_threshold=0.3, by_category=False)],
                         ids=['defaults', 'other'])
def test_call_batch_nms_equals_post_of_the_oracle_candidates(post):
    from openpifpaf_amd import native
    fields = det_fields()
    want = oracle_post(fields, **post)
    cat, sc, bx, cnt = native.CifDet().call_batch_nms(torch.from_numpy(fields).cuda(), 8, **post)
    torch.cuda.synchronize()
    cat, sc, bx, cnt = cat.cpu().numpy(), sc.cpu().numpy(), bx.cpu().numpy(), cnt.cpu().numpy()
    assert sum(len(w) for w in want) > 6
    for b in range(len(fields)):
        m = int(cnt[b])
        assert cn.same_bits((cat[b, :m], sc[b, :m], bx[b, :m]), as_arrays(want[b])), b
    # CPU tensors in, CPU tensors out
    got = native.CifDet().call_batch_nms(torch.from_numpy(fields[:2]), 8, **post)
    assert all(not t.is_cuda for t in got) and got[3].tolist() == cnt[:2].tolist()


def det_decoder():
    from openpifpaf_amd import decoder, headmeta
    meta = headmeta.CifDet('cifdet', 'synthetic', categories=['c%d' % i for i in range(8)])
    meta.head_index, meta.base_stride, meta.upsample_stride = 0, 16, 2
    return decoder.CifDet.factory([meta])[0]


def test_decoder_runs_without_the_host_loop(monkeypatch):
    from openpifpaf_amd import decoder
    fields = det_fields()
    want = oracle_post(fields, **cn.DEFAULTS)

    def no_host_loop(self, *args):
        raise AssertionError('_post was called')
    monkeypatch.setattr(decoder.CifDet, '_post', no_host_loop)
    dec = det_decoder()
    dev = torch.from_numpy(fields).cuda()
    got = dec.batch(lambda images: (dev,), torch.zeros((6, 3, 8, 8)), device=torch.device('cuda'))
    assert len(got) == 6 and [rows(g) for g in got] == [rows(w) for w in want]
    assert all(a.category == 'c%d' % (a.category_id - 1) for g in got for a in g)
    assert dec.last_decoder_time > 0
    for b in (0, 3, 5):                                                   # one image, device and host tensors
        assert rows(dec([dev[b]])) == rows(want[b])
    assert rows(dec([torch.from_numpy(fields[2])])) == rows(want[2])
    # the class's settings reach the kernel
    other = dict(iou_threshold=0.3, suppression=0.5, instance_threshold=0.3, by_category=False)
    monkeypatch.undo()
    want_other = oracle_post(fields, **other)
    monkeypatch.setattr(decoder.CifDet, '_post', no_host_loop)
    dec.iou_threshold, dec.suppression, dec.instance_threshold, dec.nms_by_category = 0.3, 0.5, 0.3, False
    got = dec.batch(lambda images: (dev,), torch.zeros((6, 3, 8, 8)), device=torch.device('cuda'))
    assert [rows(g) for g in got] == [rows(w) for w in want_other] and [rows(w) for w in want_other] != [rows(w) for w in want]


def test_above_the_kernel_capacity_the_host_post_processes(monkeypatch):
    from openpifpaf_amd import _lib, decoder, native
    fields = det_fields()
    dev = torch.from_numpy(fields).cuda()
    dec = det_decoder()
    at_120 = dec.batch(lambda images: (dev,), torch.zeros((6, 3, 8, 8)), device=torch.device('cuda'))
    old = native.CifDet.get_max_detections_before_nms()
    calls = []
    original = decoder.CifDet._post

    def counting(self, *args):
        calls.append(len(args[1]))
        return original(self, *args)
    try:
        native.CifDet.set_max_detections_before_nms(2000)
        with pytest.raises(_lib.NativeError, match='INVALID_ARGUMENT.*OPA_CIFDET_NMS_MAX'):
            native.CifDet().call_batch_nms(dev, 8)
        cat = torch.ones((1, 2000), dtype=torch.int64, device='cuda')
        with pytest.raises(_lib.NativeError, match='INVALID_ARGUMENT'):
            native.CifDet().nms(cat, torch.ones((1, 2000), device='cuda'), torch.ones((1, 2000, 4), device='cuda'),
                                torch.ones((1,), dtype=torch.int32, device='cuda'))
        torch.cuda.synchronize()                                          # (nothing was queued: nothing to fail here)
        want = oracle_post(fields, max_detections=2000, **cn.DEFAULTS)
        monkeypatch.setattr(decoder.CifDet, '_post', counting)
        got = dec.batch(lambda images: (dev,), torch.zeros((6, 3, 8, 8)), device=torch.device('cuda'))
        assert len(calls) == 6
        assert [rows(g) for g in got] == [rows(w) for w in want]
        assert rows(dec([dev[4]])) == rows(want[4]) and len(calls) == 7
        ticket = dec.batch_async(lambda images: (dev,), torch.zeros((6, 3, 8, 8)), device=torch.device('cuda'))
        assert ticket.done() and [rows(g) for g in ticket.result()] == [rows(w) for w in want] and len(calls) == 13
        if max(calls) < 120:                                              # no image reached the reference's cap: the same detections
            assert [rows(g) for g in got] == [rows(g) for g in at_120]
    finally:
        native.CifDet.set_max_detections_before_nms(old)
    assert native.CifDet.get_max_detections_before_nms() == 120


def test_batch_async_equals_batch_in_any_collection_order(monkeypatch):
    from openpifpaf_amd import decoder
    batches = [det_fields(3, 300 + 10 * i) for i in range(5)]

    class FieldModel:                       # emits the field batch the images name (their first value)
        def __call__(self, images):
            return (torch.from_numpy(batches[int(images[0, 0, 0, 0].item())]).cuda(),)

    def images(i):
        return torch.full((3, 3, 16, 16), float(i))
    cuda = torch.device('cuda')
    old = decoder.CifDet.decoder_workers
    try:
        for workers in (1, 2, 3):
            decoder.CifDet.decoder_workers = workers
            dec = decoder.Multi([det_decoder()])
            assert dec.pipeline_depth == workers
            sync = [[rows(g) for g in dec.batch(FieldModel(), images(i), device=cuda)] for i in range(5)]
            for i in range(5):
                assert sync[i] == [rows(w) for w in oracle_post(batches[i], **cn.DEFAULTS)]
            pend, got = [], {}
            for i in range(5):                       # in flight: as many as there are lanes, collected oldest first
                if len(pend) >= workers:
                    j, p = pend.pop(0)
                    got[j] = [rows(g) for g in p.result()]
                pend.append((i, dec.batch_async(FieldModel(), images(i), device=cuda)))
            for j, p in reversed(pend):              # the rest, newest first
                got[j] = [rows(g) for g in p.result()]
            assert [got[i] for i in range(5)] == sync
            # a lane that is submitted to again before its batch was collected keeps that batch's result
            first = dec.batch_async(FieldModel(), images(0), device=cuda)
            later = [dec.batch_async(FieldModel(), images(1 + k), device=cuda) for k in range(workers)]
            assert [rows(g) for g in first.result()] == sync[0] and first.result() is first.result()
            for k, p in enumerate(later):
                assert [rows(g) for g in p.result()] == sync[1 + k]
            assert dec.last_decoder_time > 0
        # a ticket whose collection fails raises every time it is asked, is spent, and its lane takes the next batches
        inner = dec.decoders[0]
        build = inner._annotations_from_host

        def broken(host_views, n_images):
            raise RuntimeError('no annotations today')
        bad = [inner.batch_async(FieldModel(), images(i), device=cuda) for i in range(3)]       # one per lane
        monkeypatch.setattr(inner, '_annotations_from_host', broken)
        for t in bad:
            for _ in range(2):
                with pytest.raises(RuntimeError, match='no annotations today'):
                    t.result()
        assert not inner._lane_pending
        monkeypatch.setattr(inner, '_annotations_from_host', build)
        good = [inner.batch_async(FieldModel(), images(i), device=cuda) for i in range(4)]
        assert [[rows(g) for g in t.result()] for t in good] == sync[:4]
        with pytest.raises(RuntimeError, match='no annotations today'):
            bad[0].result()
        with pytest.raises(ValueError, match='inverse_transform'):
            inner.batch_async(FieldModel(), images(0), device=cuda, meta_batch=[{}] * 3)
    finally:
        decoder.CifDet.decoder_workers = old


def test_predictor_pipelines_a_cifdet_network():
    """A random-init network with a CifDet head through ``Predictor``, synchronously and pipelined over the decode lanes.  The
    fields of the synchronous run are recorded; in the pipelined run the network runs as always and the recorded fields are
    then copied into its output tensor on the network's stream, so both runs decode identical fields whatever the
    convolutions' reproducibility from call to call.  The pipelined run must equal the synchronous one for every image, bit for
    bit, and both must equal ``_post`` of the oracle's candidates for those fields, transformed back with the image's meta."""
    from openpifpaf_amd import Predictor, decoder, headmeta, network
    from oracle import port
    meta = headmeta.CifDet('cifdet', 'synthetic', categories=['c%d' % i for i in range(6)])
    meta.upsample_stride = 2
    net = network.factory('resnet18', [meta])
    with torch.no_grad():                                # boxes of about four cells instead of a random head's sizes around zero
        net.head_nets[0].conv.bias.view(6, 6, 4)[:, 4:6] += 4.0
    Predictor.long_edge, Predictor.batch_size = 161, 2
    try:
        pred = Predictor(model=net)
        assert isinstance(pred.processor.decoders[0], decoder.CifDet) and pred.processor.pipeline_depth >= 1
        rng = np.random.default_rng(6)
        images = [(rng.random((120 + 10 * k, 160, 3)) * 255).astype(np.uint8) for k in range(5)]
        recorded, replay, forward = [], [], pred._forward

        def recording(image_batch):
            heads = forward(image_batch)                 # (the network runs in both runs, on the current stream)
            if replay:
                heads[0].copy_(replay.pop(0))            # same stream, behind the network: the lane's wait covers it
            recorded.append(heads[0].clone())
            return heads
        pred._forward = recording

        def run(pipelined, fields=()):
            recorded.clear()
            replay[:] = list(fields)
            pred.pipelined = pipelined
            out = list(pred.numpy_images(images))
            assert not replay
            return out, list(recorded)
        run(False)                                       # (every shape once: kernel choices are made at a first call)
        want, want_fields = run(False)
        got, got_fields = run(True, want_fields)
        assert len(got) == len(want) == 5 and pred.total_images == 15
        assert len(got_fields) == len(want_fields) == 3 and all(torch.equal(a, b) for a, b in zip(got_fields, want_fields))
        fields = np.concatenate([f.cpu().numpy() for f in want_fields])
        assert fields.shape[:3] == (5, 6, 6)
        model = cn.post_model(**cn.DEFAULTS)
        model.metas = [meta]

        def key(anns):
            return [(a.category_id, a.score, np.asarray(a.bbox).tobytes()) for a in anns]
        n_boxes = 0
        for i, ((g, _, gm), (w, _, wm)) in enumerate(zip(got, want)):
            assert np.array_equal(gm['offset'], wm['offset']) and np.array_equal(gm['scale'], wm['scale'])
            assert key(g) == key(w), i                                           # pipelined == synchronous
            oracle = [a.inverse_transform(wm) for a in model._post(*port.cifdet_decode(fields[i], meta.stride))]
            assert key(w) == key(oracle), i                                      # == _post of the oracle's candidates
            n_boxes += len(w)
        print('predictor: %d detections in 5 images' % n_boxes)
        assert n_boxes > 0                               # (the random network finds something: the comparison is not empty)
    finally:
        Predictor.long_edge, Predictor.batch_size = None, 1


def test_torchscript_methods_equal_the_ctypes_mirror(tmp_path):
    from openpifpaf_amd import native, torchscript
    D = torchscript.load().CifDet
    post = (0.4, 0.3, 0.2, True)
    keys = dict(iou_threshold=0.4, suppression=0.3, instance_threshold=0.2, by_category=True)

    class Holder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.d = D()

        def forward(self, field):
            cat, sc, bx, cnt = self.d.call_batch(field, 8)
            return self.d.call_batch_nms(field, 8, 0.4, 0.3, 0.2, True), self.d.nms(cat, sc, bx, cnt, 0.4, 0.3, 0.2, True)
    fields = torch.from_numpy(det_fields(4, 70)).cuda()
    module = torch.jit.script(Holder())
    both, split = module(fields)
    ref = native.CifDet()
    want = ref.call_batch_nms(fields, 8, **keys)
    want_split = ref.nms(*ref.call_batch(fields, 8), **keys)
    torch.cuda.synchronize()
    n = want[3].cpu().tolist()
    assert sum(n) > 4 and both[3].cpu().tolist() == n == split[3].cpu().tolist() == want_split[3].cpu().tolist()
    for b in range(4):
        for got in (both, split, want_split):
            assert all(torch.equal(g[b, :n[b]], w[b, :n[b]]) for g, w in zip(got[:3], want[:3])), b
    direct = D().nms(*[t.cpu() for t in ref.call_batch(fields, 8)], *post)          # CPU tensors in, CPU tensors out
    assert all(not t.is_cuda for t in direct) and direct[3].tolist() == n


def test_captured_call_batch_nms_replays_equal_to_the_eager_run():
    from openpifpaf_amd import native
    det = native.CifDet()
    first, second = (torch.from_numpy(det_fields(4, seed)).cuda() for seed in (80, 90))
    eager = [tuple(t.clone() for t in det.call_batch_nms(f, 8)) for f in (first, second)]       # (and the workspace exists)
    torch.cuda.synchronize()
    static = first.clone()
    block, out = native.CifDet.output_block(4, 120, device=static.device)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        det.call_batch_nms(static, 8, out=out)
    for field, want in ((first, eager[0]), (second, eager[1]), (first, eager[0])):
        static.copy_(field)
        block.zero_()
        graph.replay()
        torch.cuda.synchronize()
        n = want[3].tolist()
        assert out[3].tolist() == n and sum(n) > 4
        for b in range(4):
            assert all(torch.equal(g[b, :n[b]], w[b, :n[b]]) for g, w in zip(out[:3], want[:3])), b


def test_captured_nms_at_the_largest_capacity_after_an_eager_first_call():
    """Above 64 KB of LDS the first call on a device raises the kernel's LDS limit and has to be eager (the header says so);
    from then on the kernel captures at that capacity too: 1024 candidates, the replay equal to the eager run."""
    from openpifpaf_amd import native
    case = [c for c in cn.CASES if c[0] == 'n1024'][0]
    _, arrays = batch_of(case)
    dev = [torch.from_numpy(a).cuda() for a in arrays]
    det = native.CifDet()
    eager = [t.clone() for t in det.nms(*dev, **cn.settings(case))]                # the eager first call
    torch.cuda.synchronize()
    out = sentinels(3, 1024)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        det.nms(*dev, out=out, **cn.settings(case))
    for _ in range(2):
        for t, fill in zip(out, (SENTINEL_CAT, SENTINEL, SENTINEL, -1)):
            t.fill_(fill)
        graph.replay()
        torch.cuda.synchronize()
        n = eager[3].tolist()
        assert out[3].tolist() == n and n[0] > 0 and n[1] == 0
        for b in range(3):
            assert all(torch.equal(g[b, :n[b]], w[b, :n[b]]) for g, w in zip(out[:3], eager[:3])), b
