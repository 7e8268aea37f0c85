"""``preprocess_batch_device`` on the GPU, one batch of 32 frames per call: the kernels of ``csrc/preprocess.hip`` against the
torch-op model the branch keeps byte for byte (``predictor.preprocess_batch_torch``, the path before the kernels existed),
called on the same CUDA device in the same process.  The two alternate ``--windows`` times (3 at least); every timed window
follows a warm-up, holds ``--batches`` batches (20 at least) and ends in a device synchronise, the clock is the host's.

    python tools/gpu/preprocess_time.py [--windows 3] [--batches 20] [--warmup 3] [--precise] [--workload NAME ...]

``kernels_plan_rebuilt`` is the kernel path with its per-batch plan cache emptied before every call (batches whose sizes never
repeat; the timed batches themselves repeat their sizes, so ``kernels`` always finds its plan).
One JSON line per workload: milliseconds per batch of every window for every path, their medians, the baseline's spread
(max - min of its windows), whether the medians differ by more than that spread and whether every kernel window beat every
baseline window, whether the two outputs are equal, and the
bytes the kernels move, computed from the shapes (source + intermediate written and read + float32 output).
``--trace`` runs only the kernel path, ``--batches`` batches per workload between two markers on stdout, for a
``rocprofv3 --kernel-trace --stats`` run around it (kernel time, and with the bytes above the achieved bytes/s)."""
import argparse
import json
import os
import sys
import time

parser = argparse.ArgumentParser()
parser.add_argument('--package-root', default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
parser.add_argument('--images', type=int, default=32)
parser.add_argument('--long-edge', type=int, default=641)
parser.add_argument('--windows', type=int, default=3)
parser.add_argument('--batches', type=int, default=20, help='batches per timed window')
parser.add_argument('--warmup', type=int, default=3)
parser.add_argument('--precise', action='store_true', help="scipy's order-1 zoom instead of Pillow's bilinear resize")
parser.add_argument('--workload', nargs='+', default=['coco_480x640', 'video_1080x1920', 'mixed', 'square_641'])
parser.add_argument('--trace', action='store_true')
args = parser.parse_args()
assert args.trace or (args.windows >= 3 and args.batches >= 20), 'at least 3 alternations of at least 20 batches'
sys.path.insert(0, os.path.abspath(args.package_root))

import numpy as np      # noqa: E402
import torch            # noqa: E402

from openpifpaf_amd import predictor      # noqa: E402

assert torch.cuda.is_available(), 'this measurement needs the GPU'
device = torch.device('cuda')
fast = not args.precise


def workload(name):
    rng = np.random.default_rng(2024)
    if name == 'coco_480x640':
        sizes = [(480, 640)] * args.images
    elif name == 'video_1080x1920':
        sizes = [(1080, 1920)] * args.images
    elif name == 'square_641':
        sizes = [(args.long_edge, args.long_edge)] * args.images
    elif name == 'mixed':                              # COCO-like: long side 480..640, aspect ratio 0.5..1, either orientation
        sizes = []
        for _ in range(args.images):
            long_side = int(rng.integers(480, 641))
            short_side = int(long_side * rng.uniform(0.5, 1.0))
            sizes.append((long_side, short_side) if rng.random() < 0.3 else (short_side, long_side))
    else:
        raise SystemExit('unknown workload %r' % name)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]


def bytes_moved(frames):
    """What the kernels have to move, from the shapes: every source byte once, the horizontal pass' intermediate written
    and read once, the float32 canvas written once."""
    plan = predictor.preprocess_plan([f.shape[:2] for f in frames], long_edge=args.long_edge, batch_mode=True, fast=fast)
    source = sum(f.size for f in frames)
    mid = sum(int(d['h0']) * int(d['tw']) * 3 for d in plan['images'] if fast and d['tw'] != d['w0'])
    out = len(frames) * 3 * plan['canvas'][0] * plan['canvas'][1] * 4
    return {'source': source, 'intermediate_written': mid, 'intermediate_read': mid, 'output': out,
            'total': source + 2 * mid + out}


def kernels(frames):
    return predictor.preprocess_batch_device(frames, long_edge=args.long_edge, device=device, fast=fast, channels_last=True)[0]


def kernels_plan_rebuilt(frames):
    # a stream of batches whose sizes never repeat: the plan cache of preprocess_batch_device misses every time
    predictor._plans.clear()
    return kernels(frames)


def baseline(frames):
    # what Predictor ran before: the torch-op batch, then _forward's copy into channels_last
    return predictor.preprocess_batch_torch(frames, long_edge=args.long_edge, device=device, fast=fast)[0].contiguous(
        memory_format=torch.channels_last)


def window(fn, frames, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn(frames)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


for name in args.workload:
    frames = workload(name)
    if args.trace:
        window(kernels, frames, args.warmup)
        print('TRACE-BEGIN %s after %d warm-up batches' % (name, args.warmup), flush=True)
        window(kernels, frames, args.batches)
        print('TRACE-END %s %d batches %s' % (name, args.batches, json.dumps(bytes_moved(frames))), flush=True)
        continue
    equal = bool(torch.equal(kernels(frames), baseline(frames)))
    times = {'kernels': [], 'kernels_plan_rebuilt': [], 'baseline': []}
    for _ in range(args.windows):                      # alternating: both paths see the same machine state
        for label, fn in (('baseline', baseline), ('kernels', kernels), ('kernels_plan_rebuilt', kernels_plan_rebuilt)):
            window(fn, frames, args.warmup)
            times[label].append(window(fn, frames, args.batches))
    med = {k: float(np.median(v)) for k, v in times.items()}
    spread = max(times['baseline']) - min(times['baseline'])
    print(json.dumps({
        'workload': name, 'images': len(frames), 'long_edge': args.long_edge, 'fast': fast,
        'sizes': sorted({f.shape[:2] for f in frames})[:4], 'batches_per_window': args.batches,
        'ms_per_batch': {k: [round(t, 3) for t in v] for k, v in times.items()},
        'median_ms_per_batch': {k: round(v, 3) for k, v in med.items()},
        'baseline_spread_ms': round(spread, 3), 'speedup': round(med['baseline'] / med['kernels'], 2),
        'faster_by_more_than_the_spread': bool(med['baseline'] - med['kernels'] > spread),
        'every_window_faster': bool(max(times['kernels']) < min(times['baseline'])),
        'outputs_equal': equal, 'bytes': bytes_moved(frames)}), flush=True)
