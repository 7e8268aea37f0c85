"""``decoder.CifDet.batch``, decode only: a model stub hands out 32 precomputed ``synth_det_field`` images that already lie on
the device, so what is timed is candidates + NMS + score filter + box conversion + the way back to the host + building the
``AnnotationDet`` objects.  Every timed window follows a warm-up and ends in a device synchronise.

    python tools/gpu/cifdet_batch_time.py [--package-root DIR] [--windows 3] [--batches 20] [--warmup 5]

``--package-root`` puts another checkout's root in front of ``sys.path`` (to time two versions alternately from one shell
loop); one JSON line per run.  ``--trace`` runs only ``--batches`` batches after the warm-up, between two markers on stdout,
for a ``rocprofv3 --kernel-trace --memory-copy-trace --stats`` run around it."""
import argparse
import json
import os
import sys
import time

parser = argparse.ArgumentParser()
parser.add_argument('--package-root', default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
parser.add_argument('--images', type=int, default=32)
parser.add_argument('--categories', type=int, default=80)
parser.add_argument('--objects', type=int, nargs='+', default=[5, 20, 60, 150], help='objects per image, cycled over the batch')
parser.add_argument('--size', type=int, default=81, help='field height and width')
parser.add_argument('--windows', type=int, default=3)
parser.add_argument('--batches', type=int, default=20, help='batches per timed window')
parser.add_argument('--warmup', type=int, default=5)
parser.add_argument('--trace', action='store_true')
parser.add_argument('--label', default='')
args = parser.parse_args()
sys.path.insert(0, os.path.abspath(args.package_root))

import numpy as np      # noqa: E402
import torch            # noqa: E402

from openpifpaf_amd import decoder, headmeta, synth      # noqa: E402

assert torch.cuda.is_available(), 'this measurement needs the GPU'
fields = np.stack([synth.synth_det_field(100 + b, args.objects[b % len(args.objects)], n_categories=args.categories,
                                         height=args.size, width=args.size) for b in range(args.images)])
dev = torch.from_numpy(fields).cuda()
images = torch.zeros((args.images, 3, 8, 8), device='cuda')
meta = headmeta.CifDet('cifdet', 'synthetic', categories=['c%d' % i for i in range(args.categories)])
meta.head_index, meta.base_stride, meta.upsample_stride = 0, 16, 2
dec = decoder.CifDet.factory([meta])[0]


def model(image_batch):
    return (dev,)


def run(n):
    out = None
    for _ in range(n):
        out = dec.batch(model, images)
    torch.cuda.synchronize()
    return out


result = run(args.warmup)
detections = [len(r) for r in result]
if args.trace:
    print('TRACE-BEGIN after %d warm-up batches' % args.warmup, flush=True)
    run(args.batches)
    print('TRACE-END %d batches' % args.batches, flush=True)
windows = []
for _ in range(0 if args.trace else args.windows):
    t0 = time.perf_counter()
    run(args.batches)
    windows.append((time.perf_counter() - t0) / args.batches * 1e3)
print(json.dumps({'label': args.label, 'images': args.images,
                  'categories': args.categories, 'field': args.size, 'batches_per_window': args.batches,
                  'warmup_batches': args.warmup, 'ms_per_batch': [round(w, 3) for w in windows],
                  'detections_per_image': detections, 'has_device_nms': hasattr(dec, 'batch_async')}))
