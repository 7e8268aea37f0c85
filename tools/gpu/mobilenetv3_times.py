"""Forward time of the MobileNetV3 trunks (with the cocokp heads) at 641 px, batch 32, float32 channels-last on one MI355X: the block
routes on the project's kernels against the same commit's plain torch / MIOpen forward (the default until this has been run: ``OPA_MBV3=1`` switches the routes on; what a PyTorch-ROCm user
gets), alternating in one process.  Device events around ``--steps`` forwards after ``--warmup`` of each; ``--rounds`` rounds give
the spread.  One JSON line per (model, route).

    python tools/gpu/mobilenetv3_times.py                       # both models, both routes
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/gpu/mobilenetv3_times.py --models mobilenetv3large --routes on --rounds 1 --steps 1
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
from openpifpaf_amd import fused, headmeta, network  # noqa: E402


def stencil_times(batch, reps=20):
    """The depthwise stencil alone, ReLU (float32 accumulation) against hardswish (float64 accumulation), at layers of both trunks
    at 641 px: one JSON line per (shape, activation) with the time and the bytes moved (input read once + output written) per second."""
    for C, hw, k, s in ((240, 161, 5, 1), (96, 321, 5, 2), (672, 81, 3, 1), (576, 41, 5, 1)):
        x = torch.randn(batch, C, hw, hw, device='cuda').contiguous(memory_format=torch.channels_last)
        taps, bias = torch.randn(k * k, C, device='cuda'), torch.randn(C, device='cuda')
        for act in (fused.ACT_RELU, fused.ACT_HARDSWISH):
            for _ in range(3):
                out = fused.dwconv_bias_act(x, taps, bias, k, s, act=act)
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(reps):
                fused.dwconv_bias_act(x, taps, bias, k, s, act=act)
            end.record()
            end.synchronize()
            ms = start.elapsed_time(end) / reps
            print(json.dumps({'stencil': [batch, C, hw, hw], 'k': k, 'stride': s, 'act': 'relu/f32' if act == 1 else 'hardswish/f64',
                              'ms': ms, 'TB_per_s': 4 * (x.numel() + out.numel()) / ms / 1e9}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--stencil', action='store_true', help='time the depthwise stencil alone (see stencil_times) and stop')
    ap.add_argument('--models', nargs='+', default=['mobilenetv3large', 'mobilenetv3small'])
    ap.add_argument('--routes', nargs='+', default=['on', 'off'], choices=['on', 'off'])
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=641)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    if args.stencil:
        return stencil_times(args.batch)
    for name in args.models:
        net = network.factory(name, list(headmeta.cocokp_metas()))
        network.optimize_for_inference_(net)
        net = net.cuda().to(memory_format=torch.channels_last)
        x = torch.randn(args.batch, 3, args.size, args.size, device='cuda').contiguous(memory_format=torch.channels_last)
        times = {route: [] for route in args.routes}
        outs = {}
        with torch.no_grad():
            for route in args.routes:                       # warm up every shape of both routes (code objects, MIOpen's search)
                fused.MBV3 = route == 'on'
                for _ in range(args.warmup):
                    outs[route] = net(x)
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for route in args.routes:
                    fused.MBV3 = route == 'on'
                    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    start.record()
                    for _ in range(args.steps):
                        net(x)
                    end.record()
                    end.synchronize()
                    times[route].append(start.elapsed_time(end) / args.steps)
        delta = None
        if len(outs) == 2:                                  # the two routes compute the same fields (reordered float32 sums)
            delta = max(float((a - b).abs().max()) / float(b.abs().max()) for a, b in zip(outs['on'], outs['off']))
        for route in args.routes:
            ms = sorted(times[route])
            print(json.dumps({'model': name, 'route': route, 'batch': args.batch, 'size': args.size, 'steps': args.steps,
                              'ms_per_batch_median': ms[len(ms) // 2], 'ms_per_batch_all': times[route],
                              'images_per_s': 1e3 * args.batch / ms[len(ms) // 2], 'max_rel_delta_on_vs_off': delta}), flush=True)


if __name__ == '__main__':
    main()
