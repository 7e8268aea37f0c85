"""Forward time of the MobileNetV2 trunk and of a LeakyReLU shufflenetv2k16 trunk (each with the cocokp heads) at 641 px, batch 32 and
batch 1, float32 channels-last on one MI355X: the routes this tool is about -- ``fused.MBV2`` (the MobileNetV2 blocks and last
convolution on the unit-mode GEMM and the depthwise stencil with ReLU6) and ``fused.UNIT_LEAKY`` (the 1x1 convolutions of the LeakyReLU
units and ``conv5`` on the unit-mode GEMM) -- against the torch forward of the SAME optimised model with the switch off (what ships),
alternating in one process.  Device events around ``--steps`` forwards after ``--warmup`` of each; ``--rounds`` rounds give the
spread.  One JSON line per (model, batch, route).  The LeakyReLU units are decided like every unit, by the choice table, else by
size; ``--pick x3`` forces the unit GEMM for both sides of the comparison where a size alone would leave it to torch (batch 1).

    python tools/gpu/mobilenetv2_times.py                       # both models, both batches, both routes
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/gpu/mobilenetv2_times.py --models mobilenetv2 --routes on --rounds 1 --steps 1
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
from openpifpaf_amd import fused, headmeta, network  # noqa: E402

MODELS = {'mobilenetv2': ('MBV2', lambda: _rescaled_(network.factory('mobilenetv2', list(headmeta.cocokp_metas())))),
          'shufflenetv2k16-leaky': ('UNIT_LEAKY', lambda: _rescaled_(_leaky_k16()))}


def _leaky_k16():
    torch.manual_seed(0)
    base = network.ShuffleNetV2K('shufflenetv2k16', leaky_relu=True)
    return network.Shell(base, [network.CompositeField4(m, base.out_features) for m in headmeta.cocokp_metas()]).eval()


def _rescaled_(net):
    """Weights of a size that keeps the activations' size from layer to layer -- He's variance by the true fan-out of a grouped
    convolution (the networks' own initialisation counts a depthwise convolution's as C times too large, and without trained
    batch norms the signal dies within a few blocks) -- so that the clips and the comparison of the two routes' outputs see data.
    The times do not depend on the values."""
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for m in net.base_net.modules():
            if isinstance(m, torch.nn.Conv2d):
                fan_out = m.out_channels * m.kernel_size[0] * m.kernel_size[1] // m.groups
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / fan_out) ** 0.5)
    return net


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--models', nargs='+', default=list(MODELS), choices=list(MODELS))
    ap.add_argument('--routes', nargs='+', default=['on', 'off'], choices=['on', 'off'])
    ap.add_argument('--batches', nargs='+', type=int, default=[32, 1])
    ap.add_argument('--size', type=int, default=641)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--pick', choices=['x3', 'conv'], default=None, help='force every pick() to that side (fused.FORCE_PICK)')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    fused.FORCE_PICK = args.pick
    for name in args.models:
        switch, make = MODELS[name]
        net = network.optimize_for_inference_(make()).cuda().to(memory_format=torch.channels_last)
        for batch in args.batches:
            x = torch.randn(batch, 3, args.size, args.size, device='cuda').contiguous(memory_format=torch.channels_last)
            times = {route: [] for route in args.routes}
            outs = {}
            with torch.no_grad():
                for route in args.routes:                   # warm up every shape of both routes (code objects, MIOpen's search)
                    setattr(fused, switch, route == 'on')
                    for _ in range(args.warmup):
                        outs[route] = net(x)
                torch.cuda.synchronize()
                for _ in range(args.rounds):
                    for route in args.routes:
                        setattr(fused, switch, route == 'on')
                        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        start.record()
                        for _ in range(args.steps):
                            net(x)
                        end.record()
                        end.synchronize()
                        times[route].append(start.elapsed_time(end) / args.steps)
            setattr(fused, switch, False)
            delta = None
            if len(outs) == 2:                              # the two routes compute the same fields (reordered float32 sums)
                delta = max(float((a - b).abs().max()) / float(b.abs().max()) for a, b in zip(outs['on'], outs['off']))
            for route in args.routes:
                ms = sorted(times[route])
                print(json.dumps({'model': name, 'switch': switch, 'route': route, 'pick': args.pick, 'batch': batch, 'size': args.size,
                                  'steps': args.steps, 'ms_per_batch_median': ms[len(ms) // 2], 'ms_per_batch_all': times[route],
                                  'images_per_s': 1e3 * batch / ms[len(ms) // 2], 'max_rel_delta_on_vs_off': delta}), flush=True)


if __name__ == '__main__':
    main()
