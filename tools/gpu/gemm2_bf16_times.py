"""Times of the bf16 two-source GEMM route of a ResNet cast to bfloat16 (``fused.PAIR_BF16``, ``csrc/gemm2_bf16.hip``) at 641 px, batch
32 and batch 1, channels-last on one MI355X.

1. The LAYER: for each of the seven distinct blocks with a downsampling convolution of resnet50 (four Bottlenecks) and resnet18 (three
   BasicBlocks), found by running the network once with hooks on those blocks, the tail of the block both ways on the same operands:
   ``new``   Bottleneck: the one launch ``fused.conv1x1_pair_bias_act_bf16`` (conv3 + downsampling + bias + ReLU);
             BasicBlock: ``fused.conv1x1_strided_bf16`` and the bf16 3x3 kernel with the identity as its residual;
   ``off``   what runs with the switch off: torch's bfloat16 ``nn.Conv2d`` for the downsampling convolution, then the tail GEMM with
             the identity as its residual (``fused.conv1x1_bias_act``) for a Bottleneck, the same bf16 3x3 kernel with the identity as
             its residual for a BasicBlock (``fused.CONV3_BF16`` on: the new path changes only the first of the two launches).
   The yardstick is ``off`` in that run.  ``slower``: the median of ``new`` exceeds the median of ``off`` by more than ``off``'s own
   round-to-round spread (max / min); such a layer at batch 32 gets its ``key`` (k1, k2, n, stride) into ``fused.PAIR_BF16_DECLINED``.
2. The WHOLE NETWORK, trunk + heads, of resnet50 and resnet18 in bfloat16 with ``CONV3_BF16`` on: the route on against off.

Device events around a window of calls after ``--warmup`` of each side; the sides alternate in one process, ``--rounds`` rounds give
the spread, medians are reported.  A window of the layer part is ``--kernel-steps`` calls or as many as fill ``--kernel-window-ms``
on the faster side, whichever is more (``steps`` of the line).  The times are device events AROUND the calls on unchanged inputs -- at
batch 1 the operands stay in the caches for both sides.  Every (part, network, batch) runs in a child process of its own under a
``timeout`` of its own, and the first that fails ends the run; one JSON line per layer or network, appended to
``profiles/gemm2_bf16/times.log``.

    python tools/gpu/gemm2_bf16_times.py                               # everything
    python tools/gpu/gemm2_bf16_times.py --parts layer --batches 32
"""
import argparse
import copy
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path.insert(0, ROOT)
from openpifpaf_amd import fused, network  # noqa: E402

LOG = os.path.join(ROOT, 'profiles', 'gemm2_bf16', 'times.log')
MODELS = ('resnet50', 'resnet18')
CL = torch.channels_last
BF16 = torch.bfloat16


def _net(name):
    return network.optimize_for_inference_(network.factory(name)).cuda().to(BF16).to(memory_format=CL).requires_grad_(False)


def blocks(net, size):
    """-> [(block, h_in, w_in)]: every block with a downsampling convolution, in the order it runs, with its input's size."""
    seen = []
    handles = [m.register_forward_pre_hook(lambda block, inputs: seen.append((block, inputs[0].shape[2], inputs[0].shape[3])))
               for m in net.modules() if getattr(m, 'downsample', None) is not None]
    fused.PAIR_BF16 = False
    with torch.no_grad():
        net(torch.zeros(1, 3, size, size, device='cuda', dtype=BF16).contiguous(memory_format=CL))
    for h in handles:
        h.remove()
    return seen


def _window(fn, steps):
    """-> ms per call of ``steps`` calls between two device events."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / steps


def _rounds(sides, steps, warmup, rounds, window_ms=0.0):
    """``sides``: {name: callable}.  -> ({name: [ms per call, one per round]}, calls per window), the sides alternating inside every
    round.  ``window_ms``: a window is at least this long on the fastest side (at most 20 000 calls)."""
    times = {name: [] for name in sides}
    for fn in sides.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    if window_ms > 0:
        fastest = min(_window(fn, steps) for fn in sides.values())
        steps = min(max(steps, int(window_ms / max(fastest, 1e-6)) + 1), 20000)
    for _ in range(rounds):
        for name, fn in sides.items():
            times[name].append(_window(fn, steps))
    return times, steps


def _median(v):
    return sorted(v)[len(v) // 2]


def _verdict(new, off):
    """The issue's yardstick: the route off in this run, and its own round-to-round spread as the margin."""
    spread = max(off) / min(off)
    return {'new_ms_median': _median(new), 'new_ms_all': new, 'off_ms_median': _median(off), 'off_ms_all': off, 'off_spread': spread,
            'new_over_off': _median(new) / _median(off), 'slower': _median(new) > spread * _median(off),
            'faster': _median(new) * spread < _median(off)}


def layer_case(args, name, block, h, w, batch):
    torch.manual_seed(0)
    dconv = block.downsample[0]
    s, k2, n = dconv.stride[0], dconv.in_channels, dconv.out_channels
    ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
    x = torch.randn(batch, k2, h, w, device='cuda').relu_().to(BF16).contiguous(memory_format=CL)
    fused.PAIR_BF16 = fused.CONV3_BF16 = True
    if isinstance(block, network._Bottleneck):
        conv, bias = block.conv3, block.fb3
        k1 = conv.in_channels
        inner = torch.randn(batch, k1, ho, wo, device='cuda').relu_().to(BF16).contiguous(memory_format=CL)
        w2d = conv.weight.reshape(n, k1).contiguous()
        assert fused.pair_bf16_supported(conv, dconv, inner, x, bias) and fused.conv1x1_supported(inner, conv.weight, bias, dconv(x))
        sides = {'new': lambda: fused.conv1x1_pair_bias_act_bf16(conv, dconv, inner, x, bias),
                 'off': lambda: fused.conv1x1_bias_act(inner, w2d, bias, dconv(x), True)}
    else:
        conv, bias = block.conv2, block.fb2
        k1 = 0
        inner = torch.randn(batch, conv.in_channels, ho, wo, device='cuda').relu_().to(BF16).contiguous(memory_format=CL)
        assert fused.conv1x1_strided_bf16_supported(dconv, x) and fused.conv3x3_bf16_supported(conv, inner, bias, dconv(x))
        sides = {'new': lambda: fused.conv3x3_bias_act_bf16(conv, inner, bias, fused.conv1x1_strided_bf16(dconv, x)),
                 'off': lambda: fused.conv3x3_bias_act_bf16(conv, inner, bias, dconv(x))}
    with torch.no_grad():
        times, steps = _rounds(sides, args.kernel_steps, args.warmup, args.rounds, args.kernel_window_ms)
        theirs = sides['off']().float()
        delta = float((sides['new']().float() - theirs).abs().max()) / float(theirs.abs().max())
    line = {'part': 'layer', 'network': name, 'block': type(block).__name__.strip('_'), 'key': [k1, k2, n, s], 'h_in': h, 'w_in': w,
            'batch': batch, 'm': batch * ho * wo, 'size': args.size, 'steps': steps, 'max_rel_delta_new_vs_off': delta}
    line.update(_verdict(times['new'], times['off']))
    return line


def trunk_case(args, name, batch):
    net = _net(name)
    net32 = copy.deepcopy(net).float()
    x = torch.randn(batch, 3, args.size, args.size, device='cuda').to(BF16).contiguous(memory_format=CL)
    fused.CONV3_BF16 = True
    outs = {}

    def side(on):
        def run():
            fused.PAIR_BF16 = on
            outs[on] = net(x)
        return run
    with torch.no_grad():
        times, _ = _rounds({'on': side(True), 'off': side(False)}, args.steps, args.warmup, args.rounds)
        fused.PAIR_BF16 = fused.CONV3_BF16 = False
        ref = net32(x.float())

    def rms(which):
        num = sum(float(((a.double() - b.double()) ** 2).sum()) for a, b in zip(outs[which], ref))
        return (num / sum(float((b.double() ** 2).sum()) for b in ref)) ** 0.5
    line = {'part': 'trunk', 'model': name, 'batch': batch, 'size': args.size, 'steps': args.steps, 'conv3_bf16': True,
            'rms_error_vs_float32_on': rms(True), 'rms_error_vs_float32_off': rms(False)}
    line.update(_verdict(times['on'], times['off']))
    return line


def groups(args):
    """-> [group id]: 'layer/<network>/<batch>' and 'trunk/<network>/<batch>', each a child process"""
    return ['%s/%s/%d' % (part, name, b) for part in ('layer', 'trunk') if part in args.parts for name in args.models for b in args.batches]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parts', nargs='+', default=['layer', 'trunk'], choices=['layer', 'trunk'])
    ap.add_argument('--models', nargs='+', default=list(MODELS), choices=list(MODELS))
    ap.add_argument('--batches', nargs='+', type=int, default=[32, 1])
    ap.add_argument('--size', type=int, default=641)
    ap.add_argument('--steps', type=int, default=5, help='forwards per round of a whole network')
    ap.add_argument('--kernel-steps', type=int, default=20, help='calls per round of one layer alone, at least')
    ap.add_argument('--kernel-window-ms', type=float, default=10.0, help='... and as many as make the faster side\'s window this long')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--group-timeout', type=int, default=240, help='seconds a child process may take')
    ap.add_argument('--log', default=LOG)
    ap.add_argument('--group', help='(a child process:) run this one group and print its lines')
    args = ap.parse_args()
    if args.group:
        assert torch.cuda.is_available(), 'needs a GPU'
        part, name, batch = args.group.split('/')
        if part == 'layer':
            net = _net(name)
            for block, h, w in blocks(net, args.size):
                print(json.dumps(layer_case(args, name, block, h, w, int(batch))), flush=True)
        else:
            print(json.dumps(trunk_case(args, name, int(batch))), flush=True)
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    passed = [a for a in sys.argv[1:]]
    with open(args.log, 'a') as log:
        for group in groups(args):
            cmd = ['timeout', '-k', '10', str(args.group_timeout), sys.executable, os.path.abspath(__file__)] + passed + ['--group', group]
            proc = subprocess.run(cmd, capture_output=True, text=True)
            for line in (ln for ln in proc.stdout.split('\n') if ln.startswith('{')):
                print(line, flush=True)
                log.write(line + '\n')
            log.flush()
            if proc.returncode != 0:                     # a fault, an abort, a time limit: nothing more is started on this GPU
                print('%s: exit status %d\n%s' % (group, proc.returncode, proc.stderr[-2000:]), file=sys.stderr, flush=True)
                return proc.returncode
    return 0


if __name__ == '__main__':
    sys.exit(main())
