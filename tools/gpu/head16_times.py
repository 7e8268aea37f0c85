"""Times of the 16-bit head route (``fused.HEAD16``: ``csrc/head16.hip``, the head's 1x1 convolution and ``CompositeField4``'s epilogue
in one kernel) at 641 px, batch 32 and batch 1, bfloat16 and float16, channels-last on one MI355X.

1. The LAYER: the COCO Cif (N = 340) and Caf (N = 608) heads of resnet50 (K = 2048) and resnet18 (K = 512) on the trunk's own output,
   two ways on the same operands:
   ``head16``  ``fused.head_conv_fields16``: one launch;
   ``torch``   what runs without the switch: torch's 16-bit ``nn.Conv2d`` followed by ``fused.head_epilogue`` (``opa_head_epilogue``).
   The yardstick is ``torch`` in that run.  ``faster``: the new route's slowest round is faster than torch's fastest round;
   ``slower``: the reverse -- such a layer at batch 32 belongs into ``fused.HEAD16_DECLINED``.
2. The WHOLE NETWORK, trunk + heads, of resnet50 and resnet18 in both types (``OPA_CONV1X1=gemm``, the trunk's own 16-bit switches on
   on both sides): ``HEAD16`` on against off.

Device events around a window of calls after ``--warmup`` of each side; the sides alternate in one process, ``--rounds`` rounds give
the spread, medians are reported.  A window of the layer part is ``--kernel-steps`` calls or as many as fill ``--kernel-window-ms``
on the fastest side, whichever is more (``steps`` of the line).  The times are device events AROUND the calls on unchanged inputs -- at
batch 1 the operands stay in the caches for every side.  Every (part, network, batch) runs in a child process of its own under a
``timeout`` of its own, and the first that fails ends the run; one JSON line per layer or network, appended to
``profiles/head16/times.log``.

    python tools/gpu/head16_times.py                               # everything
    python tools/gpu/head16_times.py --parts layer --batches 32
"""
import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path.insert(0, ROOT)
from openpifpaf_amd import fused, network  # noqa: E402

LOG = os.path.join(ROOT, 'profiles', 'head16', 'times.log')
MODELS = ('resnet50', 'resnet18')
CL = torch.channels_last
DTYPES = {'bfloat16': torch.bfloat16, 'float16': torch.float16}


def _net(name, dtype):
    return network.optimize_for_inference_(network.factory(name)).cuda().to(dtype).to(memory_format=CL).requires_grad_(False)


def _trunk_switches(dtype, on=True):
    """The trunk's own 16-bit routes of ``dtype``: the same on both sides of every comparison."""
    fused.F16 = on and dtype == torch.float16
    fused.CONV3_BF16 = fused.PAIR_BF16 = fused.STEM7_BF16 = on and dtype == torch.bfloat16


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


def layer_cases(args, name, batch):
    os.environ['OPA_CONV1X1'] = 'gemm'
    for dtype_name, dtype in DTYPES.items():
        net = _net(name, dtype)
        _trunk_switches(dtype)
        fused.HEAD16 = True
        with torch.no_grad():
            x = net.base_net(torch.randn(batch, 3, args.size, args.size, device='cuda').to(dtype).contiguous(memory_format=CL))
            for head in net.head_nets:
                conv, meta = head.conv, head.meta
                assert fused.head_conv_fields16_supported(conv, x, meta)
                sides = {'head16': lambda: fused.head_conv_fields16(conv, x, meta), 'torch': lambda: fused.head_epilogue(conv(x), meta)}
                assert fused.head_epilogue_supported(conv(x), meta)
                times, steps = _rounds(sides, args.kernel_steps, args.warmup, args.rounds, args.kernel_window_ms)
                ref = sides['torch']()
                delta = float((sides['head16']() - ref).abs().max()) / float(ref.abs().max())
                t, n = _median(times['head16']), conv.out_channels
                m, k = x.shape[0] * x.shape[2] * x.shape[3], conv.in_channels
                fields = ref.numel() * 4
                yield {'part': 'layer', 'network': name, 'head': meta.name, 'dtype': dtype_name, 'batch': batch, 'size': args.size,
                       'key': [k, n, meta.upsample_stride], 'pixels': m, 'steps': steps,
                       'head16_ms_median': t, 'head16_ms_all': times['head16'], 'torch_ms_median': _median(times['torch']), 'torch_ms_all': times['torch'],
                       'torch_over_head16': _median(times['torch']) / t, 'head16_over_torch': t / _median(times['torch']),
                       'faster': max(times['head16']) < min(times['torch']), 'slower': min(times['head16']) > max(times['torch']),
                       'head16_bytes_x_plus_fields': m * k * 2 + fields, 'torch_bytes_plus_conv_output_twice': m * k * 2 + fields + 2 * m * n * 2,
                       'head16_call_tb_per_s': (m * k * 2 + fields) / (t * 1e-3) / 1e12, 'max_rel_delta_head16_vs_torch': delta}


def trunk_cases(args, name, batch):
    os.environ['OPA_CONV1X1'] = 'gemm'
    for dtype_name, dtype in DTYPES.items():
        net = _net(name, dtype)
        _trunk_switches(dtype)
        x = torch.randn(batch, 3, args.size, args.size, device='cuda').to(dtype).contiguous(memory_format=CL)

        def side(on):
            def run():
                fused.HEAD16 = on
                net(x)
            return run
        with torch.no_grad():
            times, _ = _rounds({'on': side(True), 'off': side(False)}, args.steps, args.warmup, args.rounds)
        fused.HEAD16 = False
        yield {'part': 'trunk', 'model': name, 'dtype': dtype_name, 'batch': batch, 'size': args.size, 'steps': args.steps,
               'head16_on_ms_median': _median(times['on']), 'head16_on_ms_all': times['on'],
               'head16_off_ms_median': _median(times['off']), 'head16_off_ms_all': times['off'],
               'off_over_on': _median(times['off']) / _median(times['on']),
               'faster': max(times['on']) < min(times['off']), 'slower': min(times['on']) > max(times['off'])}


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
    ap.add_argument('--kernel-window-ms', type=float, default=10.0, help='... and as many as make the fastest side\'s window this long')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--group-timeout', type=int, default=240, help='seconds a child process may take')
    ap.add_argument('--log', default=LOG)
    ap.add_argument('--group', help='(a child process:) run this one group and print its lines')
    args = ap.parse_args()
    if args.group:
        assert torch.cuda.is_available(), 'needs a GPU'
        part, name, batch = args.group.split('/')
        for line in (layer_cases if part == 'layer' else trunk_cases)(args, name, int(batch)):
            print(json.dumps(line), flush=True)
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
