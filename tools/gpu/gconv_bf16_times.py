"""Times of the bf16 grouped 3x3 implicit-GEMM route of a ResNeXt cast to bfloat16 (``fused.GCONV_BF16``, ``csrc/gconv3x3_bf16.hip``) at
641 px, batch 32 and batch 1, channels-last on one MI355X.

1. The KERNEL against what runs without the switch for the same layer -- torch's bfloat16 grouped ``nn.Conv2d`` followed by
   ``fused.bias_act_`` (the folded bias and the ReLU; inside a network that epilogue is the next GEMM's operand prologue instead, so
   this side is the layer on its own, not its share of the network) -- for every distinct grouped 3x3 layer of resnext50 and
   resnext101: (C, CG, stride, dilation, input side), found by running the network once with hooks on its convolutions.  ``faster``:
   the kernel's slowest round is faster than torch's fastest round; ``slower``: the reverse.  ``bytes_moved``: x read once + the
   output written once + the packed weight read once; ``kernel_bytes_per_s``: those over the kernel's time, launch overhead included,
   beside the 6.29 TB/s float4 copy rate measured on this GPU (``MI355X_MICROARCH.md``): a share of the measured copy rate, not of the
   specification's peak.  ``kernel_call_tflops``: the MFMA work the kernel does (2 M 9 C 32 with CG <= 32, 2 M 9 C 64 with CG = 64:
   off-group zeros included) over the same time.
2. The WHOLE NETWORK, trunk + heads, of resnext50 and resnext101 in bfloat16 with the other three bf16 switches (``CONV3_BF16``,
   ``STEM7_BF16``, ``PAIR_BF16``) on: this route on against off, and the head fields' rms error against the float32 network for both.

Device events around a window of calls after ``--warmup`` of each side; the sides alternate in one process, ``--rounds`` rounds give
the spread, medians are reported.  A window of the kernel part is ``--kernel-steps`` calls or as many as fill ``--kernel-window-ms``
on the faster side, whichever is more (``steps`` of the line).  The times are device events AROUND the calls on one unchanged input
-- at batch 1 the operands stay in the caches for both sides.  Every (part, network, batch) runs in a child process of its own under
a ``timeout`` of its own, and the first that fails ends the run; one JSON line per layer or network, appended to
``profiles/gconv_bf16/times.log``; the trunk lines' errors also to ``profiles/gconv_bf16/route_errors.log``.

    python tools/gpu/gconv_bf16_times.py                               # everything
    python tools/gpu/gconv_bf16_times.py --parts kernel --batches 32
"""
import argparse
import copy
import json
import os
import subprocess
import sys

import torch
from torch import nn

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path.insert(0, ROOT)
from openpifpaf_amd import fused, network  # noqa: E402

LOG = os.path.join(ROOT, 'profiles', 'gconv_bf16', 'times.log')
ERRORS = os.path.join(ROOT, 'profiles', 'gconv_bf16', 'route_errors.log')
MODELS = ('resnext50', 'resnext101')
COPY_RATE = 6.29e12
PEAK_TFLOPS = 2500.0
CL = torch.channels_last
BF16 = torch.bfloat16


def _net(name):
    net = network.optimize_for_inference_(network.factory(name)).cuda().to(BF16).to(memory_format=CL).requires_grad_(False)
    return net


def layers(name, size):
    """-> [(C, CG, stride, dilation, h, w)]: each distinct grouped 3x3 layer of the trunk once, in the order it runs."""
    net, seen = _net(name), []

    def hook(conv, inputs):
        x = inputs[0]
        key = (conv.in_channels, conv.in_channels // conv.groups, conv.stride[0], conv.dilation[0], x.shape[2], x.shape[3])
        if key not in seen:
            seen.append(key)
    handles = [m.register_forward_pre_hook(hook) for m in net.modules()
               if isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3) and m.groups > 1]
    fused.GCONV_BF16 = False
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


def kernel_case(args, name, layer, batch):
    c, cg, s, d, h, w = layer
    torch.manual_seed(0)
    conv = nn.Conv2d(c, c, 3, s, d, dilation=d, groups=c // cg, bias=False).cuda().to(BF16).requires_grad_(False)
    bias = (torch.randn(c, device='cuda') * 0.5).to(BF16)
    x = torch.randn(batch, c, h, w, device='cuda').relu_().to(BF16).contiguous(memory_format=CL)
    ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
    fused.GCONV_BF16 = True
    assert fused.gconv3x3_bf16_supported(conv, x, bias)
    sides = {'kernel': lambda: fused.gconv3x3_bias_act_bf16(conv, x, bias, relu=True),
             'torch': lambda: fused.bias_act_(conv(x), bias, None, True)}
    with torch.no_grad():
        times, steps = _rounds(sides, args.kernel_steps, args.warmup, args.rounds, args.kernel_window_ms)
        theirs = sides['torch']().float()
        delta = float((sides['kernel']().float() - theirs).abs().max()) / float(theirs.abs().max())
    m = batch * ho * wo
    seconds = _median(times['kernel']) * 1e-3
    moved = 2 * (batch * h * w * c + m * c + c * 9 * 64)
    tflops = 2.0 * m * 9 * c * (32 if cg <= 32 else 64) / seconds / 1e12
    return {'part': 'kernel', 'network': name, 'channels': c, 'group_width': cg, 'stride': s, 'dilation': d, 'h': h, 'w': w,
            'batch': batch, 'm': m, 'size': args.size, 'steps': steps, 'kernel_ms_median': _median(times['kernel']),
            'kernel_ms_all': times['kernel'], 'torch_ms_median': _median(times['torch']), 'torch_ms_all': times['torch'],
            'kernel_over_torch': _median(times['kernel']) / _median(times['torch']),
            'faster': max(times['kernel']) < min(times['torch']), 'slower': min(times['kernel']) > max(times['torch']),
            'bytes_moved': moved, 'kernel_bytes_per_s': moved / seconds, 'measured_copy_rate_bytes_per_s': COPY_RATE,
            'share_of_measured_copy_rate': moved / seconds / COPY_RATE, 'kernel_call_tflops': tflops,
            'share_of_bf16_peak': tflops / PEAK_TFLOPS, 'max_rel_delta_kernel_vs_torch': delta}


def trunk_case(args, name, batch):
    net = _net(name)
    net32 = copy.deepcopy(net).float()
    x = torch.randn(batch, 3, args.size, args.size, device='cuda').to(BF16).contiguous(memory_format=CL)
    outs = {}
    fused.CONV3_BF16 = fused.STEM7_BF16 = fused.PAIR_BF16 = True

    def side(on):
        def run():
            fused.GCONV_BF16 = on
            outs[on] = net(x)
        return run
    with torch.no_grad():
        times, _ = _rounds({'on': side(True), 'off': side(False)}, args.steps, args.warmup, args.rounds)
        fused.GCONV_BF16 = fused.CONV3_BF16 = fused.STEM7_BF16 = fused.PAIR_BF16 = False
        ref = net32(x.float())

    def rms(which):
        num = sum(float(((a.double() - b.double()) ** 2).sum()) for a, b in zip(outs[which], ref))
        return (num / sum(float((b.double() ** 2).sum()) for b in ref)) ** 0.5
    return {'part': 'trunk', 'model': name, 'batch': batch, 'size': args.size, 'steps': args.steps,
            'other_bf16_switches': 'CONV3_BF16 STEM7_BF16 PAIR_BF16 on',
            'gconv_bf16_on_ms_median': _median(times['on']), 'gconv_bf16_on_ms_all': times['on'],
            'gconv_bf16_off_ms_median': _median(times['off']), 'gconv_bf16_off_ms_all': times['off'],
            'faster': max(times['on']) < min(times['off']), 'slower': min(times['on']) > max(times['off']),
            'rms_error_vs_float32_on': rms(True), 'rms_error_vs_float32_off': rms(False)}


def groups(args):
    """-> [group id]: 'kernel/<network>/<batch>' and 'trunk/<network>/<batch>', each a child process"""
    return ['%s/%s/%d' % (part, name, b) for part in ('kernel', 'trunk') if part in args.parts for name in args.models for b in args.batches]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parts', nargs='+', default=['kernel', 'trunk'], choices=['kernel', 'trunk'])
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
    ap.add_argument('--errors-log', default=ERRORS)
    ap.add_argument('--group', help='(a child process:) run this one group and print its lines')
    args = ap.parse_args()
    if args.group:
        assert torch.cuda.is_available(), 'needs a GPU'
        part, name, batch = args.group.split('/')
        if part == 'kernel':
            for layer in layers(name, args.size):
                print(json.dumps(kernel_case(args, name, layer, int(batch))), flush=True)
        else:
            print(json.dumps(trunk_case(args, name, int(batch))), flush=True)
        return 0
    for path in (args.log, args.errors_log):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    passed = [a for a in sys.argv[1:]]
    with open(args.log, 'a') as log, open(args.errors_log, 'a') as errors:
        for group in groups(args):
            cmd = ['timeout', '-k', '10', str(args.group_timeout), sys.executable, os.path.abspath(__file__)] + passed + ['--group', group]
            proc = subprocess.run(cmd, capture_output=True, text=True)
            for line in (ln for ln in proc.stdout.split('\n') if ln.startswith('{')):
                print(line, flush=True)
                log.write(line + '\n')
                row = json.loads(line)
                if row['part'] == 'trunk':
                    errors.write('GCONVBF16TIMES %s | batch %d | %d px | e_off (torch grouped bfloat16) %.4e | e_on (bf16 grouped implicit '
                                 'GEMM) %.4e | e_on / e_off %.3f\n' % (row['model'], row['batch'], row['size'], row['rms_error_vs_float32_off'],
                                                                       row['rms_error_vs_float32_on'],
                                                                       row['rms_error_vs_float32_on'] / row['rms_error_vs_float32_off']))
            log.flush()
            errors.flush()
            if proc.returncode != 0:                     # a fault, an abort, a time limit: nothing more is started on this GPU
                print('%s: exit status %d\n%s' % (group, proc.returncode, proc.stderr[-2000:]), file=sys.stderr, flush=True)
                return proc.returncode
    return 0


if __name__ == '__main__':
    sys.exit(main())
