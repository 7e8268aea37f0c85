"""Times of the float16 routes of a ShuffleNetV2K cast with ``.half()`` (``fused.UNIT_F16``: the unit-mode GEMM of
``csrc/gemm_unit_bf16.hip`` on the f16 MFMA, the depthwise stencil of ``csrc/dwconv.hip``) at 641 px, batch 32 and batch 1, channels-last on
one MI355X.  The layers, the windows and the words are ``tools/gpu/unit_bf16_times.py``'s, whose functions this tool imports.

1. ``kernel``: the GEMM against what runs without the switch for the same layer -- torch's float16 ``nn.Conv2d`` (with the folded bias)
   followed by its in-place ReLU -- for every distinct 1x1 layer of shufflenetv2k16 and shufflenetv2k30 (``unit_bf16_times.layers``),
   ``conv5`` and, for k16, the two heads.  For a layer with a partner torch's side is also given with the interleave pass the kernel saves.
2. ``stencil``: the depthwise kernel against torch's float16 grouped ``nn.Conv2d`` (MIOpen) for every distinct depthwise layer: per
   stage the two strided 5 x 5 convolutions of a first unit (on the stage's input and on branch 2's first GEMM output) and the
   stride-1 one of a later unit.
3. ``trunk``: the WHOLE NETWORK, trunk + heads, in float16: the switch on against off.

``faster``: the kernel's slowest round is faster than torch's fastest round; ``slower``: the reverse.  Device events around a window of
calls after ``--warmup`` of each side; the sides alternate in one process, ``--rounds`` rounds give the spread, medians are reported.
Every (part, network, batch) runs in a child process of its own under a ``timeout`` of its own, and the first that fails ends the run;
one JSON line per layer or network, appended to ``profiles/unit_f16/times.log``.

    python tools/gpu/unit_f16_times.py                               # everything
    python tools/gpu/unit_f16_times.py --parts kernel --batches 32
"""
import argparse
import copy
import json
import os
import subprocess
import sys

import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, '..', '..')
sys.path[:0] = [ROOT, HERE]
from openpifpaf_amd import fused, network  # noqa: E402
import unit_bf16_times as bt  # noqa: E402

LOG = os.path.join(ROOT, 'profiles', 'unit_f16', 'times.log')
CL = torch.channels_last
F16 = torch.float16


def _activation(batch, channels, side):
    return torch.randn(batch, channels, side, side, device='cuda').relu_().to(F16).contiguous(memory_format=CL)


def kernel_case(args, name, index, batch):
    label, k, n, side, operand, third = bt.layers(name, args.size)[index]
    torch.manual_seed(0)
    conv = nn.Conv2d(k, n, 1).cuda().to(F16).requires_grad_(False)
    relu = third != 'head'
    nonlin = nn.ReLU(inplace=True) if relu else nn.Identity()
    x = _activation(batch, 2 * k, side)[:, k:] if operand == 'slice' else _activation(batch, k, side)
    partner = _activation(batch, 2 * n, side)[:, :n] if third == 'partner' else None
    fused.UNIT_F16 = True
    assert fused.unit_conv_f16_supported(conv, x, partner)
    sides = {'kernel': lambda: fused.conv1x1_unit_f16(conv, x, relu=relu, partner=partner), 'torch': lambda: nonlin(conv(x))}
    if partner is not None:
        sides['torch+interleave'] = lambda: fused.channel_interleave(partner, nonlin(conv(x)))
    with torch.no_grad():
        times, steps = bt._rounds(sides, args.kernel_steps, args.warmup, args.rounds, args.kernel_window_ms)
        theirs = sides['torch+interleave' if partner is not None else 'torch']().float()
        delta = float((sides['kernel']().float() - theirs).abs().max()) / float(theirs.abs().max())
    m = batch * side * side
    line = {'part': 'kernel', 'network': name, 'layer': label, 'k': k, 'n': n, 'side': side, 'batch': batch, 'm': m, 'operand': operand,
            'third': third, 'size': args.size, 'steps': steps, 'kernel_ms_median': bt._median(times['kernel']),
            'kernel_ms_all': times['kernel'], 'torch_ms_median': bt._median(times['torch']), 'torch_ms_all': times['torch'],
            'faster': max(times['kernel']) < min(times['torch']), 'slower': min(times['kernel']) > max(times['torch']),
            'kernel_call_tflops': 2.0 * m * k * n / (bt._median(times['kernel']) * 1e-3) / 1e12,       # (of the call, launch overhead included)
            'max_rel_delta_kernel_vs_torch': delta}
    if partner is not None:
        line.update(torch_plus_interleave_ms_median=bt._median(times['torch+interleave']), torch_plus_interleave_ms_all=times['torch+interleave'])
    return line


def stencils(name, size):
    """-> [(label, channels, input side, stride)]: each distinct depthwise layer (5 x 5, padding 2) once."""
    c0, b2, b3, b4, _ = bt.WIDTHS[name]
    sides = [(size - 1) // 2 + 1]
    for _ in range(3):
        sides.append((sides[-1] - 1) // 2 + 1)
    out, cin = [], c0
    for stage, (b, sa, sb) in enumerate(zip((b2, b3, b4), sides[:3], sides[1:]), start=2):
        out += [('stage%d first unit, branch1 depthwise' % stage, cin, sa, 2), ('stage%d first unit, branch2 depthwise' % stage, b, sa, 2),
                ('stage%d unit, depthwise' % stage, b, sb, 1)]
        cin = 2 * b
    return out


def stencil_case(args, name, index, batch):
    label, c, side, stride = stencils(name, args.size)[index]
    torch.manual_seed(0)
    conv = nn.Conv2d(c, c, 5, stride, 2, groups=c).cuda().to(F16).requires_grad_(False)
    taps = fused.depthwise_taps(conv.weight)
    x = _activation(batch, c, side)
    fused.UNIT_F16 = True
    if not fused.dwconv_supported(x, 5, stride):             # (batch x output rows above the kernel's grid: the route declines too)
        return {'part': 'stencil', 'network': name, 'layer': label, 'channels': c, 'side': side, 'stride': stride, 'batch': batch, 'declined': True}
    sides = {'kernel': lambda: fused.dwconv_bias_act(x, taps, conv.bias, 5, stride), 'torch': lambda: conv(x)}
    with torch.no_grad():
        times, steps = bt._rounds(sides, args.kernel_steps, args.warmup, args.rounds, args.kernel_window_ms)
        theirs = sides['torch']().float()
        delta = float((sides['kernel']().float() - theirs).abs().max()) / float(theirs.abs().max())
    out = (side - 1) // stride + 1
    moved = batch * c * (side * side + out * out) * 2
    return {'part': 'stencil', 'network': name, 'layer': label, 'channels': c, 'side': side, 'stride': stride, 'batch': batch, 'size': args.size,
            'steps': steps, 'kernel_ms_median': bt._median(times['kernel']), 'kernel_ms_all': times['kernel'],
            'torch_ms_median': bt._median(times['torch']), 'torch_ms_all': times['torch'],
            'faster': max(times['kernel']) < min(times['torch']), 'slower': min(times['kernel']) > max(times['torch']),
            'kernel_call_gb_per_s': moved / (bt._median(times['kernel']) * 1e-3) / 1e9, 'max_rel_delta_kernel_vs_torch': delta}


def trunk_case(args, name, batch):
    net32 = network.optimize_for_inference_(network.factory(name)).cuda().to(memory_format=CL).requires_grad_(False)
    net = copy.deepcopy(net32).half()
    x32 = torch.randn(batch, 3, args.size, args.size, device='cuda').contiguous(memory_format=CL)
    x = x32.half()
    outs = {}

    def side(on):
        def run():
            fused.UNIT_F16 = on
            outs[on] = net(x)
        return run
    with torch.no_grad():
        times, _ = bt._rounds({'on': side(True), 'off': side(False)}, args.steps, args.warmup, args.rounds)
        fused.UNIT_F16 = False
        outs['float32'] = net32(x32)
    torch.cuda.synchronize()

    def rms(which):
        num = sum(float(((a.double() - b.double()) ** 2).sum()) for a, b in zip(outs[which], outs['float32']))
        return (num / sum(float((b.double() ** 2).sum()) for b in outs['float32'])) ** 0.5
    return {'part': 'trunk', 'model': name, 'batch': batch, 'size': args.size, 'steps': args.steps,
            'f16_route_on_ms_median': bt._median(times['on']), 'f16_route_on_ms_all': times['on'],
            'f16_route_off_ms_median': bt._median(times['off']), 'f16_route_off_ms_all': times['off'],
            'faster': max(times['on']) < min(times['off']), 'slower': min(times['on']) > max(times['off']),
            'rms_error_vs_float32_on': rms(True), 'rms_error_vs_float32_off': rms(False)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parts', nargs='+', default=['kernel', 'stencil', 'trunk'], choices=['kernel', 'stencil', 'trunk'])
    ap.add_argument('--models', nargs='+', default=list(bt.WIDTHS), choices=list(bt.WIDTHS))
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
        if part == 'kernel':
            for index in range(len(bt.layers(name, args.size))):
                print(json.dumps(kernel_case(args, name, index, int(batch))), flush=True)
        elif part == 'stencil':
            for index in range(len(stencils(name, args.size))):
                print(json.dumps(stencil_case(args, name, index, int(batch))), flush=True)
        else:
            print(json.dumps(trunk_case(args, name, int(batch))), flush=True)
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    passed = [a for a in sys.argv[1:]]
    with open(args.log, 'a') as log:
        for group in ['%s/%s/%d' % (part, name, b) for part in args.parts for name in args.models for b in args.batches]:
            cmd = ['timeout', '-k', '10', str(args.group_timeout), sys.executable, os.path.abspath(__file__)] + passed + ['--group', group]
            proc = subprocess.run(cmd, capture_output=True, text=True)
            lines = [ln for ln in proc.stdout.split('\n') if ln.startswith('{')]
            for line in lines:
                print(line, flush=True)
                log.write(line + '\n')
            log.flush()
            if proc.returncode != 0:                     # a fault, an abort, a time limit: nothing more is started on this GPU
                print('%s: exit status %d\n%s' % (group, proc.returncode, proc.stderr[-2000:]), file=sys.stderr, flush=True)
                return proc.returncode
    return 0


if __name__ == '__main__':
    sys.exit(main())
