"""Times of the float16 grouped 3x3 and 7x7 stem routes of a ResNeXt / ResNet cast with ``.half()`` (``fused.GCONV_F16``,
``fused.STEM7_F16``: csrc/gconv3x3_bf16.hip and csrc/stem7x7_bf16.hip on v_mfma_f32_32x32x16_f16) at 641 px, batch 32 and batch 1,
channels-last on one MI355X, in the manner of ``gconv_bf16_times.py`` and ``stem7_bf16_times.py``.

1. ``gconv``: the grouped KERNEL against what runs without the switch for the same layer -- torch's float16 grouped ``nn.Conv2d``
   followed by ``fused.bias_act_`` (inside a network that epilogue is the next GEMM's operand prologue instead, so this side is the
   layer on its own, not its share of the network) -- for every distinct grouped 3x3 layer of resnext50 and resnext101: (C, CG,
   stride, dilation, input side), found by running the network once with hooks on its convolutions.
2. ``stem``: the 7x7 stem, 64 channels, stride 2, against torch's float16 ``nn.Conv2d`` + ``fused.bias_act_``; ``pooled``: both sides
   with ``F.max_pool2d(3, 2, 1)`` behind them (the pool kernel takes no float16 tensor), as ``Resnet._input_block_fused`` runs them
   with ``pool0_stride=2``.
3. ``trunk``: the WHOLE NETWORK, trunk + heads, of resnext50, resnext101, resnet50 and resnet18 in float16 with ``F16`` and ``HEAD16``
   on: the two new switches on against off, and the head fields' rms error against the float32 network for both.

``faster``: the kernel's slowest round is faster than torch's fastest round; ``slower``: the reverse -- a layer that is ``slower`` at
batch 32 belongs in ``fused.GCONV_F16_DECLINED`` / ``fused.STEM7_F16_DECLINED``.  Device events around a window of calls after
``--warmup`` of each side; the sides alternate in one process, ``--rounds`` rounds give the spread, medians are reported.  The times
are device events AROUND the calls on one unchanged input -- at batch 1 the operands stay in the caches for both sides.  Every
(part, network, batch) runs in a child process of its own under a ``timeout`` of its own, and the first that fails ends the run; one
JSON line per layer or network, appended to ``profiles/f16x/times.log``.

    python tools/gpu/f16x_times.py                               # everything
    python tools/gpu/f16x_times.py --parts gconv --batches 32
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

LOG = os.path.join(ROOT, 'profiles', 'f16x', 'times.log')
GROUPED = ('resnext50', 'resnext101')
TRUNKS = ('resnext50', 'resnext101', 'resnet50', 'resnet18')
CL = torch.channels_last
F16 = torch.float16


def _net(name):
    return network.optimize_for_inference_(network.factory(name)).cuda().to(F16).to(memory_format=CL).requires_grad_(False)


def layers(name, size):
    """-> [(C, CG, stride, dilation, h, w)]: each distinct grouped 3x3 layer of the trunk once, in the order it runs."""
    net, seen = _net(name).base_net, []

    def hook(conv, inputs):
        x = inputs[0]
        key = (conv.in_channels, conv.in_channels // conv.groups, conv.stride[0], conv.dilation[0], x.shape[2], x.shape[3])
        if key not in seen:
            seen.append(key)
    handles = [m.register_forward_pre_hook(hook) for m in net.modules()
               if isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3) and m.groups > 1]
    fused.GCONV_F16 = False
    with torch.no_grad():
        net(torch.zeros(1, 3, size, size, device='cuda', dtype=F16).contiguous(memory_format=CL))
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


def _sides_row(times, steps):
    return {'steps': steps, 'kernel_ms_median': _median(times['kernel']), 'kernel_ms_all': times['kernel'],
            'torch_ms_median': _median(times['torch']), 'torch_ms_all': times['torch'],
            'kernel_over_torch': _median(times['kernel']) / _median(times['torch']),
            'faster': max(times['kernel']) < min(times['torch']), 'slower': min(times['kernel']) > max(times['torch'])}


def gconv_case(args, name, layer, batch):
    c, cg, s, d, h, w = layer
    torch.manual_seed(0)
    conv = nn.Conv2d(c, c, 3, s, d, dilation=d, groups=c // cg, bias=False).cuda().to(F16).requires_grad_(False)
    bias = (torch.randn(c, device='cuda') * 0.5).to(F16)
    x = torch.randn(batch, c, h, w, device='cuda').relu_().to(F16).contiguous(memory_format=CL)
    fused.GCONV_F16 = True
    assert fused.gconv3x3_bf16_supported(conv, x, bias)
    sides = {'kernel': lambda: fused.gconv3x3_bias_act_bf16(conv, x, bias, relu=True),
             'torch': lambda: fused.bias_act_(conv(x), bias, None, True)}
    with torch.no_grad():
        times, steps = _rounds(sides, args.kernel_steps, args.warmup, args.rounds, args.kernel_window_ms)
        theirs = sides['torch']().float()
        delta = float((sides['kernel']().float() - theirs).abs().max()) / float(theirs.abs().max())
    m = batch * ((h - 1) // s + 1) * ((w - 1) // s + 1)
    row = {'part': 'gconv', 'network': name, 'channels': c, 'group_width': cg, 'stride': s, 'dilation': d, 'h': h, 'w': w,
           'batch': batch, 'm': m, 'size': args.size}
    row.update(_sides_row(times, steps))
    row['kernel_call_tflops'] = 2.0 * m * 9 * c * (32 if cg <= 32 else 64) / (row['kernel_ms_median'] * 1e-3) / 1e12
    row['max_rel_delta_kernel_vs_torch'] = delta
    return row


def stem_case(args, batch, pooled):
    torch.manual_seed(0)
    n, s = 64, 2
    conv = nn.Conv2d(3, n, 7, s, 3, bias=False).cuda().to(F16).to(memory_format=CL).requires_grad_(False)
    bias = (torch.randn(n, device='cuda') * 0.5).to(F16)
    x = torch.randn(batch, 3, args.size, args.size, device='cuda').to(F16).contiguous(memory_format=CL)
    fused.STEM7_F16 = True
    assert fused.stem7x7_bf16_supported(conv, x, bias, pooled)
    pool = (lambda t: torch.nn.functional.max_pool2d(t, 3, 2, 1)) if pooled else (lambda t: t)
    sides = {'kernel': lambda: pool(fused.stem7x7_bias_act_bf16(conv, x, bias, relu=True)),
             'torch': lambda: pool(fused.bias_act_(conv(x), bias, None, True))}
    with torch.no_grad():
        times, steps = _rounds(sides, args.kernel_steps, args.warmup, args.rounds, args.kernel_window_ms)
        theirs = sides['torch']().float()
        delta = float((sides['kernel']().float() - theirs).abs().max()) / float(theirs.abs().max())
    row = {'part': 'stem', 'pooled': pooled, 'c_out': n, 'stride': s, 'batch': batch, 'size': args.size}
    row.update(_sides_row(times, steps))
    row['max_rel_delta_kernel_vs_torch'] = delta
    return row


def trunk_case(args, name, batch):
    net = _net(name)
    x = torch.randn(batch, 3, args.size, args.size, device='cuda').to(F16).contiguous(memory_format=CL)
    outs = {}
    fused.F16 = fused.HEAD16 = True

    def side(on):
        def run():
            fused.GCONV_F16 = fused.STEM7_F16 = on
            outs[on] = net(x)
        return run
    with torch.no_grad():
        times, _ = _rounds({'on': side(True), 'off': side(False)}, args.steps, args.warmup, args.rounds)
        fused.GCONV_F16 = fused.STEM7_F16 = fused.F16 = fused.HEAD16 = False
        ref = copy.deepcopy(net).float()(x[:1].float())                # (the error on the first image: the float32 forward is the long part)

    def rms(which):
        num = sum(float(((a[:1].double() - b.double()) ** 2).sum()) for a, b in zip(outs[which], ref))
        return (num / sum(float((b.double() ** 2).sum()) for b in ref)) ** 0.5
    return {'part': 'trunk', 'model': name, 'batch': batch, 'size': args.size, 'steps': args.steps, 'other_switches': 'F16 HEAD16 on',
            'f16x_on_ms_median': _median(times['on']), 'f16x_on_ms_all': times['on'],
            'f16x_off_ms_median': _median(times['off']), 'f16x_off_ms_all': times['off'],
            'on_over_off': _median(times['on']) / _median(times['off']),
            'faster': max(times['on']) < min(times['off']), 'slower': min(times['on']) > max(times['off']),
            'rms_error_vs_float32_on': rms(True), 'rms_error_vs_float32_off': rms(False)}


def groups(args):
    """-> [group id]: 'gconv/<network>/<batch>', 'stem/-/<batch>' and 'trunk/<network>/<batch>', each a child process"""
    out = []
    for b in args.batches:
        out += ['gconv/%s/%d' % (name, b) for name in GROUPED if 'gconv' in args.parts]
        out += ['stem/-/%d' % b] if 'stem' in args.parts else []
    for b in args.batches:
        out += ['trunk/%s/%d' % (name, b) for name in args.models if 'trunk' in args.parts]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parts', nargs='+', default=['gconv', 'stem', 'trunk'], choices=['gconv', 'stem', 'trunk'])
    ap.add_argument('--models', nargs='+', default=list(TRUNKS), choices=list(TRUNKS))
    ap.add_argument('--batches', nargs='+', type=int, default=[32, 1])
    ap.add_argument('--size', type=int, default=641)
    ap.add_argument('--steps', type=int, default=3, help='forwards per round of a whole network')
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
        if part == 'gconv':
            for layer in layers(name, args.size):
                print(json.dumps(gconv_case(args, name, layer, int(batch))), flush=True)
        elif part == 'stem':
            for pooled in (False, True):
                print(json.dumps(stem_case(args, int(batch), pooled)), flush=True)
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
