"""Times of the float16 routes of a ResNet cast with ``.half()`` (``fused.F16``: ``csrc/gemm_epilogue.hip``, ``csrc/conv3x3_bf16.hip`` and
``csrc/gemm2_bf16.hip`` instantiated for float16) at 641 px, batch 32 and batch 1, channels-last on one MI355X.

1. The LAYER: every distinct 1x1, 3x3 and tail layer of resnet50 and resnet18, found by running the network once with hooks on its
   blocks and convolutions, three ways on operands of the same values:
   ``f16``    the float16 kernel: ``fused.conv1x1_bias_act`` (1x1), ``fused.conv3x3_bias_act_bf16`` (3x3, with the identity as its
              residual where the layer closes a BasicBlock), ``fused.conv1x1_pair_bias_act_bf16`` (a Bottleneck's conv3 + downsampling
              convolution) or ``fused.conv1x1_strided_bf16`` (a BasicBlock's downsampling convolution alone);
   ``torch``  what runs without the switch: torch's float16 ``nn.Conv2d`` followed by ``fused.bias_act_`` -- for the tail both
              convolutions, the identity as the pass's residual; for the strided 1x1 alone the convolution alone;
   ``bf16``   the same layer in bfloat16 on the bfloat16 instantiation of the same kernel.
   The yardstick is ``torch`` in that run.  ``faster``: the float16 kernel's slowest round is faster than torch's fastest round;
   ``slower``: the reverse.
2. The WHOLE NETWORK, trunk + heads, of resnet50 and resnet18 in float16 (``OPA_CONV1X1=gemm``): the switch on against off.

Device events around a window of calls after ``--warmup`` of each side; the sides alternate in one process, ``--rounds`` rounds give
the spread, medians are reported.  A window of the layer part is ``--kernel-steps`` calls or as many as fill ``--kernel-window-ms``
on the fastest side, whichever is more (``steps`` of the line).  The times are device events AROUND the calls on unchanged inputs -- at
batch 1 the operands stay in the caches for every side.  Every (part, network, batch) runs in a child process of its own under a
``timeout`` of its own, and the first that fails ends the run; one JSON line per layer or network, appended to
``profiles/f16/times.log``.

    python tools/gpu/f16_times.py                               # everything
    python tools/gpu/f16_times.py --parts layer --batches 32
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

LOG = os.path.join(ROOT, 'profiles', 'f16', 'times.log')
MODELS = ('resnet50', 'resnet18')
CL = torch.channels_last
F16, BF16 = torch.float16, torch.bfloat16


def _net(name, dtype=F16):
    return network.optimize_for_inference_(network.factory(name)).cuda().to(dtype).to(memory_format=CL).requires_grad_(False)


def _switches(on):
    fused.F16 = fused.CONV3_BF16 = fused.PAIR_BF16 = on


def layers(name, size):
    """-> [key]: each distinct layer of the trunk once, in the order it runs: ('1x1', c_in, c_out, h, w, with a residual),
    ('3x3', c_in, c_out, stride, dilation, h, w, with a residual), ('tail', k1, k2, n, stride, h_in, w_in) -- a Bottleneck's conv3 +
    downsampling convolution -- and ('strided', k2, n, stride, h_in, w_in), a BasicBlock's downsampling convolution."""
    net, seen = _net(name), []

    def add(key):
        if key not in seen:
            seen.append(key)
    handles = []
    for block in net.modules():
        if isinstance(block, network._Bottleneck):
            tail = block.downsample is not None
            handles.append(block.conv1.register_forward_pre_hook(
                lambda conv, inputs: add(('1x1', conv.in_channels, conv.out_channels) + tuple(inputs[0].shape[2:]) + (False,))))
            handles.append(block.conv2.register_forward_pre_hook(
                lambda conv, inputs: add(('3x3', conv.in_channels, conv.out_channels, conv.stride[0], conv.dilation[0])
                                         + tuple(inputs[0].shape[2:]) + (False,))))
            if tail:
                handles.append(block.register_forward_pre_hook(
                    lambda b, inputs: add(('tail', b.conv3.in_channels, b.downsample[0].in_channels, b.conv3.out_channels,
                                           b.downsample[0].stride[0]) + tuple(inputs[0].shape[2:]))))
            else:
                handles.append(block.conv3.register_forward_pre_hook(
                    lambda conv, inputs: add(('1x1', conv.in_channels, conv.out_channels) + tuple(inputs[0].shape[2:]) + (True,))))
        elif isinstance(block, network._BasicBlock):
            for conv, closing in ((block.conv1, False), (block.conv2, True)):
                handles.append(conv.register_forward_pre_hook(
                    lambda conv, inputs, closing=closing: add(('3x3', conv.in_channels, conv.out_channels, conv.stride[0], conv.dilation[0])
                                                              + tuple(inputs[0].shape[2:]) + (closing,))))
            if block.downsample is not None:
                handles.append(block.downsample[0].register_forward_pre_hook(
                    lambda conv, inputs: add(('strided', conv.in_channels, conv.out_channels, conv.stride[0]) + tuple(inputs[0].shape[2:]))))
    _switches(False)
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


def _image(batch, c, h, w, dtype):
    return torch.randn(batch, c, h, w, device='cuda').relu_().to(dtype).contiguous(memory_format=CL)


def _conv(c_in, c_out, k, stride, dilation, dtype, seed):
    torch.manual_seed(seed)
    pad = dilation if k == 3 else 0
    return nn.Conv2d(c_in, c_out, k, stride, pad, dilation=dilation, bias=False).cuda().to(dtype).requires_grad_(False)


def _sides_of(key, batch, dtype):
    """-> (the kernel's call, torch's call, multiply-adds of the layer) for operands of ``dtype``"""
    kind = key[0]
    torch.manual_seed(0)
    if kind == '1x1':
        _, c, n, h, w, with_residual = key
        conv, x, bias = _conv(c, n, 1, 1, 1, dtype, 1), _image(batch, c, h, w, dtype), (torch.randn(n, device='cuda') * 0.5).to(dtype)
        residual = _image(batch, n, h, w, dtype) if with_residual else None
        w2d = conv.weight.reshape(n, c).contiguous()
        assert fused.conv1x1_supported(x, conv.weight, bias, residual)
        return (lambda: fused.conv1x1_bias_act(x, w2d, bias, residual, True), lambda: fused.bias_act_(conv(x), bias, residual, True),
                batch * h * w * c * n)
    if kind == '3x3':
        _, c, n, s, d, h, w, with_residual = key
        ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
        conv, x, bias = _conv(c, n, 3, s, d, dtype, 1), _image(batch, c, h, w, dtype), (torch.randn(n, device='cuda') * 0.5).to(dtype)
        residual = _image(batch, n, ho, wo, dtype) if with_residual else None
        assert fused.conv3x3_bf16_supported(conv, x, bias, residual)
        return (lambda: fused.conv3x3_bias_act_bf16(conv, x, bias, residual, relu=True), lambda: fused.bias_act_(conv(x), bias, residual, True),
                batch * ho * wo * 9 * c * n)
    if kind == 'tail':
        _, k1, k2, n, s, h, w = key
        ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
        conv, dconv = _conv(k1, n, 1, 1, 1, dtype, 1), _conv(k2, n, 1, s, 1, dtype, 2)
        inner, x, bias = _image(batch, k1, ho, wo, dtype), _image(batch, k2, h, w, dtype), (torch.randn(n, device='cuda') * 0.5).to(dtype)
        assert fused.pair_bf16_supported(conv, dconv, inner, x, bias)
        return (lambda: fused.conv1x1_pair_bias_act_bf16(conv, dconv, inner, x, bias),
                lambda: fused.bias_act_(conv(inner), bias, dconv(x), True), batch * ho * wo * (k1 + k2) * n)
    _, k2, n, s, h, w = key
    ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
    dconv, x = _conv(k2, n, 1, s, 1, dtype, 2), _image(batch, k2, h, w, dtype)
    assert fused.conv1x1_strided_bf16_supported(dconv, x)
    return lambda: fused.conv1x1_strided_bf16(dconv, x), lambda: dconv(x), batch * ho * wo * k2 * n


def layer_case(args, name, key, batch):
    _switches(True)
    f16, theirs, macs = _sides_of(key, batch, F16)
    bf16, _, _ = _sides_of(key, batch, BF16)
    sides = {'f16': f16, 'torch': theirs, 'bf16': bf16}
    with torch.no_grad():
        times, steps = _rounds(sides, args.kernel_steps, args.warmup, args.rounds, args.kernel_window_ms)
        ref = theirs().float()
        delta = float((f16().float() - ref).abs().max()) / float(ref.abs().max())
    t = _median(times['f16'])
    return {'part': 'layer', 'network': name, 'kind': key[0], 'key': list(key[1:]), 'batch': batch, 'size': args.size, 'steps': steps,
            'f16_ms_median': t, 'f16_ms_all': times['f16'], 'torch_ms_median': _median(times['torch']), 'torch_ms_all': times['torch'],
            'bf16_ms_median': _median(times['bf16']), 'bf16_ms_all': times['bf16'],
            'torch_over_f16': _median(times['torch']) / t, 'f16_over_torch': t / _median(times['torch']), 'f16_over_bf16': t / _median(times['bf16']),
            'faster': max(times['f16']) < min(times['torch']), 'slower': min(times['f16']) > max(times['torch']),
            'f16_call_tflops': 2.0 * macs / (t * 1e-3) / 1e12, 'max_rel_delta_f16_vs_torch': delta}


def trunk_case(args, name, batch):
    os.environ['OPA_CONV1X1'] = 'gemm'
    net = _net(name)
    net32 = copy.deepcopy(net).float()
    x = torch.randn(batch, 3, args.size, args.size, device='cuda').to(F16).contiguous(memory_format=CL)
    fused.CONV3_BF16 = fused.PAIR_BF16 = False
    outs = {}

    def side(on):
        def run():
            fused.F16 = on
            outs[on] = net(x)
        return run
    with torch.no_grad():
        times, _ = _rounds({'on': side(True), 'off': side(False)}, args.steps, args.warmup, args.rounds)
        fused.F16 = False
        ref = net32(x.float())

    def rms(which):
        num = sum(float(((a.double() - b.double()) ** 2).sum()) for a, b in zip(outs[which], ref))
        return (num / sum(float((b.double() ** 2).sum()) for b in ref)) ** 0.5
    return {'part': 'trunk', 'model': name, 'batch': batch, 'size': args.size, 'steps': args.steps,
            'f16_on_ms_median': _median(times['on']), 'f16_on_ms_all': times['on'],
            'f16_off_ms_median': _median(times['off']), 'f16_off_ms_all': times['off'],
            'off_over_on': _median(times['off']) / _median(times['on']),
            'faster': max(times['on']) < min(times['off']), 'slower': min(times['on']) > max(times['off']),
            'rms_error_vs_float32_on': rms(True), 'rms_error_vs_float32_off': rms(False)}


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
        if part == 'layer':
            for key in layers(name, args.size):
                print(json.dumps(layer_case(args, name, key, int(batch))), flush=True)
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
