"""What one forward of an optimized ResNet trunk launches and computes, for comparing two versions of the Python route layer on ONE
built library: for resnet18 and resnet50 in float32, resnet50 in bfloat16 with ``CONV3_BF16`` on, resnet50 with a dilated block 5 in
float32 and resnext50 in float32 with ``GCONV`` on -- each at a fixed seed on ``[2, 3, 97, 65]``, with ``FORCE_PICK='x3'``, Winograd
mode 'winograd', an empty choice table and ``OPA_CONV1X1=gemm`` (nothing is timed) -- the launch trace (every symbol with its
arguments, an address as null / ptr, and ``miopen:<module>`` for every ``nn.Conv2d`` that was called) and the SHA-256 of the output's
bytes.

    python tools/gpu/resnet_route_digests.py --out A.json [--sources DIR]   # DIR: where the ``openpifpaf_amd`` sources to import lie
    python tools/gpu/resnet_route_digests.py --compare PARENT.json PARENT_AGAIN.json NEW.json

``--sources`` other than this tree: the library is this tree's (``OPA_LIB_PATH``).  The outputs themselves go to ``<out>.pt``.
``--compare``: traces must be equal everywhere; digests must be equal where no MIOpen step is on the route (MIOpen's split-K solver
does not repeat: ``tests/test_gpu_trunk_routes.py``'s ``rec``); where one is, the largest difference NEW - PARENT must not exceed
PARENT_AGAIN - PARENT.  Exit status 1 if any of that does not hold.  ``profiles/resnet_routes/`` keeps what was measured."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
# name -> (configuration, options, dtype, switches that are on)
CASES = {'resnet18-float32': ('resnet18', {}, 'float32', ()),
         'resnet50-float32': ('resnet50', {}, 'float32', ()),
         'resnet50-bfloat16-conv3_bf16': ('resnet50', {}, 'bfloat16', ('CONV3_BF16',)),
         'resnet50-dilated-float32': ('resnet50', {'block5_dilation': 2}, 'float32', ()),
         'resnext50-float32-gconv': ('resnext50', {}, 'float32', ('GCONV',))}


def record(args):
    os.environ['OPA_CONV1X1'] = 'gemm'
    sources = os.path.abspath(args.sources)
    if sources != ROOT:
        os.environ.setdefault('OPA_LIB_PATH', os.path.join(ROOT, 'openpifpaf_amd', 'lib', 'libopenpifpaf_amd.so'))
    sys.path.insert(0, sources)
    import torch
    from torch import nn
    from openpifpaf_amd import fused, network, winograd
    assert os.path.dirname(os.path.dirname(os.path.abspath(network.__file__))) == sources, network.__file__
    assert torch.cuda.is_available(), 'needs a GPU'
    trace, launch = [], fused._launch

    def recording_launch(symbol, *a):
        trace.append('%s(%s)' % (symbol, ', '.join('null' if v is None else 'ptr' if isinstance(v, int) and v >= 2 ** 32 else str(v)
                                                   for v in a)))
        return launch(symbol, *a)
    fused._launch = recording_launch
    fused.FORCE_PICK = 'x3'
    winograd.set_mode('winograd')
    result, tensors = {}, {}
    for name, (config, options, dtype, switches) in CASES.items():
        fused.set_choices({}, replace=True)
        for switch in ('CONV3_BF16', 'GCONV'):
            setattr(fused, switch, switch in switches)
        torch.manual_seed(1)
        net = network.Resnet(config, **options).eval()
        g = torch.Generator().manual_seed(2)
        with torch.no_grad():
            for m in net.modules():                 # batch norms far from the identity: the folded biases are of the activations' size
                if isinstance(m, nn.BatchNorm2d):
                    m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.5)
                    m.running_var.copy_(torch.rand(m.num_features, generator=g) * 1.5 + 0.5)
                    m.weight.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                    m.bias.copy_(torch.randn(m.num_features, generator=g) * 0.5)
        net = network.optimize_for_inference_(net).to(getattr(torch, dtype)).cuda().to(memory_format=torch.channels_last)
        for module_name, m in net.named_modules():
            if isinstance(m, nn.Conv2d):
                m.register_forward_hook(lambda mod, a, out, n=module_name: trace.append('miopen:' + n))
        x = torch.randn((2, 3, 97, 65), generator=torch.Generator().manual_seed(3)).to(getattr(torch, dtype))
        x = x.cuda().contiguous(memory_format=torch.channels_last)
        del trace[:]
        with torch.no_grad():
            out = net(x)
        torch.cuda.synchronize()
        out = out.float().contiguous().cpu()
        assert bool(out.isfinite().all())
        result[name] = {'sha256': hashlib.sha256(out.numpy().tobytes()).hexdigest(), 'trace': list(trace)}
        tensors[name] = out
        print('%s: output %s sha256 %s, %d launches, %d of them MIOpen\'s' % (
            name, list(out.shape), result[name]['sha256'], len(trace), sum(t.startswith('miopen:') for t in trace)))
        for t in trace:
            print('    ' + t)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
    torch.save(tensors, args.out + '.pt')
    return 0


def compare(paths):
    import torch
    parent, again, new = (json.load(open(p)) for p in paths)
    tp, ta, tn = (torch.load(p + '.pt') for p in paths)
    bad = 0
    print('| network | launches (MIOpen\'s) | traces equal | digest parent / parent again / new | max abs difference parent again - parent | new - parent | verdict |')
    print('|---|---|---|---|---|---|---|')
    for name in parent:
        trace = parent[name]['trace']
        miopen = sum(t.startswith('miopen:') for t in trace)
        same_trace = trace == again[name]['trace'] == new[name]['trace']
        d_again, d_new = float((ta[name] - tp[name]).abs().max()), float((tn[name] - tp[name]).abs().max())
        same_bits = parent[name]['sha256'] == new[name]['sha256']
        ok = same_trace and (same_bits if miopen == 0 else d_new <= d_again)
        bad += not ok
        print('| %s | %d (%d) | %s | %s / %s / %s | %.3e | %.3e | %s |' % (
            name, len(trace), miopen, same_trace, parent[name]['sha256'][:12], again[name]['sha256'][:12], new[name]['sha256'][:12],
            d_again, d_new, 'ok' if ok else 'DIFFERENT'))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', help='record: the JSON file to write (the outputs go to <out>.pt)')
    ap.add_argument('--sources', default=ROOT, help='the directory that holds the openpifpaf_amd package to import')
    ap.add_argument('--compare', nargs=3, metavar=('PARENT', 'PARENT_AGAIN', 'NEW'))
    args = ap.parse_args()
    if args.compare:
        return compare(args.compare)
    assert args.out, 'give --out or --compare'
    return record(args)


if __name__ == '__main__':
    sys.exit(main())
