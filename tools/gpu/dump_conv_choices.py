"""Round 6: measures the 1x1-convolution kernel choice (fused.conv_bias_act: MFMA GEMM / epilogue pass + GEMM / MIOpen) for the shapes
of the BASELINE configurations on this GPU and writes the table the package ships (openpifpaf_amd/conv1x1_pinned.json), so that the
ranks of a multi-GPU job run the same kernels without a collective.

    python tools/gpu/dump_conv_choices.py [out.json]

The 'unit' decisions (fused.pick(..., timing=False): the ShuffleNetV2K units and conv5 on the split-operand GEMM's unit mode) are
never timed by the package; this tool is where they are measured -- the WHOLE unit, today's route against the new one, the units
that share a key (a stage's first unit and its other units) summed:

    python tools/gpu/dump_conv_choices.py --units [out.json]      # only these, as table rows + the times behind them
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from openpifpaf_amd import fused, headmeta, network  # noqa: E402

torch.backends.cudnn.benchmark = True
UNIT_CASES = [('shufflenetv2k16', headmeta.cocokp_metas, 1, 641), ('shufflenetv2k16', headmeta.cocokp_metas, 32, 641),
              ('shufflenetv2k30', headmeta.wholebody_metas, 16, 641)]


def time_units(path):
    """Times every 'unit' decision of UNIT_CASES where it is made (a forward pre-hook: the unit's real input, in place in the
    network) and writes the winners as table rows."""
    ms = {}                                                        # key -> [old route, new route], summed over the units sharing it

    def unit_hook(mod, args):
        x = args[0]
        if not mod._unit_route_supported(x):
            return
        last = mod.branch2[5]
        key = ('torch.float32/unit', fused.out_pixels(x, mod.branch2[3].stride[0]), last.in_channels, last.out_channels, True, False)
        t = ms.setdefault(key, [0.0, 0.0])
        t[0] += fused._time_ms(lambda: mod._forward_fused(x))
        t[1] += fused._time_ms(lambda: mod._forward_unit(x))

    def conv5_hook(mod, args):
        x, conv = args[0], mod[0]
        if not fused.unit_conv_x3_supported(conv, x):
            return
        t = ms.setdefault(('torch.float32/unit', fused.out_pixels(x), conv.in_channels, conv.out_channels, False, False),
                          [0.0, 0.0])
        t[0] += fused._time_ms(lambda: mod[2](mod[0](x)))
        t[1] += fused._time_ms(lambda: fused.conv1x1_unit_x3(conv, x))

    fused.FORCE_PICK = 'conv'                                       # (the forward itself goes on along today's route)
    for name, metas, B, edge in UNIT_CASES:
        model = network.optimize_for_inference_(network.factory(name, list(metas())).cuda()).to(memory_format=torch.channels_last)
        for m in model.modules():
            if isinstance(m, network._InvertedResidualK):
                m.register_forward_pre_hook(unit_hook)
        model.base_net.conv5.register_forward_pre_hook(conv5_hook)
        x = torch.randn((B, 3, edge, edge), device='cuda').contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            model(x)
        torch.cuda.synchronize()
        print(name, B, edge, len(ms), flush=True)
        del model, x
        torch.cuda.empty_cache()
    rows = []
    for key, (old, new) in sorted(ms.items(), key=lambda kv: str(kv[0])):
        rows.append(list(key) + ['x3' if new <= old else 'conv'])
        print('%-60s conv %8.3f ms  x3 %8.3f ms  -> %s' % (key, old, new, rows[-1][-1]), flush=True)
    os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
    json.dump({'device': torch.cuda.get_device_name(0), 'columns': ['dtype', 'M', 'K', 'N', 'residual', 'a_bias', 'choice'], 'table': rows,
               'ms': [list(k) + v for k, v in sorted(ms.items(), key=lambda kv: str(kv[0]))]}, open(path, 'w'), indent=0)
    print('wrote', path, len(rows), 'entries')


if len(sys.argv) > 1 and sys.argv[1] == '--units':
    time_units(sys.argv[2] if len(sys.argv) > 2 else 'unit_choices.json')
    sys.exit(0)
out = sys.argv[1] if len(sys.argv) > 1 else 'gpurun_out/conv1x1_pinned.json'
fused.set_choices({}, replace=True)
cases = [('resnet50', headmeta.cocokp_metas, 32, 641), ('resnet50', headmeta.cocokp_metas, 1, 641), ('resnet50', headmeta.cocokp_metas, 16, 641),
         ('resnet50', headmeta.cocokp_metas, 8, 641), ('resnet50', headmeta.cocokp_metas, 4, 641), ('resnet50', headmeta.cocokp_metas, 2, 641),
         ('resnet18', headmeta.cocokp_metas, 1, 321), ('shufflenetv2k16', headmeta.cocokp_metas, 32, 641),
         ('shufflenetv2k30', headmeta.wholebody_metas, 16, 641)]
for name, metas, B, edge in cases:
    for dtype in (torch.float32, torch.bfloat16):
        model = network.factory(name, list(metas())).cuda()
        network.optimize_for_inference_(model)
        model = model.to(memory_format=torch.channels_last)
        if dtype != torch.float32:
            model = model.to(dtype)
        x = torch.randn((B, 3, edge, edge), device='cuda', dtype=dtype).contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            for _ in range(2):
                model(x)
        torch.cuda.synchronize()
        print(name, B, edge, dtype, len(fused.choices()), flush=True)
        del model, x
        torch.cuda.empty_cache()
table = [list(k) + [v] for k, v in sorted(fused.choices().items(), key=lambda kv: str(kv[0]))]
os.makedirs(os.path.dirname(out) or '.', exist_ok=True)
json.dump({'device': torch.cuda.get_device_name(0), 'columns': ['dtype', 'M', 'K', 'N', 'residual', 'a_bias', 'choice'], 'table': table},
          open(out, 'w'), indent=0)
print('wrote', out, len(table), 'entries')
