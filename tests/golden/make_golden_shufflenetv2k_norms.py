"""Writes ``tests/golden/shufflenetv2k_norms.npz``: the reference's own ``ShuffleNetV2K`` class (``network/basenetworks.py:245-400``)
under ``layer_norm`` as ``--shufflenetv2k-instance-norm`` and ``--shufflenetv2k-group-norm`` set it (``:395-400``), and the group norm
with LeakyReLU, on a tiny network, in float64.

Run in the build container (needs the reference's Python package, ``oracle/reference_python.py``):
``python tests/golden/make_golden_shufflenetv2k_norms.py``.  Written the way ``make_golden_shufflenetv2k_options.py`` writes its file,
whose key mapping this uses: per variant ``<variant>/keys`` (the IN-TREE state-dict keys), ``<variant>/sizes`` and ``<variant>/w``
(float32 values, flattened one behind the other), the reference's float64 output ``<variant>/out`` on the shared input ``x``
``[1, 3, 33, 25]``.  Running statistics (the instance norm's) and affine terms are drawn at random.  ``group_leaky`` computes with the
weights of ``group`` (``group_leaky/w_from`` names the variant; the file stays below the size limit for a committed file).  Arrays only.

The widths are ones the reference's group rule divides: 24, 32 and 64 (4 groups), 116 and 232 (29 groups: 4 and 8 channels each), 128
(32 groups)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

from oracle import reference_python                          # noqa: E402
from openpifpaf_amd import network                           # noqa: E402
from make_golden_shufflenetv2k_options import in_tree_key    # noqa: E402

REPEATS, CHANNELS = [1, 1, 1], [24, 232, 64, 256, 24]
# variant -> (layer norm, LeakyReLU, the variant whose weights it computes with)
VARIANTS = {'instance': ('instance', False, None), 'group': ('group', False, None), 'group_leaky': ('group', True, 'group')}
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'shufflenetv2k_norms.npz')


def reference_layer_norm(kind):
    """What the reference's ``configure`` assigns (``network/basenetworks.py:395-400``)."""
    if kind == 'instance':
        return lambda x: torch.nn.InstanceNorm2d(x, affine=True, track_running_stats=True)
    return lambda x: torch.nn.GroupNorm((32 if x % 32 == 0 else 29) if x > 100 else 4, x)


def main():
    reference_python.load()
    from openpifpaf.network import basenetworks
    basenetworks.torchvision.models.shufflenetv2.channel_shuffle = network._channel_shuffle
    cls = basenetworks.ShuffleNetV2K
    defaults = dict(input_conv2_stride=0, input_conv2_outchannels=None, stage4_dilation=1, kernel_width=5, conv5_as_stage=False,
                    non_linearity=None, layer_norm=None)
    g = torch.Generator().manual_seed(2025)
    x = torch.randn((1, 3, 33, 25), generator=g)
    arrays, drawn = {'x': x.numpy()}, {}
    for variant, (kind, leaky, w_from) in VARIANTS.items():
        attrs = dict(defaults, layer_norm=reference_layer_norm(kind))
        if leaky:
            attrs['non_linearity'] = lambda: torch.nn.LeakyReLU(inplace=True)
        for k, v in attrs.items():
            setattr(cls, k, v)
        try:
            net = cls('tiny', REPEATS, CHANNELS).double().eval()
        finally:
            for k, v in defaults.items():
                setattr(cls, k, v)
        keys, flat, eps = [], [], set()
        with torch.no_grad():
            for m in net.modules():
                if isinstance(m, (torch.nn.InstanceNorm2d, torch.nn.GroupNorm)):
                    eps.add(m.eps)
            for key, t in net.state_dict().items():
                if key.endswith('num_batches_tracked'):
                    continue
                if w_from is not None:
                    v = drawn[w_from][key]
                elif key.endswith('running_var'):
                    v = torch.rand(t.shape, generator=g) * 1.5 + 0.5
                elif key.endswith('running_mean') or key.endswith('bias'):
                    v = torch.randn(t.shape, generator=g) * 0.5
                elif t.dim() == 1:                                   # a norm's weight
                    v = torch.rand(t.shape, generator=g) + 0.5
                else:
                    fan_in = t.shape[1] * t.shape[2] * t.shape[3]
                    v = torch.randn(t.shape, generator=g) * (2.0 / fan_in) ** 0.5
                t.copy_(v.double())                                  # float32 values, float64 arithmetic
                drawn.setdefault(variant, {})[key] = v
                keys.append(in_tree_key(key))
                flat.append(v.numpy().ravel())
            out = net(x.double())
        assert out.dtype == torch.float64 and bool(out.isfinite().all()) and float(out.abs().max()) > 0
        assert len(eps) == 1
        arrays['%s/keys' % variant] = np.array(keys)
        arrays['%s/sizes' % variant] = np.array([len(a) for a in flat], dtype=np.int64)
        if w_from is None:
            arrays['%s/w' % variant] = np.concatenate(flat)
        else:
            arrays['%s/w_from' % variant] = np.array(w_from)
        arrays['%s/eps' % variant] = np.array(sorted(eps), dtype=np.float64)
        arrays['%s/out' % variant] = out.numpy()
        print('%-12s stride %2d out %s max |out| %.3f parameters %d eps %s' % (
            variant, net.stride, tuple(out.shape), float(out.abs().max()), sum(p.numel() for p in net.parameters()), sorted(eps)))
    np.savez_compressed(OUT, **arrays)
    print('wrote %s: %d arrays, %d bytes' % (OUT, len(arrays), os.path.getsize(OUT)))


if __name__ == '__main__':
    main()
