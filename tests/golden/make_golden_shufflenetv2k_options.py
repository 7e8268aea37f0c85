"""Writes ``tests/golden/shufflenetv2k_options.npz``: the reference's own ``ShuffleNetV2K`` class (``network/basenetworks.py:245-400``)
under each of its options, on a tiny network, in float64.

Run in the build container (needs the reference's Python package, ``oracle/reference_python.py``):
``python tests/golden/make_golden_shufflenetv2k_options.py``.  The reference's ``torchvision.models.shufflenetv2.channel_shuffle`` is
not installed there (torchvision is mocked); the in-tree ``network._channel_shuffle`` -- torchvision's four lines -- stands in.

Per variant the file holds the weights under the IN-TREE state-dict keys -- ``<variant>/keys`` (the names), ``<variant>/sizes``
(elements of each) and ``<variant>/w`` (all of them flattened, one behind the other: one array instead of 140 keeps the archive's
directory small); float32 values, which the reference computes with as float64; the reference nests its stem,
``input_block.0.0.weight``, where this tree keeps ``input_block.0.weight`` and puts the second input convolution at
``input_block.3`` -- and the reference's float64 output (``<variant>/out``) on the shared input ``x`` ``[1, 3, 65, 49]``.
Arrays only."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import reference_python        # noqa: E402
from openpifpaf_amd import network         # noqa: E402

REPEATS, CHANNELS = [2, 2, 2], [4, 8, 16, 32, 32]
# variant -> the reference's class attributes
VARIANTS = {
    'default': {},
    'dilation2': dict(stage4_dilation=2),
    'dilation4': dict(stage4_dilation=4),
    'conv2_stride2': dict(input_conv2_stride=2),
    'conv2_stride1': dict(input_conv2_stride=1),
    'conv2_out6': dict(input_conv2_stride=2, input_conv2_outchannels=6),
    'kernel3': dict(kernel_width=3),
    'kernel7': dict(kernel_width=7),
    'conv5_stage': dict(conv5_as_stage=True),
    'conv5_stage_dilation2': dict(conv5_as_stage=True, stage4_dilation=2),
    'leaky_relu': dict(leaky_relu=True),
}
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'shufflenetv2k_options.npz')


def in_tree_key(key):
    """The reference's ``input_block.<i>.<j>.*`` -> this tree's ``input_block.<j>.*`` (i = 0) / ``input_block.3.<j>.*`` (i = 1)."""
    parts = key.split('.')
    if parts[0] == 'input_block':
        parts = ['input_block'] + ([parts[2]] if parts[1] == '0' else ['3', parts[2]]) + parts[3:]
    return '.'.join(parts)


def main():
    reference_python.load()
    from openpifpaf.network import basenetworks
    basenetworks.torchvision.models.shufflenetv2.channel_shuffle = network._channel_shuffle
    cls = basenetworks.ShuffleNetV2K
    defaults = dict(input_conv2_stride=0, input_conv2_outchannels=None, stage4_dilation=1, kernel_width=5, conv5_as_stage=False,
                    non_linearity=None)
    g = torch.Generator().manual_seed(2024)
    x = torch.randn((1, 3, 65, 49), generator=g)
    arrays = {'x': x.numpy()}
    for variant, options in VARIANTS.items():
        attrs = dict(defaults, **options)
        if attrs.pop('leaky_relu', False):
            attrs['non_linearity'] = lambda: torch.nn.LeakyReLU(inplace=True)
        for k, v in attrs.items():
            setattr(cls, k, v)
        try:
            net = cls('tiny', REPEATS, CHANNELS).double().eval()
        finally:
            for k, v in defaults.items():
                setattr(cls, k, v)
        keys, flat = [], []
        with torch.no_grad():
            for key, t in net.state_dict().items():
                if key.endswith('num_batches_tracked'):
                    continue
                if key.endswith('running_var'):
                    v = torch.rand(t.shape, generator=g) * 1.5 + 0.5
                elif key.endswith('running_mean') or key.endswith('bias'):
                    v = torch.randn(t.shape, generator=g) * 0.5
                elif t.dim() == 1:                                   # a batch norm's weight
                    v = torch.rand(t.shape, generator=g) + 0.5
                else:
                    fan_in = t.shape[1] * t.shape[2] * t.shape[3]
                    v = torch.randn(t.shape, generator=g) * (2.0 / fan_in) ** 0.5
                t.copy_(v.double())                                  # float32 values, float64 arithmetic
                keys.append(in_tree_key(key))
                flat.append(v.numpy().ravel())
            out = net(x.double())
        assert out.dtype == torch.float64 and bool(out.isfinite().all()) and float(out.abs().max()) > 0
        arrays['%s/keys' % variant] = np.array(keys)
        arrays['%s/sizes' % variant] = np.array([len(a) for a in flat], dtype=np.int64)
        arrays['%s/w' % variant] = np.concatenate(flat)
        arrays['%s/out' % variant] = out.numpy()
        print('%-24s stride %2d out %s max |out| %.3f parameters %d' % (
            variant, net.stride, tuple(out.shape), float(out.abs().max()), sum(p.numel() for p in net.parameters())))
    np.savez_compressed(OUT, **arrays)
    print('wrote %s: %d arrays, %d bytes' % (OUT, len(arrays), os.path.getsize(OUT)))


if __name__ == '__main__':
    main()
