"""Error of the SqueezeNet trunk (with the cocokp heads) against its float64 model with six and with nine terms in the Fire route
(``fused.FIRE_TERMS``), next to the error of torch's own float32 forward (``e0``): max and rms relative to the largest reference
value, and the regression slope of the error on the reference value -- a coherent shrink of the output shows as a negative slope.
Three seeds, an odd and an even input size, the heads' convolutions on the split-operand kernel (``X3_TERMS`` = 6) and on MIOpen.
The run behind ``FIRE_TERMS = 9`` is kept in ``profiles/squeezenet/terms.log``.

    python tools/gpu/squeezenet_terms.py
"""
import copy
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
from openpifpaf_amd import fused, network  # noqa: E402


def randomize_(module, seed):
    """Kaiming weights and biases of the activations' own size, seeded (the heads' convolutions included)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.Conv2d):
                fan_out = m.out_channels * m.kernel_size[0] * m.kernel_size[1]
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / fan_out) ** 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.5)
    return module.eval()


def errors(got, ref64):
    """(max, rms) of ``got - ref64`` relative to ``max |ref64|``."""
    d = got.double() - ref64
    scale = ref64.abs().max().item()
    return d.abs().max().item() / scale, d.pow(2).mean().sqrt().item() / scale


def slope(got, ref64):
    d = got.double() - ref64
    return float((d * ref64).sum() / (ref64 * ref64).sum())


def main():
    assert torch.cuda.is_available(), 'needs a GPU'
    fused.FIRE = True
    for seed in (7, 8, 9):
        for shape in ((2, 3, 65, 49), (1, 3, 64, 50)):
            net = randomize_(network.factory('squeezenet'), seed)
            x = torch.randn(shape, generator=torch.Generator().manual_seed(seed + 1)).cuda().contiguous(memory_format=torch.channels_last)
            with torch.no_grad():
                ref64 = copy.deepcopy(net).double().cuda()(x.double())
                plain = copy.deepcopy(net).cuda().to(memory_format=torch.channels_last)
                fused.FORCE_PICK = 'conv'
                torch_out = plain(x)
                e0 = [errors(t, r) for t, r in zip(torch_out, ref64)]
                opt = network.optimize_for_inference_(copy.deepcopy(net)).cuda().to(memory_format=torch.channels_last)
                for terms, pick in ((6, 'x3'), (9, 'x3'), (6, 'conv'), (9, 'conv')):
                    fused.FIRE_TERMS, fused.FORCE_PICK = terms, pick
                    for i, (g, r) in enumerate(zip(opt(x), ref64)):
                        err = errors(g, r)
                        print('seed %d %s fire terms %d heads %s head %d | e0 max %.3e rms %.3e | err max %.3e rms %.3e | err/e0 max %.2f rms %.2f | slope %.3e'
                              % (seed, 'x'.join(map(str, shape)), terms, pick, i, e0[i][0], e0[i][1], err[0], err[1], err[0] / e0[i][0],
                                 err[1] / e0[i][1], slope(g, r)), flush=True)
            print('seed %d %s torch float32 | slope head 0 %.3e head 1 %.3e'
                  % (seed, 'x'.join(map(str, shape)), slope(torch_out[0], ref64[0]), slope(torch_out[1], ref64[1])), flush=True)


if __name__ == '__main__':
    main()
