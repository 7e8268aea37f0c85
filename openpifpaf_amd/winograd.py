"""3x3 stride-1 convolutions of the float32 trunk as Winograd F(2x2, 3x3) (HIP, ``csrc/winograd.hip``).

The reference runs its ResNet bottlenecks through ``torch.nn.Conv2d`` (``network/basenetworks.py:71-150``); at 641 px the
thirteen stride-1 3x3 convolutions of ResNet-50 are half of the float32 step.  ``conv3x3`` computes the same convolution
with 16 instead of 36 multiplications per 2x2 outputs, in float32 throughout; the filter side ``G g G^T`` is computed once
per weight, in float64, and stored in the order the kernel's lanes read it.
"""
import os

import torch

from . import _lib, fused

# variant -> (K-chunk, 32-wide channel blocks per workgroup): must match launch_winograd_f23 (csrc/winograd.hip)
VARIANTS = {0: (16, 2), 1: (8, 1), 2: (16, 2), 3: (16, 2), 4: (16, 2),     # 2: variant 0's tile and filter layout, eight waves
            5: (16, 4)}     # 5: variant 4's 128-channel workgroups, forced (variant 4 picks them by the launcher's rule)
DEFAULT_VARIANT = 2         # eight waves in two shifts (csrc/winograd.hip): 5-8 % faster than variant 0 on every ResNet-50 shape
X3_VARIANT = 4              # variant 2 on the bf16 MFMA pipe with exactly split operands (opa_conv3x3_winograd_f32x3)
# OPA_WINO_X3=0: the network's Winograd convolutions stay on variant 2 (float32 MFMA) -- read ONCE, at import; the two round
# differently, so it is a switch for a whole job, never a per-call choice
X3 = fused._switch('OPA_WINO_X3', '1')
MIN_WORKGROUPS = 256        # below one workgroup per compute unit the launch does not fill the chip: MIOpen's convolution
_G = ((1.0, 0.0, 0.0), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5), (0.0, 0.0, 1.0))


_mode = os.environ.get('OPA_CONV3X3', 'auto')      # read ONCE, when the module is imported; set_mode() afterwards
if _mode not in ('auto', 'conv', 'winograd'):
    raise ValueError('OPA_CONV3X3 must be auto, conv or winograd, not %r' % _mode)


def set_mode(mode):
    """'auto' (the shape rule of :func:`takes`), 'conv' (always MIOpen's convolution) or 'winograd' (the kernel wherever the
    operands qualify, however small the launch) -> the previous mode.  The two paths round differently: a job's ranks must agree."""
    global _mode
    if mode not in ('auto', 'conv', 'winograd'):
        raise ValueError(mode)
    previous, _mode = _mode, mode
    return previous


def get_mode():
    return _mode


def workgroups(x_shape, c_out, variant=DEFAULT_VARIANT):
    B, _, H, W = x_shape
    return ((B * ((H + 1) // 2) * ((W + 1) // 2) + 63) // 64) * (c_out // (32 * VARIANTS[variant][1]))


def takes(conv, x, u, variant=DEFAULT_VARIANT):
    """True if the Winograd kernel runs ``conv(x)`` for this bias-free 3x3 ``torch.nn.Conv2d``: ``u`` says that the kernel may (its
    transformed filter, or True where the operand is derived from ``conv.weight`` at the launch, :func:`filter_of`; None or False:
    it may not), the operands qualify and the launch fills the chip -- a rule on shapes, not a timing, so that every rank of a job
    and every run take the same path (the two round differently); :func:`set_mode` (default: ``OPA_CONV3X3`` at import) forces one."""
    forced = _mode
    return (u is not None and u is not False and forced != 'conv' and (u is True or u.dtype == torch.float32) and conv.bias is None
            and supported(x, conv.weight, variant, conv.stride, conv.padding, conv.groups, conv.dilation)
            and (forced == 'winograd' or workgroups(x.shape, conv.out_channels, variant) >= MIN_WORKGROUPS)
            and not (torch.is_grad_enabled() and (x.requires_grad or conv.weight.requires_grad)))


def run(conv, x, u=True, bias=None, relu=False):
    """``conv(x)`` (+ bias, ReLU) through the kernel, where :func:`takes` holds: variant 4 on the split planes of the CURRENT
    ``conv.weight`` (:func:`split_filter_of`), or with ``OPA_WINO_X3=0`` variant 2 on its transformed filter (:func:`filter_of`;
    a tensor passed as ``u`` is taken as that filter instead)."""
    if X3:
        return conv3x3_x3(x, split_filter_of(conv), conv.out_channels, bias=bias, relu=relu)
    return conv3x3(x, filter_of(conv) if u is True else u, conv.out_channels, bias=bias, relu=relu, variant=DEFAULT_VARIANT)


def conv_or_fallback(conv, x, u, variant=DEFAULT_VARIANT):
    """``conv(x)``: through the kernel where :func:`takes` says so, else the module itself (MIOpen)."""
    if takes(conv, x, u, variant):
        return run(conv, x, u)
    return conv(x)


def supported(x, weight, variant=0, stride=(1, 1), padding=(1, 1), groups=1, dilation=(1, 1)):
    kc, nb = VARIANTS[variant]
    return (x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and x.dim() == 4
            and tuple(weight.shape[2:]) == (3, 3) and tuple(stride) == (1, 1) and tuple(padding) == (1, 1)
            and groups == 1 and tuple(dilation) == (1, 1) and weight.shape[1] == x.shape[1]
            and x.is_contiguous(memory_format=torch.channels_last)
            and weight.shape[1] % kc == 0 and weight.shape[0] % (32 * nb) == 0
            and x.numel() < 2 ** 30 and x.data_ptr() % 16 == 0 and _lib.available())     # (32-bit byte offsets)


def transform_filter(weight, variant=0):
    """``[C_out, C_in, 3, 3]`` -> the kernel's operand: U = G g G^T per (c_out, c_in) in float64, rounded to float32 once,
    laid out ``[channel block][K-chunk][position 16][j][kq][lane 64][4]`` -- lane ``l`` of a wave multiplies
    ``U[k = 2 * (4 * kq + e) + l // 32][c = 32 * j + l % 32]`` in its e-th MFMA of group kq, so a lane's four values are
    one 16-byte load and a wave's load is 1 KB contiguous."""
    kc, nb = VARIANTS[variant]
    cout, cin = weight.shape[:2]
    g = torch.tensor(_G, dtype=torch.float64, device=weight.device)
    u = torch.einsum('ar,oirs,bs->aboi', g, weight.detach().double(), g)        # [4, 4, cout, cin]
    u = u.permute(0, 1, 3, 2).reshape(16, cin, cout)                            # [position, k, c]
    u = u.reshape(16, cin // kc, kc // 8, 4, 2, cout // (32 * nb), nb, 32)      # [pos, chunk, kq, e, khalf, block, j, c]
    u = u.permute(5, 1, 0, 6, 2, 4, 7, 3)                                       # [block, chunk, pos, j, kq, khalf, c, e]
    return u.contiguous().float().reshape(-1)


def split_filter(weight):
    """``[C_out, C_in, 3, 3]`` -> the operand of variant 4: ``U = transform_filter(weight, 2)`` (the same float32 numbers variant 2
    multiplies) cut exactly into three bfloat16 planes (``fused.split_weight``: ``u1 + u2 + u3 == U`` bit for bit), laid out
    ``[channel block][K-chunk][position 16][j][piece 3][lane 64][8]``: element ``e`` of lane ``l`` is piece ``q`` of
    ``U[k = 2 e + l // 32][c = 32 j + l % 32]`` of the chunk -- the bf16 fragment of virtual k' = 8 (l // 32) + e, i.e. the chunk's
    K permutation k' = 8 h + e <-> k = 2 e + h, which the kernel applies to the pixel operand alike.  A wave's load of one piece
    is 1 KB contiguous."""
    cout, cin = weight.shape[:2]
    u = transform_filter(weight, DEFAULT_VARIANT)
    u = u.reshape(cout // 64, cin // 16, 16, 2, 2, 64, 4).permute(0, 1, 2, 3, 5, 4, 6)    # [.., j, kq, lane, e] -> [.., j, lane, kq, e]
    planes = fused.split_weight(u)                                                       # [3, block, chunk, pos, j, lane, kq, e]
    return planes.permute(1, 2, 3, 4, 0, 5, 6, 7).contiguous().reshape(-1)


def split_filter_of(conv):
    """``split_filter(conv.weight)``, kept on the module and computed again whenever the weight was replaced, moved, converted or
    changed in place (``load_state_dict`` into an optimized network): ``fused.derived``'s key (data pointer, version counter, device,
    dtype)."""
    return fused.derived(conv, '_opa_wino_u3', (conv.weight,), lambda: split_filter(conv.weight))


def filter_of(conv):
    """``transform_filter(conv.weight, 2)`` in the weight's dtype -- variant 2's operand -- kept on the module and kept current
    like :func:`split_filter_of` (a snapshot taken when the network was optimized would outlive ``load_state_dict``)."""
    return fused.derived(conv, '_opa_wino_u', (conv.weight,),
                         lambda: transform_filter(conv.weight, DEFAULT_VARIANT).to(conv.weight.dtype))


# direct-convolution flops of the launches that went through the kernel since the last reset: a measurement (bench.py) that
# quotes a convolutional network's FLOP/s has to say how many of its multiplications F(2x2, 3x3) did not execute
_direct_flops = 0.0


def reset_flop_counter():
    global _direct_flops
    _direct_flops = 0.0


def direct_flops():
    """Flops (2 x MACs of the DIRECT form) of the convolutions run by the kernel since ``reset_flop_counter``; the kernel's
    MFMAs execute 1 / 2.25 of them."""
    return _direct_flops


def _run_kernel(symbol, x, u, c_out, bias, relu, variant, order, out):
    """One launch of either entry point (they take the same arguments), counted in ``direct_flops``."""
    global _direct_flops
    B, cin, H, W = x.shape
    _direct_flops += 18.0 * B * H * W * cin * c_out
    if out is None:
        out = fused._empty_nhwc(x, c_out, dtype=torch.float32)
    fused._launch(symbol, fused._ptr(x), fused._ptr(u), fused._ptr(bias), fused._ptr(out), B, H, W, cin, c_out, int(bool(relu)),
                  variant, order)
    return out


def conv3x3(x, u, c_out, bias=None, relu=False, variant=0, order=0, out=None):
    """``conv2d(x, weight, padding=1)`` (+ bias, ReLU) for the ``u = transform_filter(weight, variant)`` of a 3x3 weight.
    ``x``: ``[B, C_in, H, W]`` float32 channels_last on the GPU -> ``[B, c_out, H, W]`` channels_last."""
    return _run_kernel('opa_conv3x3_winograd_f32', x, u, c_out, bias, relu, variant, order, out)


def conv3x3_x3(x, u3, c_out, bias=None, relu=False, variant=X3_VARIANT, order=0, out=None):
    """:func:`conv3x3` through variant 4 (bf16 MFMA pipe, exactly split operands) for ``u3 = split_filter(weight)``."""
    return _run_kernel('opa_conv3x3_winograd_f32x3', x, u3, c_out, bias, relu, variant, order, out)


def reference_f23(x, weight):
    """The same algorithm in plain PyTorch (float64 on the CPU): the model the CPU tests check the transform matrices and
    the filter layout against, tile by tile like the kernel.  ``x`` ``[B, C, H, W]`` -> ``[B, C_out, H, W]``."""
    x = x.double()
    B, C, H, W = x.shape
    th, tw = (H + 1) // 2, (W + 1) // 2
    xp = torch.zeros((B, C, 2 * th + 2, 2 * tw + 2), dtype=torch.float64)
    xp[:, :, 1:H + 1, 1:W + 1] = x
    bt = torch.tensor(((1, 0, -1, 0), (0, 1, 1, 0), (0, -1, 1, 0), (0, 1, 0, -1)), dtype=torch.float64)
    at = torch.tensor(((1, 1, 1, 0), (0, 1, -1, -1)), dtype=torch.float64)
    g = torch.tensor(_G, dtype=torch.float64)
    u = torch.einsum('ar,oirs,bs->aboi', g, weight.double(), g)
    tiles = xp.unfold(2, 4, 2).unfold(3, 4, 2)                                   # [B, C, th, tw, 4, 4]
    v = torch.einsum('ai,bcyxij,dj->adbcyx', bt, tiles, bt)                       # [4, 4, B, C, th, tw]
    m = torch.einsum('adoc,adbcyx->adboyx', u, v)
    yt = torch.einsum('pa,adboyx,qd->boypxq', at, m, at)                          # [B, O, th, 2, tw, 2]
    return yt.reshape(B, -1, 2 * th, 2 * tw)[:, :, :H, :W]
