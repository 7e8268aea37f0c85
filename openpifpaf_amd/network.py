"""Field producers on PyTorch-ROCm: backbones + CompositeField4 heads.

This is the "plumbing" in front of the decode path: plain ``torch.nn`` modules
(MIOpen / hipBLASLt convolutions, no custom kernels) restated without
torchvision, with random initialisation (no checkpoints offline).  Architecture
follows the reference so that the field tensors have the reference's shapes:

* ``Resnet``: torchvision ResNet topology with the input max-pool removed, so
  the overall stride is 16 (reference ``network/basenetworks.py:71-150``,
  factories ``network/factory.py:51-57``); the reference's options put the pool
  back, change the stem's stride, add a second input convolution, dilate
  block 5 or drop it (``network/basenetworks.py:79-142``).
* ``ShuffleNetV2K``: reference ``network/basenetworks.py:186-355`` (k16: stages
  [4,8,4], channels [24,348,696,1392,1392]; k30: [8,16,6], [32,512,1024,2048,2048]); the reference's options add a second
  input convolution, dilate stage 4, change the depthwise kernel's width, make ``conv5`` two units or put a LeakyReLU in
  place of every ReLU (``network/basenetworks.py:245-400``).
* ``ShuffleNetV2``: torchvision's ``shufflenet_v2_x1_0`` / ``_x2_0`` without the max-pool and the classifier, stride 16 (reference
  ``network/basenetworks.py:36-69``): the K unit with a 3x3 window under torchvision's names.
* ``MobileNetV2``: torchvision's ``mobilenet_v2`` features, stride 32 (reference ``network/basenetworks.py:407-430``).
* ``MobileNetV3``: torchvision's ``mobilenet_v3_large`` / ``mobilenet_v3_small`` feature extractors with the stride of the first
  convolution set to 1, stride 16 (reference ``network/basenetworks.py:432-446``, ``network/factory.py:53-56``).
* ``SqueezeNet``: torchvision's ``squeezenet1_1`` features with padding 1 on the stem and on the ceil-mode max-pools, stride 16
  (reference ``network/basenetworks.py:461-487``).
* ``CompositeField4``: 1x1 conv -> PixelShuffle(2) -> crop last row/col -> view
  ``[B, F, C, H, W]`` -> sigmoid / index-add / softplus (reference
  ``network/heads.py:272-378``); 641 px -> 41 -> 82 -> 81.
* ``Shell``: reference ``network/nets.py:11-48``.
"""
import math

import torch
from torch import nn

from . import fused, headmeta, winograd


def _take_biases(block, conv_names):
    """Move the (BN-folded) conv biases of a residual block into buffers ``fb1..`` applied by the
    fused epilogue; the downsample conv's bias is merged into the last one (both are added
    before the block's final ReLU)."""
    for i, name in enumerate(conv_names, 1):
        conv = getattr(block, name)
        bias = conv.bias.detach().clone() if conv.bias is not None else torch.zeros(conv.out_channels)
        if i == len(conv_names) and block.downsample is not None:
            dconv = block.downsample[0]
            if dconv.bias is not None:
                bias = bias + dconv.bias.detach().to(bias.device)
                dconv.bias = None
        conv.bias = None
        block.register_buffer('fb%d' % i, bias)


# The routes of a ResNet's 3x3 convolution in precedence order ("3x3 convolution of a ResNet -> route").  Per row: its
# name; the predicate; the launcher -- ``bare``: the convolution alone, no bias (Winograd: none, the split-operand kernel: a zero
# one) and no ReLU; whether the kernel adds the residual itself; (kind, flag_b) of its ``fused.pick`` against MIOpen + ``bias_act_``,
# or None where it does not compete.  Every row reaches ``fused.*`` / ``winograd.*`` at the call: the route tests put recorders there.
_CONV3_ROUTES = (
    ('wino', lambda c, x, b, r, u: winograd.takes(c, x, u),
     lambda c, x, b, r, u, bare: winograd.run(c, x, u, bias=None if bare else b, relu=not bare), False, None),
    ('x3', lambda c, x, b, r, u: fused.conv3x3_x3_supported(c, x, b),
     lambda c, x, b, r, u, bare: fused.conv3x3_bias_act_x3(c, x, _zero_bias(c, b) if bare else b, not bare), False,
     lambda c, r: ('conv3', False)),
    ('x3-dilated', lambda c, x, b, r, u: c.dilation != (1, 1) and fused.conv3x3_dilated_x3_supported(c, x, b),
     lambda c, x, b, r, u, bare: fused.conv3x3_dilated_bias_act_x3(c, x, _zero_bias(c, b) if bare else b, not bare), False,
     lambda c, r: ('conv3d%d' % c.dilation[0], r is not None)),
    ('gconv', lambda c, x, b, r, u: fused.gconv3x3_supported(c, x, b),
     lambda c, x, b, r, u, bare: fused.gconv3x3_bias_act(c, x, None if bare else b, not bare), False, None),
    # (bfloat16 behind fused.CONV3_BF16 and float16 behind fused.F16: one row for both 16-bit types)
    ('bf16', lambda c, x, b, r, u: fused.conv3x3_bf16_supported(c, x, b, r),
     lambda c, x, b, r, u, bare: fused.conv3x3_bias_act_bf16(c, x, b, r, relu=not bare), True, None),
    # (bfloat16 behind fused.GCONV_BF16 and float16 behind fused.GCONV_F16: one row for both 16-bit types)
    ('gconv-bf16', lambda c, x, b, r, u: fused.gconv3x3_bf16_supported(c, x, b),
     lambda c, x, b, r, u, bare: fused.gconv3x3_bias_act_bf16(c, x, None if bare else b, not bare), False, None),
)


def _zero_bias(conv, bias):
    return fused.derived(conv, '_opa_zero_bias', (conv.weight,), lambda: torch.zeros_like(bias))


def _conv3x3(conv, x, bias, residual=None, *, u=False, defer=False, skip=()):
    """``relu(conv(x) + bias (+ residual))`` for a bias-free 3x3 ``conv`` of a ResNet through the first route of ``_CONV3_ROUTES`` that
    takes it -> (the result, what is still owed).  A kernel without a residual operand runs bare where there is a residual, and
    ``fused.bias_act_`` adds the rest, as behind MIOpen.  ``u``: ``winograd.takes``'s.  No route: MIOpen + ``bias_act_``, nothing owed;
    with ``defer`` MIOpen's raw output, and owed is ``bias``: the caller's next GEMM applies bias + ReLU to its operand (``a_bias``).
    ``skip``: names of routes not to try."""
    for name, takes, run, adds_residual, pick_key in _CONV3_ROUTES:
        if name in skip or not takes(conv, x, bias, residual, u):
            continue
        bare = residual is not None and not adds_residual
        if pick_key is None:                    # (no closure on this path: it is the one every stride-1 block of a float32 step takes)
            return _run_route(run, conv, x, bias, residual, u, bare), None
        (kind, flag_b), s = pick_key(conv, residual), conv.stride[0]
        return fused.pick(kind, fused.out_pixels(x, s), 9 * x.shape[1], conv.out_channels, s > 1, flag_b,
                          lambda: _run_route(run, conv, x, bias, residual, u, bare),
                          lambda: fused.bias_act_(conv(x), bias, residual)), None
    return (conv(x), bias) if defer else (fused.bias_act_(conv(x), bias, residual), None)


def _run_route(run, conv, x, bias, residual, u, bare):
    out = run(conv, x, bias, residual, u, bare)
    return fused.bias_act_(out, bias, residual) if bare else out


class _Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None, groups=1, base_width=64):
        super().__init__()
        width = int(planes * base_width / 64) * groups       # torchvision's rule (ResNeXt: 32 groups of base_width * planes / 64)
        self.conv1 = nn.Conv2d(inplanes, width, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, 3, stride, 1, groups=groups, bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = nn.Conv2d(width, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.fused = False

    def enable_fused_(self):
        _take_biases(self, ('conv1', 'conv2', 'conv3'))
        self._wino = self.conv2.stride == (1, 1)     # the stride-1 3x3 may go to the Winograd kernel
        self.fused = True

    @property
    def wino_u(self):
        """G g G^T of the CURRENT ``conv2.weight`` in the Winograd kernel's operand order (``winograd.filter_of``: derived, cached,
        no part of a checkpoint); no such attribute before ``enable_fused_`` or on a strided block."""
        if not self.__dict__.get('_wino'):
            raise AttributeError('wino_u')
        return winograd.filter_of(self.conv2)

    def forward(self, x):
        if self.fused:      # conv (no bias) -> ONE fused bias(+residual)+ReLU pass each
            out = fused.conv_bias_act(self.conv1, x, self.fb1)            # 1x1: fused MFMA GEMM
            # 3x3: whatever route takes it; where none does, MIOpen's raw output, and conv2's bias + ReLU are owed to the next operand
            out, a_bias = _conv3x3(self.conv2, out, self.fb2, u=self._wino, defer=True)

            def two_launches():
                identity = x if self.downsample is None else self.downsample[0](x)
                # (a_bias: conv2's bias + ReLU applied by the 1x1 GEMM while it stages its operand)
                return fused.conv_bias_act(self.conv3, out, self.fb3, identity, a_bias=a_bias)
            # a block WITH a downsampling convolution, bfloat16 with fused.PAIR_BF16 or float16 with fused.F16: conv3(out) + downsample(x)
            # as ONE launch on the 16-bit MFMA, one rounding; conv2's bias + ReLU applied to the operand where conv2 left them out
            if self.downsample is not None and fused.pair_bf16_supported(self.conv3, self.downsample[0], out, x, self.fb3, a_bias):
                return fused.conv1x1_pair_bias_act_bf16(self.conv3, self.downsample[0], out, x, self.fb3, True, a_bias)
            # a block WITH a downsampling convolution, float32: conv3(out) + downsample(x) as ONE product (the identity tensor
            # is never written), conv2's bias + ReLU applied to the operand where conv2 left them out -- where that is faster
            if self.downsample is not None and fused.pair_supported(self.conv3, self.downsample[0], out, x, self.fb3, a_bias):
                # (written: with a_bias, two_launches may apply conv2's epilogue to ``out`` in place -- once, not once per timed call)
                return fused.pick('pair', fused.out_pixels(out), self.conv3.in_channels + self.downsample[0].in_channels,
                                  self.conv3.out_channels, self.downsample[0].stride[0] > 1, a_bias is not None,
                                  lambda: fused.conv1x1_pair_bias_act_x3(self.conv3, self.downsample[0], out, x, self.fb3, True, a_bias),
                                  two_launches, written=out if a_bias is not None else None)
            return two_launches()
        identity = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        return self.relu(out + identity)


class _BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.fused = False

    def enable_fused_(self):
        _take_biases(self, ('conv1', 'conv2'))
        # stride-1 3x3 of the kernel's channel counts: may go to the Winograd kernel (see _Bottleneck)
        self._wino = tuple(conv.stride == (1, 1) and conv.in_channels % 16 == 0 and conv.out_channels % 64 == 0
                           for conv in (self.conv1, self.conv2))
        self.fused = True

    def _wino_u(self, i):
        if not self.__dict__.get('_wino', (False, False))[i - 1]:
            raise AttributeError('wino_u%d' % i)
        return winograd.filter_of(getattr(self, 'conv%d' % i))

    wino_u1 = property(lambda self: self._wino_u(1), doc='like ``_Bottleneck.wino_u``, of ``conv1``')
    wino_u2 = property(lambda self: self._wino_u(2), doc='like ``_Bottleneck.wino_u``, of ``conv2``')

    # The plain (d = 1) split-operand kernel is not tried, although the strided convolutions of resnet18/34 qualify: the exclusion is
    # inherited from the block's first fused forward and has never been timed.  Lifting it changes what runs: with a measurement.
    _SKIP = ('x3',)

    def forward(self, x):
        if self.fused:
            if self.downsample is None:
                identity = x
            elif fused.conv1x1_strided_bf16_supported(self.downsample[0], x):    # (PAIR_BF16, or F16 for float16:) the strided 1x1 on the 16-bit MFMA
                identity = fused.conv1x1_strided_bf16(self.downsample[0], x)
            else:
                identity = self.downsample[0](x)
            out = _conv3x3(self.conv1, x, self.fb1, u=self._wino[0], skip=self._SKIP)[0]
            return _conv3x3(self.conv2, out, self.fb2, identity, u=self._wino[1], skip=self._SKIP)[0]       # (the 16-bit kernel adds the identity)
        identity = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        return self.relu(out + identity)


class BaseNetwork(nn.Module):
    def __init__(self, name, *, stride, out_features):
        super().__init__()
        self.name = name
        self.stride = stride
        self.out_features = out_features

    fused = False

    def enable_fused_(self):
        """After conv+BN folding: ``forward`` may take the project's kernels; no parameter or buffer changes."""
        self.fused = True


def _dilate_(block5, dilation):
    """Block 5 with dilated convolutions instead of a stride (reference ``network/basenetworks.py:121-135``): every convolution gets
    stride 1, the downsampling 1x1 included, every other one dilation = padding = ``dilation`` (k x k: (k - 1) / 2 times that)."""
    for m in block5.modules():
        if not isinstance(m, nn.Conv2d):
            continue
        m.stride = (1, 1)
        if m.kernel_size[0] == 1:
            continue
        m.dilation = (dilation, dilation)
        m.padding = ((m.kernel_size[0] - 1) // 2 * dilation,) * 2
    return block5


class Resnet(BaseNetwork):
    """ResNet-18/34/50/101/152 and ResNeXt-50 (32x4d) / -101 (32x8d) (reference ``network/factory.py:51-79``) with the reference's
    five options (``network/basenetworks.py:71-183``); each keyword defaults to the class attribute of its name, which
    ``configure`` sets from the command line.  The defaults give stride 16: no input max-pool, stem of stride 2, no dilation.

    * ``pool0_stride``: 0 removes the input max-pool; else ``input_block.3 = MaxPool2d(3, pool0_stride, 1)``, the overall stride
      times 2 (``int(stride * 2 / pool0_stride)`` for a stride other than 2, as the reference counts).
    * ``input_conv_stride`` s: the stem's stride; the overall stride follows it, ``stride * s / 2`` (8 for s = 1: what the network
      does.  The reference writes ``int(stride * 2 / s)`` here, 32 for s = 1, which no head could decode with).
    * ``input_conv2_stride`` s: ``input_block.3 = Sequential(Conv2d(64, 64, 3, s, 1), BatchNorm2d, ReLU)`` in place of the pool (refused
      together with ``pool0_stride``), the overall stride times s (the reference builds this convolution with stride 2 whatever s
      is and counts 2: the same for s = 2, the one value it documents).
    * ``block5_dilation`` d != 1: see ``_dilate_``; the overall stride is halved.
    * ``remove_last_block``: no block 5; the stride and ``out_features`` are halved.  The reference's own ``forward`` would call
      ``None`` here: this one skips the block, the evident intent.  (With ``block5_dilation`` the reference fails on the missing
      block when it is built; here the combination is refused.)"""
    CONFIGS = {
        'resnet18': (_BasicBlock, [2, 2, 2, 2]),
        'resnet34': (_BasicBlock, [3, 4, 6, 3]),
        'resnet50': (_Bottleneck, [3, 4, 6, 3]),
        'resnet101': (_Bottleneck, [3, 4, 23, 3]),
        'resnet152': (_Bottleneck, [3, 8, 36, 3]),
        'resnext50': (_Bottleneck, [3, 4, 6, 3], 32, 4),          # (..., groups, base width)
        'resnext101': (_Bottleneck, [3, 4, 23, 3], 32, 8),
    }
    pool0_stride = 0
    input_conv_stride = 2
    input_conv2_stride = 0
    block5_dilation = 1
    remove_last_block = False
    OPTIONS = ('pool0_stride', 'input_conv_stride', 'input_conv2_stride', 'block5_dilation', 'remove_last_block')

    def __init__(self, name='resnet50', *, pool0_stride=None, input_conv_stride=None, input_conv2_stride=None, block5_dilation=None,
                 remove_last_block=None):
        given = dict(zip(self.OPTIONS, (pool0_stride, input_conv_stride, input_conv2_stride, block5_dilation, remove_last_block)))
        pool0_stride, input_conv_stride, input_conv2_stride, block5_dilation, remove_last_block = (
            getattr(type(self), k) if v is None else v for k, v in given.items())
        block, layers, *grouped = self.CONFIGS[name]
        stride, out_features = 32, 512 * block.expansion             # (the reference's arithmetic, step by step)
        if pool0_stride:
            if pool0_stride != 2:
                stride = int(stride * 2 / pool0_stride)
        else:
            stride //= 2
        if input_conv_stride != 2:
            stride = stride * input_conv_stride // 2
        if input_conv2_stride:
            assert not pool0_stride, 'the second input convolution is a replacement for the input max-pool'
            stride *= input_conv2_stride
        if remove_last_block:
            assert block5_dilation == 1, 'there is no block 5 to dilate'
            stride //= 2
            out_features //= 2
        if block5_dilation != 1:
            stride //= 2
        super().__init__(name, stride=stride, out_features=out_features)
        self.pool0_stride, self.input_conv_stride, self.input_conv2_stride = pool0_stride, input_conv_stride, input_conv2_stride
        self.block5_dilation, self.remove_last_block = block5_dilation, remove_last_block
        self._block_args = dict(zip(('groups', 'base_width'), grouped))
        self.inplanes = 64
        input_modules = [nn.Conv2d(3, 64, 7, input_conv_stride, 3, bias=False), nn.BatchNorm2d(64), nn.ReLU(inplace=True)]
        if pool0_stride:
            input_modules.append(nn.MaxPool2d(3, pool0_stride, 1))
        if input_conv2_stride:
            input_modules.append(nn.Sequential(
                nn.Conv2d(64, 64, 3, input_conv2_stride, 1, bias=False), nn.BatchNorm2d(64), nn.ReLU(inplace=True)))
        self.input_block = nn.Sequential(*input_modules)
        self.block2 = self._make_layer(block, 64, layers[0], 1)
        self.block3 = self._make_layer(block, 128, layers[1], 2)
        self.block4 = self._make_layer(block, 256, layers[2], 2)
        self.block5 = None if remove_last_block else self._make_layer(block, 512, layers[3], 2)
        if block5_dilation != 1:
            _dilate_(self.block5, block5_dilation)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')

    @classmethod
    def cli(cls, parser):
        """The reference's flags (``network/basenetworks.py:152-174``; nothing is pretrained here, so no ``--resnet-no-pretrain``)."""
        group = parser.add_argument_group('ResNet')
        group.add_argument('--resnet-pool0-stride', default=cls.pool0_stride, type=int,
                           help='stride of zero removes the pooling op')
        group.add_argument('--resnet-input-conv-stride', default=cls.input_conv_stride, type=int,
                           help='stride of the input convolution')
        group.add_argument('--resnet-input-conv2-stride', default=cls.input_conv2_stride, type=int,
                           help='stride of the optional 2nd input convolution')
        group.add_argument('--resnet-block5-dilation', default=cls.block5_dilation, type=int,
                           help='use dilated convs in block5')
        group.add_argument('--resnet-remove-last-block', default=False, action='store_true',
                           help='create a network without the last block')

    @classmethod
    def configure(cls, args):
        for option in cls.OPTIONS:             # (a namespace from a parser without these flags leaves the attributes as they are)
            setattr(cls, option, getattr(args, 'resnet_' + option, getattr(cls, option)))

    def _make_layer(self, block, planes, blocks, stride):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(
                nn.Conv2d(self.inplanes, planes * block.expansion, 1, stride, bias=False),
                nn.BatchNorm2d(planes * block.expansion))
        layers = [block(self.inplanes, planes, stride, downsample, **self._block_args)]
        self.inplanes = planes * block.expansion
        layers += [block(self.inplanes, planes, **self._block_args) for _ in range(1, blocks)]
        return nn.Sequential(*layers)

    def enable_fused_(self):
        """The folded biases of the stem and of the second input convolution become buffers (``fb0``, ``fb0_2``) that the fused
        forward hands to whatever kernel applies them."""
        convs = [('fb0', self.input_block[0])]
        if self.input_conv2_stride:
            convs.append(('fb0_2', self.input_block[3][0]))
        for name, conv in convs:
            self.register_buffer(name, conv.bias.detach().clone())
            conv.bias = None
        self.fused = True

    def _pooled(self, x, bias=None):
        """The input max-pool of ``relu(x + bias)`` (``bias`` None: of ``x`` as it is): one HIP kernel for stride 2 where it takes the
        tensor -- with a bias it REPLACES the epilogue pass -- else that pass and ``F.max_pool2d``."""
        if self.pool0_stride == 2 and fused.maxpool3x3_supported(x, bias):
            return fused.maxpool3x3_bias_act_(x, bias, relu=bias is not None)
        return self.input_block[3](x if bias is None else fused.bias_act_(x, bias))

    def _input_block_fused(self, x):
        conv = self.input_block[0]
        pool = bool(self.pool0_stride)
        if fused.stem_x3_supported(conv, x, self.fb0):     # float32: the stem as an implicit GEMM, bias + ReLU inside
            x0 = x
            if pool:                                        # ... and the pool behind either side: torch's raw convolution hands its
                x = fused.pick('stempool', fused.out_pixels(x0, 2), 256, conv.out_channels, True, False,       # epilogue to the pool kernel
                               lambda: self._pooled(fused.stem7x7_bias_act_x3(conv, x0, self.fb0)),
                               lambda: self._pooled(conv(x0), self.fb0))
            else:
                x = fused.pick('stem', fused.out_pixels(x0, 2), 256, conv.out_channels,
                               True, False, lambda: fused.stem7x7_bias_act_x3(conv, x0, self.fb0),
                               lambda: fused.bias_act_(conv(x0), self.fb0))
        elif fused.stem7x7_bf16_supported(conv, x, self.fb0, pool):   # bfloat16 with fused.STEM7_BF16, float16 with fused.STEM7_F16:
            x = fused.stem7x7_bias_act_bf16(conv, x, self.fb0)        # one launch, bias + ReLU inside
            if pool:                                                  # (float16: the pool kernel declines it, F.max_pool2d runs)
                x = self._pooled(x)
        elif pool:                                          # torch's raw convolution (bfloat16, a stem stride other than 2)
            x = self._pooled(conv(x), self.fb0)
        else:
            x = fused.bias_act_(conv(x), self.fb0)
        if self.input_conv2_stride:
            # (the bf16 kernel would take this convolution and was never routed here: left out as inherited, never timed)
            x = _conv3x3(self.input_block[3][0], x, self.fb0_2, skip=('bf16',))[0]
        return x

    def forward(self, x):
        x = self._input_block_fused(x) if getattr(self, 'fused', False) else self.input_block(x)
        x = self.block4(self.block3(self.block2(x)))
        return x if self.block5 is None else self.block5(x)


def _stem_act(nonlin):
    """The activation code and parameter of ``fused.stem_conv3x3_bias_act`` for a stem's non-linearity, or None."""
    kind = type(nonlin)
    if kind is nn.ReLU:
        return fused.ACT_RELU, 0.0
    if kind is nn.Hardswish:
        return fused.ACT_HARDSWISH, 0.0
    if kind is nn.LeakyReLU:
        return fused.ACT_LEAKY_RELU, nonlin.negative_slope
    if kind is nn.ReLU6:
        return fused.ACT_RELU6, 6.0
    return None


def _stem_route(net, conv, nonlin, x, norm=None):
    """``nonlin(conv(x))`` for the 3x3 RGB stem of an optimized ShuffleNetV2K, ShuffleNetV2, MobileNetV2, MobileNetV3 or SqueezeNet (``conv``
    folded with its batch norm: the bias is ``conv.bias``) in one HIP kernel, or None where the route is not taken: ``fused.STEM`` off
    (the default), a network that is not optimized, or a call ``fused.stem_conv3x3_supported`` declines (bfloat16, autocast, the CPU).
    One route for the five families, independent of their own switches; ``x`` in any layout, the result channels-last.

    ``norm``: the module between the two (a ShuffleNetV2K's): anything but an ``Identity`` did not fold into ``conv``, and the route
    declines -- but for a ``GroupNorm`` with ``fused.GN`` on: the kernel computes the convolution alone and ``_norm_act`` the rest."""
    if not (net.fused and fused.STEM and x.is_cuda and isinstance(conv, nn.Conv2d)):
        return None
    if norm is not None and not isinstance(norm, nn.Identity):
        if not (fused.GN and isinstance(norm, nn.GroupNorm) and fused.stem_conv3x3_supported(conv, x)):
            return None
        return _norm_act(norm, nonlin, fused.stem_conv3x3_bias_act(conv, x, act=fused.ACT_NONE))
    act = _stem_act(nonlin)
    if act is None or not fused.stem_conv3x3_supported(conv, x):
        return None
    return fused.stem_conv3x3_bias_act(conv, x, act=act[0], act_param=act[1])


def _layer_norm_of(layer_norm):
    """``ShuffleNetV2K.layer_norm`` -> what builds the norm of ``c`` channels (reference ``network/basenetworks.py:250-259, 395-400``):
    None ``BatchNorm2d``; 'instance' ``InstanceNorm2d`` with affine terms and running statistics (in ``eval()`` the batch-norm formula:
    it folds); 'group' ``GroupNorm`` in 32 groups where ``c`` divides, else 29, and 4 up to 100 channels (torch's own ``ValueError``
    where the count does not divide ``c``)."""
    if layer_norm is None:
        return nn.BatchNorm2d
    if layer_norm == 'instance':
        return lambda c: nn.InstanceNorm2d(c, affine=True, track_running_stats=True)
    if layer_norm == 'group':
        return lambda c: nn.GroupNorm((32 if c % 32 == 0 else 29) if c > 100 else 4, c)
    raise ValueError('layer_norm must be None, \'instance\' or \'group\', not %r' % (layer_norm,))


def _norm_act(norm, nonlin, t):
    """``nonlin(norm(t))`` (``nonlin`` None: the norm alone) behind a convolution that did not absorb ``norm``, IN PLACE on the
    producer's output ``t``: a ``GroupNorm`` followed by nothing or by an activation the kernels have a code for (``_stem_act``)
    through ``fused.group_norm_act`` where ``fused.GN`` is on and ``fused.group_norm_supported`` takes the call, else torch's modules."""
    act = (fused.ACT_NONE, 0.0) if nonlin is None else _stem_act(nonlin)
    if fused.GN and act is not None and fused.group_norm_supported(norm, t):
        return fused.group_norm_act(norm, t, act=act[0], act_param=act[1], out=t)
    t = norm(t)
    return t if nonlin is None else nonlin(t)


def _channel_shuffle(x, groups=2):
    b, c, h, w = x.shape
    return x.view(b, groups, c // groups, h, w).transpose(1, 2).reshape(b, c, h, w)


class _InvertedResidualK(nn.Module):
    """ShuffleNetV2 unit with a k x k depthwise conv (reference ``basenetworks.py:186-268``), optionally dilated (padding
    ``(k - 1) // 2 * dilation``), with ``nn.LeakyReLU`` (slope 0.01) in place of its ReLUs and with the instance or group norm of
    ``ShuffleNetV2K.layer_norm`` in place of its batch norms (``_layer_norm_of``)."""

    def __init__(self, inp, oup, first_in_stage, *, stride=1, kernel_size=5, dilation=1, leaky_relu=False, layer_norm=None):
        super().__init__()
        assert stride in (1, 2) and (stride != 1 or inp == oup or first_in_stage)
        self.first_in_stage = first_in_stage
        self.leaky_relu = bool(leaky_relu)
        bf = oup // 2
        pad = (kernel_size - 1) // 2 * dilation
        act = nn.LeakyReLU if leaky_relu else nn.ReLU
        norm = _layer_norm_of(layer_norm)
        self.branch1 = None
        if first_in_stage:
            self.branch1 = nn.Sequential(
                nn.Conv2d(inp, inp, kernel_size, stride, pad, dilation, groups=inp, bias=False), norm(inp),
                nn.Conv2d(inp, bf, 1, bias=False), norm(bf), act(inplace=True))
        self.branch2 = nn.Sequential(
            nn.Conv2d(inp if first_in_stage else bf, bf, 1, bias=False), norm(bf), act(inplace=True),
            nn.Conv2d(bf, bf, kernel_size, stride, pad, dilation, groups=bf, bias=False), norm(bf),
            nn.Conv2d(bf, bf, 1, bias=False), norm(bf), act(inplace=True))

    fused = False

    def enable_fused_(self):
        """After conv+BN folding: the depthwise convolutions run as one HIP stencil kernel each (bias fused) and
        cat + channel_shuffle as one interleave pass.  Keeps the tap-major copies of the depthwise weights."""
        for branch in (self.branch1, self.branch2):
            if branch is None:
                continue
            for m in branch:
                if isinstance(m, nn.Conv2d) and m.groups == m.in_channels and m.groups > 1:
                    m.register_buffer('w_taps', fused.depthwise_taps(m.weight))
        self.fused = True

    @staticmethod
    def taps_of(conv):
        """``w_taps`` of the CURRENT depthwise weight: the buffer (part of the state dict since it was introduced, so it stays one)
        IS the operand ``fused.derived`` keeps, so it is brought up to date -- in place where the weight was changed in place -- whenever
        the weight was replaced, converted or changed since.  An operand made while a stream is being captured is the graph's and is
        not kept (``fused.derived``): the buffer stays what it was."""
        taps = fused.derived(conv, '_opa_taps', (conv.weight,), lambda: fused.depthwise_taps(conv.weight))
        kept = getattr(conv, '_opa_taps', None)
        if kept is not None and kept[1] is taps and conv.w_taps is not taps:
            conv.w_taps = taps
        return taps

    @staticmethod
    def _dw_ok(m, x):
        """Can the convolution ``m`` of a branch run through the stencil kernel on ``x``?"""
        k, d = m.kernel_size[0], m.dilation[0]
        return (hasattr(m, 'w_taps') and m.weight.dtype == x.dtype and m.padding[0] == m.padding[1] == k // 2 * d
                and fused.dwconv_supported(x, k, m.stride[0], d))

    @staticmethod
    def _dw(m, x):
        return fused.dwconv_bias_act(x, _InvertedResidualK.taps_of(m), m.bias, m.kernel_size[0], m.stride[0], dilation=m.dilation[0])

    @staticmethod
    def _run(branch, x):
        for m in branch:
            x = _InvertedResidualK._dw(m, x) if isinstance(m, nn.Conv2d) and _InvertedResidualK._dw_ok(m, x) else m(x)
        return x

    def _unit_route_supported(self, x):
        """Can the WHOLE unit run on the project's kernels alone (``_forward_unit``)?  Every 1x1 convolution through the unit mode of
        ``x``'s dtype (``fused.unit_mode_of``: the split-operand GEMM's for float32, the bf16 GEMM's behind ``fused.UNIT_BF16`` and
        outside autocast for bfloat16, the same GEMM on the f16 MFMA behind ``fused.UNIT_F16`` for float16), every depthwise convolution
        through the stencil kernel.  The GEMM's epilogue applies the ReLU, or
        the LeakyReLU of a ``leaky_relu`` unit where ``fused.UNIT_LEAKY`` is on and outside autocast: otherwise such a unit takes
        ``_forward_fused``."""
        if fused.unit_mode_of(x) is None or x.dim() != 4:
            return False
        if self.leaky_relu and not (fused.UNIT_LEAKY and not torch.is_autocast_enabled()):
            return False
        if not all(isinstance(m, nn.Identity) for m in self._norms()):      # a norm that did not fold (a GroupNorm) must run
            return False
        return self._convs_supported(x)

    def _norms(self):
        """The modules where the unit was built with norms: ``Identity`` after folding, a ``GroupNorm`` still itself."""
        return ([] if self.branch1 is None else [self.branch1[1], self.branch1[3]]) + [self.branch2[i] for i in (1, 4, 6)]

    def _convs_supported(self, x):
        """Every 1x1 convolution through the unit-mode GEMM of ``x``'s dtype, every depthwise convolution through the stencil kernel?"""
        mode = fused.unit_mode_of(x)
        branches = (self.branch2,) if self.branch1 is None else (self.branch1, self.branch2)
        for branch in branches:
            for m in branch:
                if not isinstance(m, nn.Conv2d):
                    continue
                if m.groups > 1:
                    if not self._dw_ok(m, x):
                        return False
                elif not fused._unit_conv_ok(mode, m):
                    return False
        first = x if self.branch1 is not None else x.chunk(2, dim=1)[1]
        return fused.unit_conv_supported(self.branch2[0], first)

    def _forward_unit(self, x):
        """Three launches (five in a first unit): GEMM + bias + ReLU on the channel slice, the depthwise stencil, GEMM + bias + ReLU
        stored into the shuffled position with the pass-through half copied by the same kernel.  A ``leaky_relu`` unit: the same
        launches with the module's LeakyReLU in the GEMM's epilogue."""
        gemm, b2 = fused.conv1x1_unit, self.branch2
        act = dict(act=fused.ACT_LEAKY_RELU, act_param=b2[2].negative_slope) if self.leaky_relu else {}
        if self.branch1 is None:
            x1, x2 = x.chunk(2, dim=1)
        else:
            x1, x2 = gemm(self.branch1[2], self._dw(self.branch1[0], x), **act), x
        h = self._dw(b2[3], gemm(b2[0], x2, **act))
        return gemm(b2[5], h, partner=x1, **act)

    def _gn_route_supported(self, x):
        """Can the unit of a group-norm network run ``_forward_gn``?  ``fused.GN`` on, float32 outside autocast, every norm a
        ``GroupNorm`` and the convolutions as ``_convs_supported`` says; each norm decides for itself (``_norm_act``)."""
        return (fused.GN and x.dtype == torch.float32 and x.dim() == 4 and not torch.is_autocast_enabled()
                and all(isinstance(m, nn.GroupNorm) for m in self._norms()) and self._convs_supported(x))

    def _forward_gn(self, x):
        """The unit of a group-norm network on the project's kernels: every 1x1 convolution through the unit-mode GEMM without an
        activation, every depthwise convolution through the stencil, every norm -- with the ReLU or LeakyReLU behind it -- through
        the group-norm kernels in place on its producer's output (``_norm_act``), the interleave pass at the end."""
        b1, b2 = self.branch1, self.branch2
        if b1 is None:
            x1, x2 = x.chunk(2, dim=1)
        else:
            h = _norm_act(b1[1], None, self._dw(b1[0], x))
            x1, x2 = _norm_act(b1[3], b1[4], fused.conv1x1_unit(b1[2], h, act=fused.ACT_NONE)), x
        h = _norm_act(b2[1], b2[2], fused.conv1x1_unit(b2[0], x2, act=fused.ACT_NONE))
        h = _norm_act(b2[4], None, self._dw(b2[3], h))
        h = _norm_act(b2[6], b2[7], fused.conv1x1_unit(b2[5], h, act=fused.ACT_NONE))
        return fused.channel_interleave(x1, h)

    def _forward_fused(self, x):
        if self.branch1 is None:
            x1, x2 = x.chunk(2, dim=1)
            return fused.channel_interleave(x1, self._run(self.branch2, x2))
        return fused.channel_interleave(self._run(self.branch1, x), self._run(self.branch2, x))

    def forward(self, x):
        if self.fused and x.is_cuda:
            if self._unit_route_supported(x):       # ONE decision per unit (float32: its output pixels and its last convolution)
                last = self.branch2[5]
                return fused.pick_unit(x, fused.out_pixels(x, self.branch2[3].stride[0]), last.in_channels, last.out_channels, True,
                                       lambda: self._forward_unit(x), lambda: self._forward_fused(x))
            if self._gn_route_supported(x):
                return self._forward_gn(x)
            return self._forward_fused(x)
        if self.branch1 is None:
            x1, x2 = x.chunk(2, dim=1)
            out = torch.cat((x1, self.branch2(x2)), dim=1)
        else:
            out = torch.cat((self.branch1(x), self.branch2(x)), dim=1)
        return _channel_shuffle(out, 2)


class ShuffleNetV2K(BaseNetwork):
    """ShuffleNetV2 with 5x5 depthwise kernels, stride 16 (reference ``basenetworks.py:271-355``), with the reference's options
    (``network/basenetworks.py:245-400``); each keyword defaults to the class attribute of its name, which ``configure`` sets from
    the command line.  The reference's quirks are kept:

    * ``input_conv2_stride`` != 0: ``input_block.3 = Sequential(Conv2d(c0, out, 3, 2, 1), BatchNorm2d, non-linearity)`` with
      ``out = input_conv2_outchannels or c0``; the convolution's stride is 2 WHATEVER the option's value, and the overall stride
      doubles.
    * ``stage4_dilation`` d > 1: the first unit of stage 4 has stride 1 and every depthwise convolution of the stage dilation d;
      the overall stride is halved.
    * ``kernel_width`` k (odd): the depthwise kernel of every unit, padding ``(k - 1) // 2 * dilation``.
    * ``conv5_as_stage``: ``conv5`` is two units with dilation ``stage4_dilation``, the first a first-in-stage unit if and only if
      the widths differ.
    * ``leaky_relu``: ``nn.LeakyReLU(inplace=True)`` wherever the network has a ReLU.
    * ``layer_norm`` 'instance' / 'group' (the reference's ``--shufflenetv2k-instance-norm`` / ``--shufflenetv2k-group-norm``): in
      place of every ``BatchNorm2d`` -- stem, second input convolution, units, ``conv5`` -- ``InstanceNorm2d(c, affine=True,
      track_running_stats=True)`` or ``GroupNorm((32 if c % 32 == 0 else 29) if c > 100 else 4, c)`` at the same positions under the
      same state-dict keys (a group norm has ``weight`` and ``bias`` alone).  A width the group rule does not divide raises torch's
      ``ValueError`` as in the reference (shufflenetv2kx5's 42-channel stem).  In ``eval()`` the instance norm computes with its
      running statistics -- the batch-norm formula -- and ``fuse_conv_bn_`` folds it like one: the optimized network is a folded
      batch-norm network's and takes every route of one.  A group norm's statistics belong to the image: it folds into nothing, the
      modules stay, and an optimized network runs them through ``csrc/groupnorm.hip`` behind ``fused.GN`` (``_norm_act``), through
      torch without."""
    CONFIGS = {
        'shufflenetv2k16': ([4, 8, 4], [24, 348, 696, 1392, 1392]),
        'shufflenetv2k20': ([5, 10, 5], [32, 512, 1024, 2048, 2048]),
        'shufflenetv2k30': ([8, 16, 6], [32, 512, 1024, 2048, 2048]),
        'shufflenetv2k44': ([12, 24, 8], [32, 512, 1024, 2048, 2048]),
        'shufflenetv2kx5': ([6, 13, 6], [42, 640, 1280, 2560, 2560]),
    }
    input_conv2_stride = 0
    input_conv2_outchannels = None
    stage4_dilation = 1
    kernel_width = 5
    conv5_as_stage = False
    leaky_relu = False
    layer_norm = None
    OPTIONS = ('input_conv2_stride', 'input_conv2_outchannels', 'stage4_dilation', 'kernel_width', 'conv5_as_stage', 'leaky_relu',
               'layer_norm')

    def __init__(self, name='shufflenetv2k16', *, input_conv2_stride=None, input_conv2_outchannels=None, stage4_dilation=None,
                 kernel_width=None, conv5_as_stage=None, leaky_relu=None, layer_norm=None, config=None):
        given = dict(zip(self.OPTIONS, (input_conv2_stride, input_conv2_outchannels, stage4_dilation, kernel_width, conv5_as_stage,
                                        leaky_relu, layer_norm)))
        input_conv2_stride, input_conv2_outchannels, stage4_dilation, kernel_width, conv5_as_stage, leaky_relu, layer_norm = (
            getattr(type(self), k) if v is None else v for k, v in given.items())
        assert kernel_width % 2 == 1 and stage4_dilation >= 1
        repeats, ch = config or self.CONFIGS[name]          # (``config``: (stage repeats, five channel counts) of a network of one's own)
        stride = 16
        if input_conv2_stride:
            stride *= 2
        if stage4_dilation != 1:
            stride //= 2
        super().__init__(name, stride=stride, out_features=ch[-1])
        for option in self.OPTIONS:
            setattr(self, option, locals()[option])
        act = nn.LeakyReLU if leaky_relu else nn.ReLU
        norm = _layer_norm_of(layer_norm)
        unit = dict(kernel_size=kernel_width, leaky_relu=leaky_relu, layer_norm=layer_norm)
        input_modules = [nn.Conv2d(3, ch[0], 3, 2, 1, bias=False), norm(ch[0]), act(inplace=True)]
        inp = ch[0]
        if input_conv2_stride:
            out = input_conv2_outchannels or inp
            input_modules.append(nn.Sequential(nn.Conv2d(inp, out, 3, 2, 1, bias=False), norm(out), act(inplace=True)))
            inp = out
        self.input_block = nn.Sequential(*input_modules)
        stages = []
        for rep, oup, dilation in zip(repeats, ch[1:4], (1, 1, stage4_dilation)):
            # the first stage keeps resolution (the reference drops the max-pool and uses stride 16)
            seq = [_InvertedResidualK(inp, oup, True, stride=2 if dilation == 1 else 1, dilation=dilation, **unit)]
            seq += [_InvertedResidualK(oup, oup, False, dilation=dilation, **unit) for _ in range(rep - 1)]
            stages.append(nn.Sequential(*seq))
            inp = oup
        self.stage2, self.stage3, self.stage4 = stages
        if conv5_as_stage:
            self.conv5 = nn.Sequential(_InvertedResidualK(inp, ch[-1], inp != ch[-1], dilation=stage4_dilation, **unit),
                                       _InvertedResidualK(ch[-1], ch[-1], False, dilation=stage4_dilation, **unit))
        else:
            self.conv5 = nn.Sequential(
                nn.Conv2d(inp, ch[-1], 1, bias=False), norm(ch[-1]), act(inplace=True))

    @classmethod
    def cli(cls, parser):
        """The reference's flags (``network/basenetworks.py:357-384``).  ``--shufflenetv2k-instance-norm`` and
        ``--shufflenetv2k-group-norm`` exclude each other and share ONE destination, ``shufflenetv2k_layer_norm`` ('instance' /
        'group'; None without either), so that ``configure`` reads them like every other option."""
        group = parser.add_argument_group('shufflenetv2k')
        group.add_argument('--shufflenetv2k-input-conv2-stride', default=cls.input_conv2_stride, type=int,
                           help='stride of the optional 2nd input convolution')
        group.add_argument('--shufflenetv2k-input-conv2-outchannels', default=cls.input_conv2_outchannels, type=int,
                           help='out channels of the optional 2nd input convolution')
        group.add_argument('--shufflenetv2k-stage4-dilation', default=cls.stage4_dilation, type=int,
                           help='dilation factor of stage 4')
        group.add_argument('--shufflenetv2k-kernel', default=cls.kernel_width, type=int, help='kernel width')
        group.add_argument('--shufflenetv2k-conv5-as-stage', default=False, action='store_true')
        group.add_argument('--shufflenetv2k-leaky-relu', default=False, action='store_true')
        layer_norm = group.add_mutually_exclusive_group()
        layer_norm.add_argument('--shufflenetv2k-instance-norm', dest='shufflenetv2k_layer_norm', default=cls.layer_norm,
                                action='store_const', const='instance')
        layer_norm.add_argument('--shufflenetv2k-group-norm', dest='shufflenetv2k_layer_norm', default=cls.layer_norm,
                                action='store_const', const='group')

    @classmethod
    def configure(cls, args):
        for option in cls.OPTIONS:             # (a namespace from a parser without these flags leaves the attributes as they are)
            flag = 'shufflenetv2k_' + ('kernel' if option == 'kernel_width' else option)
            setattr(cls, option, getattr(args, flag, getattr(cls, option)))

    def _input_block_forward(self, x):
        """``input_block(x)``, the stem through ``_stem_route`` where that takes it (the second input convolution stays with torch).
        In an optimized group-norm network with ``fused.GN`` on, the norms of both convolutions go through ``_norm_act``, whoever
        computed the convolution."""
        modules = list(self.input_block)
        y = _stem_route(self, modules[0], modules[2], x, norm=modules[1])
        gn = self.fused and fused.GN and x.is_cuda and isinstance(modules[1], nn.GroupNorm)
        if y is None:
            if not gn:
                return self.input_block(x)
            y = _norm_act(modules[1], modules[2], modules[0](x))
        for m in modules[3:]:
            y = _norm_act(m[1], m[2], m[0](y)) if gn and isinstance(m, nn.Sequential) else m(y)
        return y

    def forward(self, x):
        return _conv5_forward(self, self.stage4(self.stage3(self.stage2(self._input_block_forward(x)))))


def _conv5_forward(net, x):
    """``net.conv5(x)`` of a ShuffleNetV2K or a ShuffleNetV2: ``Sequential(Conv2d 1x1, BatchNorm2d, non-linearity)`` through the
    split-operand GEMM's unit mode where that takes it, decided like the units (the table, else by size, never timed).  A stage
    ``conv5`` routes itself, unit by unit.  The GEMM's epilogue applies a ReLU, or a LeakyReLU where ``fused.UNIT_LEAKY`` is on (outside
    autocast); with the switch off a LeakyReLU ``conv5`` stays with torch.  The module between the two must be the ``Identity`` that
    folding leaves: a ``GroupNorm`` there runs -- with ``fused.GN`` on behind the GEMM without an activation (``_norm_act``), else
    with torch's ``conv5``.  A bfloat16 ``conv5`` (ReLU or, with ``fused.UNIT_LEAKY``, LeakyReLU behind an ``Identity``) takes the same
    branch where ``fused.UNIT_BF16`` is on -- ``fused.unit_conv_supported`` goes by ``x``'s dtype -- and runs: no table entry, no timing
    (``fused.pick_unit``), and so does a float16 one where ``fused.UNIT_F16`` is on; a group norm is float32's alone."""
    conv = net.conv5[0]
    if net.fused and x.is_cuda and isinstance(conv, nn.Conv2d) and fused.unit_conv_supported(conv, x):
        norm, nonlin, act = net.conv5[1], net.conv5[2], None
        if not isinstance(norm, nn.Identity):
            if fused.GN and isinstance(norm, nn.GroupNorm) and x.dtype == torch.float32 and not torch.is_autocast_enabled():
                return _norm_act(norm, nonlin, fused.conv1x1_unit(conv, x, act=fused.ACT_NONE))
            return net.conv5(x)
        if isinstance(nonlin, nn.ReLU):
            act = {}
        elif isinstance(nonlin, nn.LeakyReLU) and fused.UNIT_LEAKY and not torch.is_autocast_enabled():
            act = dict(act=fused.ACT_LEAKY_RELU, act_param=nonlin.negative_slope)
        if act is not None:
            return fused.pick_unit(x, fused.out_pixels(x), conv.in_channels, conv.out_channels, False,
                                   lambda: fused.conv1x1_unit(conv, x, **act), lambda: net.conv5(x))
    return net.conv5(x)


class ShuffleNetV2(BaseNetwork):
    """ShuffleNetV2 x1.0 / x2.0 as the reference uses them: torchvision's ``shufflenet_v2_x1_0`` / ``shufflenet_v2_x2_0`` without the
    max-pool behind ``conv1`` and without the classifier, stride 16 (reference ``network/basenetworks.py:36-69``,
    ``network/factory.py:63-67``), restated with torchvision's module tree (``conv1``, ``stage2..4.<i>.branch1|branch2.<j>``, ``conv5``),
    so that the ``base_net.*`` keys of a reference checkpoint fit.  The unit is ``_InvertedResidualK`` with a 3x3 window -- the
    same indices inside ``branch1`` / ``branch2`` as torchvision's ``InvertedResidual`` -- so the units and ``conv5`` take the routes
    ShuffleNetV2K's take.  No checkpoint can be loaded offline: the fit is checked by key names and shapes only
    (``tests/test_mobilenetv2_host.py``), never against real weights."""
    # stage repeats, [conv1, stage2, stage3, stage4, conv5] channels
    CONFIGS = {
        'shufflenetv2x1': ([4, 8, 4], [24, 116, 232, 464, 1024]),
        'shufflenetv2x2': ([4, 8, 4], [24, 244, 488, 976, 2048]),
    }

    def __init__(self, name='shufflenetv2x2'):
        repeats, ch = self.CONFIGS[name]
        super().__init__(name, stride=16, out_features=ch[-1])
        self.conv1 = nn.Sequential(nn.Conv2d(3, ch[0], 3, 2, 1, bias=False), nn.BatchNorm2d(ch[0]), nn.ReLU(inplace=True))
        inp, stages = ch[0], []
        for rep, oup in zip(repeats, ch[1:4]):
            seq = [_InvertedResidualK(inp, oup, True, stride=2, kernel_size=3)]
            seq += [_InvertedResidualK(oup, oup, False, kernel_size=3) for _ in range(rep - 1)]
            stages.append(nn.Sequential(*seq))
            inp = oup
        self.stage2, self.stage3, self.stage4 = stages
        self.conv5 = nn.Sequential(nn.Conv2d(inp, ch[-1], 1, bias=False), nn.BatchNorm2d(ch[-1]), nn.ReLU(inplace=True))

    def forward(self, x):
        y = _stem_route(self, self.conv1[0], self.conv1[2], x)
        return _conv5_forward(self, self.stage4(self.stage3(self.stage2(self.conv1(x) if y is None else y))))


def _make_divisible(v, divisor=8):
    new_v = max(divisor, int(v + divisor / 2) // divisor * divisor)
    if new_v < 0.9 * v:
        new_v += divisor
    return new_v


def _conv_bn_act(inp, oup, kernel_size, stride, groups, act):
    layers = [nn.Conv2d(inp, oup, kernel_size, stride, kernel_size // 2, groups=groups, bias=False),
              nn.BatchNorm2d(oup, eps=1e-3, momentum=0.01)]       # (the reference forces eps >= 1e-3, ``network/nets.py:78``)
    if act is not None:
        layers.append(act(inplace=True))
    return nn.Sequential(*layers)


class _SqueezeExcitation(nn.Module):
    """``x * hardsigmoid(fc2(relu(fc1(mean(x)))))`` (torchvision's ``SqueezeExcitation``: the same attribute names)."""

    def __init__(self, channels, squeeze):
        super().__init__()
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc1 = nn.Conv2d(channels, squeeze, 1)
        self.fc2 = nn.Conv2d(squeeze, channels, 1)
        self.activation = nn.ReLU()
        self.scale_activation = nn.Hardsigmoid()

    def forward(self, x):
        return x * self.scale_activation(self.fc2(self.activation(self.fc1(self.avgpool(x)))))


def _assert_folded(module):
    assert not any(isinstance(m, nn.BatchNorm2d) for m in module.modules()), 'fold the batch norms first (fuse_conv_bn_)'


class _InvertedResidual(nn.Module):
    """What the inverted residuals of MobileNetV3 and MobileNetV2 share: [expand,] depthwise, [se,] project, the block's input added
    under ``use_res_connect``, and the route that runs all of it on the project's kernels.  A subclass builds its layers and states
    ``_body`` (the attribute that holds them), ``_switch`` (the name of its switch in ``fused``), ``_act`` (code and parameter of its
    activation) and, as properties, where ``expand``, ``depthwise``, ``se`` and ``project`` sit in the body."""
    fused = False

    def enable_fused_(self):
        """After conv+BN folding: the block may run on the project's kernels alone (``_forward_unit``); no parameter or buffer changes."""
        _assert_folded(self)
        self.fused = True

    @staticmethod
    def taps_of(conv):
        """The CURRENT depthwise weight tap-major, ``[k * k, C]`` (derived and cached, no part of a checkpoint)."""
        return fused.derived(conv, '_opa_taps', (conv.weight,), lambda: fused.depthwise_taps(conv.weight))

    def _route_supported(self, x):
        """Can the WHOLE block run on the project's kernels (``_forward_unit``)?  float32 outside autocast, nothing that autograd
        follows; every intermediate tensor is a dense channels-last one this module allocates, so its layout is known and its sizes
        follow from ``x``'s."""
        if not (getattr(fused, self._switch) and x.is_cuda and x.dim() == 4 and x.dtype == torch.float32
                and not torch.is_autocast_enabled() and not x.requires_grad):
            return False
        expand, dw, se, project = self.expand, self.depthwise, self.se, self.project
        k, s = dw.kernel_size[0], dw.stride[0]
        if expand is not None and not (expand.bias is not None and fused.unit_conv_x3_supported(expand, x)):
            return False
        # (the stencil's limits are on the batch and the rows, which the expanding convolution keeps; without one the stencil reads
        #  ``x`` itself, whose layout ``dwconv_supported`` tests)
        if not (dw.weight.dtype == torch.float32 and dw.bias is not None and dw.bias.dtype == torch.float32
                and dw.weight.device == x.device and dw.padding == (k // 2, k // 2) and dw.dilation == (1, 1)
                and fused.dwconv_supported(x, k, s)):
            return False
        pixels = ((x.shape[2] - 1) // s + 1) * ((x.shape[3] - 1) // s + 1)          # of the depthwise output, which the SE kernels read
        if se is not None and not (fused._se_convs_ok(se.fc1, se.fc2) and se.fc1.weight.device == x.device
                                   and x.shape[0] <= 65535 and pixels <= fused.SE_MAX_PIXELS and fused._lib.available()):
            return False
        if not (project.bias is not None and fused._unit_conv_ok(fused.UNIT_MODE_X3, project) and project.weight.device == x.device):
            return False
        return not self.use_res_connect or fused._unit_operand_ok(fused.UNIT_MODE_X3, x, project.out_channels)

    def _forward_unit(self, x):
        """Two to six launches: [GEMM + bias + activation,] the depthwise stencil + bias + activation, [the SE pool, its gate, the
        scale in place,] GEMM + bias (+ the block's input as the residual: the projecting convolution is linear)."""
        act = dict(act=self._act[0], act_param=self._act[1])
        expand, dw, se = self.expand, self.depthwise, self.se
        h = x if expand is None else fused.conv1x1_unit_x3(expand, x, **act)
        h = fused.dwconv_bias_act(h, self.taps_of(dw), dw.bias, dw.kernel_size[0], dw.stride[0], **act)
        if se is not None:
            fused.scale_channels_(h, fused.se_gate(h, se.fc1, se.fc2))
        return fused.conv1x1_unit_x3(self.project, h, residual=x if self.use_res_connect else None, act=fused.ACT_NONE)

    def forward(self, x):
        if self.fused and self._route_supported(x):
            return self._forward_unit(x)
        out = getattr(self, self._body)(x)
        return out + x if self.use_res_connect else out


class _MBV3Block(_InvertedResidual):
    """MobileNetV3's inverted residual (torchvision's ``InvertedResidual``: ``.block`` = [expand,] depthwise, [se,] project)."""
    _body, _switch = 'block', 'MBV3'

    def __init__(self, inp, kernel_size, exp, oup, use_se, use_hs, stride):
        super().__init__()
        act = nn.Hardswish if use_hs else nn.ReLU
        layers = []
        if exp != inp:
            layers.append(_conv_bn_act(inp, exp, 1, 1, 1, act))
        layers.append(_conv_bn_act(exp, exp, kernel_size, stride, exp, act))
        if use_se:
            layers.append(_SqueezeExcitation(exp, _make_divisible(exp // 4, 8)))
        layers.append(_conv_bn_act(exp, oup, 1, 1, 1, None))
        self.block = nn.Sequential(*layers)
        self.use_res_connect = stride == 1 and inp == oup
        self._has_expand, self._has_se = exp != inp, use_se
        self._act = (fused.ACT_HARDSWISH if use_hs else fused.ACT_RELU, 0.0)

    expand = property(lambda self: self.block[0][0] if self._has_expand else None, doc='the expanding 1x1 convolution, or None')
    depthwise = property(lambda self: self.block[1 if self._has_expand else 0][0], doc='the depthwise convolution')
    se = property(lambda self: self.block[-2] if self._has_se else None, doc='the squeeze-and-excitation module, or None')
    project = property(lambda self: self.block[-1][0], doc='the projecting 1x1 convolution')


class _MobileNet(BaseNetwork):
    """What MobileNetV3 and MobileNetV2 share: ``backbone``, whose last module is a 1x1 convolution with the network's activation.  A
    subclass states ``_switch`` and ``_act`` as its blocks do."""

    def enable_fused_(self):
        """The last 1x1 convolution may run through the split-operand GEMM's unit mode (bias + activation inside); the stem stays
        with ``torch.nn.Conv2d`` like every non-ResNet stem unless ``fused.STEM`` is on (``_stem_route``).  No parameter or buffer
        changes."""
        _assert_folded(self)
        super().enable_fused_()

    def forward(self, x):
        stem, *blocks, last = self.backbone
        y = _stem_route(self, stem[0], stem[2], x)
        x = stem(x) if y is None else y
        for m in blocks:
            x = m(x)
        conv = last[0]
        if (self.fused and getattr(fused, self._switch) and x.is_cuda and not torch.is_autocast_enabled() and conv.bias is not None
                and fused.unit_conv_x3_supported(conv, x)):
            return fused.conv1x1_unit_x3(conv, x, act=self._act[0], act_param=self._act[1])
        return last(x)


class MobileNetV3(_MobileNet):
    """MobileNetV3 large / small as the reference uses them: torchvision's ``features`` with the stride of the first convolution set
    to 1, so the overall stride is 16 (reference ``network/basenetworks.py:432-446``, ``network/factory.py:53-56``), restated from the
    paper's tables with torchvision's module tree (``backbone.<i>.block.<j>...``), so that the ``base_net.backbone.*`` keys of a
    reference checkpoint fit.  No checkpoint can be loaded offline: the fit is checked by key names and shapes only
    (``tests/test_mobilenetv3_host.py``), never against real weights."""
    _switch, _act = 'MBV3', (fused.ACT_HARDSWISH, 0.0)
    # in, kernel, expanded, out, SE, hardswish, stride
    CONFIGS = {
        'mobilenetv3large': ([
            (16, 3, 16, 16, False, False, 1), (16, 3, 64, 24, False, False, 2), (24, 3, 72, 24, False, False, 1),
            (24, 5, 72, 40, True, False, 2), (40, 5, 120, 40, True, False, 1), (40, 5, 120, 40, True, False, 1),
            (40, 3, 240, 80, False, True, 2), (80, 3, 200, 80, False, True, 1), (80, 3, 184, 80, False, True, 1),
            (80, 3, 184, 80, False, True, 1), (80, 3, 480, 112, True, True, 1), (112, 3, 672, 112, True, True, 1),
            (112, 5, 672, 160, True, True, 2), (160, 5, 960, 160, True, True, 1), (160, 5, 960, 160, True, True, 1)], 960),
        'mobilenetv3small': ([
            (16, 3, 16, 16, True, False, 2), (16, 3, 72, 24, False, False, 2), (24, 3, 88, 24, False, False, 1),
            (24, 5, 96, 40, True, True, 2), (40, 5, 240, 40, True, True, 1), (40, 5, 240, 40, True, True, 1),
            (40, 5, 120, 48, True, True, 1), (48, 5, 144, 48, True, True, 1), (48, 5, 288, 96, True, True, 2),
            (96, 5, 576, 96, True, True, 1), (96, 5, 576, 96, True, True, 1)], 576),
    }

    def __init__(self, name='mobilenetv3large'):
        blocks, out_features = self.CONFIGS[name]
        super().__init__(name, stride=16, out_features=out_features)
        layers = [_conv_bn_act(3, 16, 3, 1, 1, nn.Hardswish)]              # (torchvision: stride 2; the reference sets it to 1)
        layers += [_MBV3Block(*cfg) for cfg in blocks]
        layers.append(_conv_bn_act(blocks[-1][3], out_features, 1, 1, 1, nn.Hardswish))
        self.backbone = nn.Sequential(*layers)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out')
                if m.bias is not None:
                    nn.init.zeros_(m.bias)


class _MBV2Block(_InvertedResidual):
    """MobileNetV2's inverted residual (torchvision's ``InvertedResidual``: ``.conv`` = [expand + BN + ReLU6,] depthwise + BN + ReLU6,
    the projecting ``Conv2d``, its ``BatchNorm2d``; no expanding convolution where the expansion ratio is 1)."""
    _body, _switch, _act = 'conv', 'MBV2', (fused.ACT_RELU6, 6.0)

    def __init__(self, inp, oup, stride, expand_ratio):
        super().__init__()
        hidden = inp * expand_ratio
        layers = []
        if expand_ratio != 1:
            layers.append(_conv_bn_act(inp, hidden, 1, 1, 1, nn.ReLU6))
        layers += [_conv_bn_act(hidden, hidden, 3, stride, hidden, nn.ReLU6),
                   nn.Conv2d(hidden, oup, 1, bias=False), nn.BatchNorm2d(oup, eps=1e-3, momentum=0.01)]
        self.conv = nn.Sequential(*layers)
        self.use_res_connect = stride == 1 and inp == oup
        self._has_expand = expand_ratio != 1

    expand = property(lambda self: self.conv[0][0] if self._has_expand else None, doc='the expanding 1x1 convolution, or None')
    depthwise = property(lambda self: self.conv[1 if self._has_expand else 0][0], doc='the depthwise convolution')
    se = None
    project = property(lambda self: self.conv[-2], doc='the projecting 1x1 convolution')


class MobileNetV2(_MobileNet):
    """MobileNetV2 as the reference uses it: torchvision's ``mobilenet_v2().features``, stride 32, 1280 features (reference
    ``network/basenetworks.py:407-430``, ``network/factory.py:52``), restated from the paper's table with torchvision's module tree
    (``backbone.0`` the stem, ``backbone.<i>.conv.<j>...`` the inverted residuals, ``backbone.18`` the last convolution), so that the
    ``base_net.backbone.*`` keys of a reference checkpoint fit.  No checkpoint can be loaded offline: the fit is checked by key
    names and shapes only (``tests/test_mobilenetv2_host.py``), never against real weights."""
    _switch, _act = _MBV2Block._switch, _MBV2Block._act
    # expansion ratio t, output channels c, repeats n, stride of the first repeat s
    CONFIGS = {'mobilenetv2': ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1))}

    def __init__(self, name='mobilenetv2'):
        super().__init__(name, stride=32, out_features=1280)
        layers = [_conv_bn_act(3, 32, 3, 2, 1, nn.ReLU6)]
        inp = 32
        for t, c, n, s in self.CONFIGS[name]:
            for i in range(n):
                layers.append(_MBV2Block(inp, c, s if i == 0 else 1, t))
                inp = c
        layers.append(_conv_bn_act(inp, self.out_features, 1, 1, 1, nn.ReLU6))
        self.backbone = nn.Sequential(*layers)
        for m in self.modules():               # torchvision's initialisation
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out')


class _Fire(nn.Module):
    """SqueezeNet's Fire module (torchvision's ``Fire``: the same attribute names): a 1x1 squeeze, then a 1x1 and a 3x3 expand of the
    squeezed tensor, concatenated; every convolution biased and followed by a ReLU."""

    def __init__(self, inplanes, squeeze_planes, expand1x1_planes, expand3x3_planes):
        super().__init__()
        self.squeeze = nn.Conv2d(inplanes, squeeze_planes, 1)
        self.squeeze_activation = nn.ReLU(inplace=True)
        self.expand1x1 = nn.Conv2d(squeeze_planes, expand1x1_planes, 1)
        self.expand1x1_activation = nn.ReLU(inplace=True)
        self.expand3x3 = nn.Conv2d(squeeze_planes, expand3x3_planes, 3, padding=1)
        self.expand3x3_activation = nn.ReLU(inplace=True)

    fused = False

    def enable_fused_(self):
        """The module may run on the project's kernels alone (``_forward_unit``); no parameter or buffer changes."""
        self.fused = True

    def _route_supported(self, x):
        """Can the WHOLE module run on the project's kernels (``_forward_unit``)?  A float32 channels-last tensor on the GPU, outside
        autocast, nothing that autograd follows; the squeezed tensor is a dense channels-last one this module allocates, so its
        layout is known and its size follows from ``x``'s."""
        if not (fused.FIRE and x.is_cuda and x.dim() == 4 and x.dtype == torch.float32 and not torch.is_autocast_enabled()
                and x.is_contiguous(memory_format=torch.channels_last)):
            return False
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            return False
        return (self.squeeze.bias is not None and fused.FIRE_TERMS in (6, 9) and fused.unit_conv_x3_supported(self.squeeze, x)
                and fused.fire_expand_shape_supported(self.expand1x1, self.expand3x3, x.device, x.shape[0] * x.shape[2] * x.shape[3]))

    def _forward_unit(self, x):
        """Two launches: the squeeze as GEMM + bias + ReLU (unit mode), then both expands, their biases and ReLUs and the
        concatenation (``csrc/fire.hip``); both with ``fused.FIRE_TERMS`` terms."""
        h = fused.conv1x1_unit_x3(self.squeeze, x, relu=True, terms=fused.FIRE_TERMS)
        return fused.fire_expand_bias_relu(self.expand1x1, self.expand3x3, h)

    def forward(self, x):
        if self.fused and self._route_supported(x):
            return self._forward_unit(x)
        x = self.squeeze_activation(self.squeeze(x))
        return torch.cat([self.expand1x1_activation(self.expand1x1(x)), self.expand3x3_activation(self.expand3x3(x))], 1)


class SqueezeNet(BaseNetwork):
    """SqueezeNet 1.1 as the reference uses it: torchvision's ``squeezenet1_1().features`` with the padding of the stem and of every
    max-pool set to 1 (the pools keep ``ceil_mode=True``), stride 16, 512 features (reference ``network/basenetworks.py:461-487``,
    ``network/factory.py:52-78``), restated with torchvision's module tree (``backbone.<i>.squeeze`` ...), so that the
    ``base_net.backbone.*`` keys of a reference checkpoint fit.  No checkpoint can be loaded offline: the fit is checked by key
    names and shapes only (``tests/test_squeezenet_host.py``), never against real weights."""
    # in, squeeze, expand 1x1, expand 3x3; None: a max-pool
    CONFIGS = {'squeezenet': ((64, 16, 64, 64), (128, 16, 64, 64), None, (128, 32, 128, 128), (256, 32, 128, 128), None,
                              (256, 48, 192, 192), (384, 48, 192, 192), (384, 64, 256, 256), (512, 64, 256, 256))}

    def __init__(self, name='squeezenet'):
        super().__init__(name, stride=16, out_features=512)

        def pool():
            return nn.MaxPool2d(kernel_size=3, stride=2, padding=1, ceil_mode=True)     # (torchvision: padding 0)
        layers = [nn.Conv2d(3, 64, 3, stride=2, padding=1), nn.ReLU(inplace=True), pool()]          # (torchvision: padding 0)
        layers += [pool() if cfg is None else _Fire(*cfg) for cfg in self.CONFIGS[name]]
        self.backbone = nn.Sequential(*layers)
        for m in self.modules():               # torchvision's initialisation (its last, classifying convolution aside)
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_uniform_(m.weight)
                nn.init.zeros_(m.bias)

    @staticmethod
    def _pool_route_supported(pool, x):
        return (isinstance(pool, nn.MaxPool2d) and pool.kernel_size == 3 and pool.stride == 2 and pool.padding == 1 and pool.dilation == 1
                and pool.ceil_mode and not pool.return_indices and fused.maxpool3x3_supported(x))

    def forward(self, x):
        """Fused (``fused.FIRE``): the max-pools through the ceil-mode entry point of ``csrc/pool.hip`` (the first with the stem's ReLU
        inside); the stem stays with ``torch.nn.Conv2d`` like MobileNetV3's and ShuffleNetV2K's unless ``fused.STEM`` is on -- then it
        is ``_stem_route``'s with the ReLU applied there, once, and the first max-pool runs without it."""
        modules = list(self.backbone)
        i = 0
        y = _stem_route(self, modules[0], modules[1], x)
        if y is not None:
            x, i = y, 2
        pools = self.fused and fused.FIRE and x.is_cuda and not torch.is_autocast_enabled()
        if not pools and i == 0:
            return self.backbone(x)
        while i < len(modules):
            m = modules[i]
            if pools and isinstance(m, nn.ReLU) and i + 1 < len(modules) and self._pool_route_supported(modules[i + 1], x):
                x = fused.maxpool3x3_bias_act_(x, relu=True, ceil_mode=True)        # the stem's ReLU goes into the pool (max and ReLU commute)
                i += 2
                continue
            x = fused.maxpool3x3_bias_act_(x, ceil_mode=True) if pools and self._pool_route_supported(m, x) else m(x)
            i += 1
        return x


BASE_FACTORIES = {
    **{n: (lambda n=n: Resnet(n)) for n in Resnet.CONFIGS},
    **{n: (lambda n=n: ShuffleNetV2K(n)) for n in ShuffleNetV2K.CONFIGS},
    **{n: (lambda n=n: ShuffleNetV2(n)) for n in ShuffleNetV2.CONFIGS},
    **{n: (lambda n=n: MobileNetV2(n)) for n in MobileNetV2.CONFIGS},
    **{n: (lambda n=n: MobileNetV3(n)) for n in MobileNetV3.CONFIGS},
    **{n: (lambda n=n: SqueezeNet(n)) for n in SqueezeNet.CONFIGS},
}


class CompositeField4(nn.Module):
    """Head: features -> ``[B, n_fields, n_components, H, W]`` in the layout the decoder reads."""

    def __init__(self, meta: headmeta.Base, in_features):
        super().__init__()
        self.meta = meta
        self.n_components = 1 + meta.n_confidences + meta.n_vectors * 2 + meta.n_scales
        self.conv = nn.Conv2d(in_features, meta.n_fields * self.n_components * (meta.upsample_stride ** 2), 1)
        self.upsample_op = nn.PixelShuffle(meta.upsample_stride) if meta.upsample_stride > 1 else None

    fused_epilogue = True      # one HIP kernel for everything behind the convolution (inference, channels_last)

    def forward(self, x):
        if not self.training and self.fused_epilogue and fused.head_conv_fields16_supported(self.conv, x, self.meta, self.training):
            # 16-bit inference behind fused.HEAD16: the convolution on the 16-bit MFMA and the epilogue on its float32 sums, one kernel
            return fused.head_conv_fields16(self.conv, x, self.meta)
        if not self.training and fused.head_conv_x3_supported(self.conv, x):     # float32 inference: the head's 1x1 convolution through
            conv, x0 = self.conv, x                                                # the split-operand GEMM where that is faster
            x = fused.pick('head', fused.out_pixels(x0), conv.in_channels, conv.out_channels, False, False,
                           lambda: fused.head_conv_x3(conv, x0), lambda: conv(x0))
        elif not self.training and self.conv.in_channels % 64 != 0 and fused.unit_conv_supported(self.conv, x, head=True):
            # input channels that are no multiple of 64 (k16: 1392): the unit mode of x's dtype.  float32: the same kernel, N tail native
            # (no padded pitch, no copy-out), decided like the units -- the table, else by size, never timed; bfloat16 (behind
            # fused.UNIT_BF16) and float16 (behind fused.UNIT_F16): where it is supported it runs
            conv, x0 = self.conv, x
            x = fused.pick_unit(x0, fused.out_pixels(x0), conv.in_channels, conv.out_channels, False,
                                lambda: fused.conv1x1_unit(conv, x0, relu=False), lambda: conv(x0))
        else:
            x = self.conv(x)
        if self.fused_epilogue and fused.head_epilogue_supported(x, self.meta, self.training):
            return fused.head_epilogue(x, self.meta)
        if self.upsample_op is not None:
            x = self.upsample_op(x)
            us = self.meta.upsample_stride
            low_cut = (us - 1) // 2
            high_cut = math.ceil((us - 1) / 2.0)
            x = x[:, :, low_cut:x.shape[2] - high_cut, low_cut:x.shape[3] - high_cut]
        B, _, H, W = x.shape
        m = self.meta
        x = x.float().reshape(B, m.n_fields, self.n_components, H, W).contiguous()
        if not self.training:
            nc = m.n_confidences
            x[:, :, 1:1 + nc].sigmoid_()
            ii = torch.arange(W, device=x.device, dtype=x.dtype)
            jj = torch.arange(H, device=x.device, dtype=x.dtype).unsqueeze(1)
            for i, do_offset in enumerate(m.vector_offsets):
                if do_offset:
                    x[:, :, 1 + nc + 2 * i] += ii
                    x[:, :, 1 + nc + 2 * i + 1] += jj
            first_scale = 1 + nc + m.n_vectors * 2
            x[:, :, first_scale:first_scale + m.n_scales] = nn.functional.softplus(
                x[:, :, first_scale:first_scale + m.n_scales])
        return x


class Shell(nn.Module):
    """base_net + head_nets (reference ``network/nets.py:11-48``)."""

    def __init__(self, base_net, head_nets):
        super().__init__()
        self.base_net = base_net
        self.head_nets = None
        self.set_head_nets(head_nets)

    @property
    def head_metas(self):
        return [hn.meta for hn in self.head_nets] if self.head_nets is not None else None

    def set_head_nets(self, head_nets):
        if not isinstance(head_nets, nn.ModuleList):
            head_nets = nn.ModuleList(head_nets)
        for i, hn in enumerate(head_nets):
            hn.meta.head_index = i
            hn.meta.base_stride = self.base_net.stride
        self.head_nets = head_nets

    def forward(self, image_batch):
        x = self.base_net(image_batch)
        return tuple(hn(x) for hn in self.head_nets)


def factory(base_name='resnet50', head_metas=None, *, seed=0):
    """Randomly initialised ``Shell`` for ``head_metas`` (default: cocokp CIF+CAF, upsample 2)."""
    if head_metas is None:
        head_metas = headmeta.cocokp_metas()
    gen_state = torch.random.get_rng_state()
    torch.manual_seed(seed)
    try:
        base = BASE_FACTORIES[base_name]()
        heads = [CompositeField4(m, base.out_features) for m in head_metas]
        net = Shell(base, heads)
    finally:
        torch.random.set_rng_state(gen_state)
    return net.eval()


def _folds(norm):
    """Is ``norm`` a per-channel affine map in ``eval()`` -- a ``BatchNorm2d``, or an ``InstanceNorm2d`` that has affine terms and
    running statistics (which it then uses in place of the image's: the batch-norm formula, reference ``network/basenetworks.py:395-397``)?
    Every other instance norm, and a group norm, depend on the image."""
    return isinstance(norm, nn.BatchNorm2d) or (isinstance(norm, nn.InstanceNorm2d) and norm.affine and norm.track_running_stats
                                                and not norm.training)


def _fold(conv, bn):
    """conv <- conv followed by eval-mode batch norm (or an instance norm that ``_folds``)."""
    with torch.no_grad():
        scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
        conv.weight.mul_(scale.reshape(-1, 1, 1, 1))
        bias = bn.bias - bn.running_mean * scale
        if conv.bias is not None:
            bias = bias + conv.bias * scale
        conv.bias = nn.Parameter(bias)


def fuse_conv_bn_(model):
    """Inference-time folding of every (Conv2d, BatchNorm2d) pair into the convolution
    (removes one full activation read+write per layer, the dominant non-GEMM cost at 641 px)."""
    assert not model.training
    for module in model.modules():
        if isinstance(module, nn.Sequential):
            prev_name, prev = None, None
            for name, child in list(module.named_children()):
                if _folds(child) and isinstance(prev, nn.Conv2d):
                    _fold(prev, child)
                    setattr(module, name, nn.Identity())
                prev_name, prev = name, child
        for i in (1, 2, 3):
            conv, bn = getattr(module, 'conv%d' % i, None), getattr(module, 'bn%d' % i, None)
            if isinstance(conv, nn.Conv2d) and isinstance(bn, nn.BatchNorm2d):
                _fold(conv, bn)
                setattr(module, 'bn%d' % i, nn.Identity())
    return model


def optimize_for_inference_(model):
    """Fold every conv+BN pair, then switch each family to its kernels:

    * the ResNet and ResNeXt blocks to the fused-epilogue forward (conv without bias followed by ONE ``fused.bias_act_`` pass);
    * the ShuffleNetV2K and ShuffleNetV2 units and ``conv5`` to the HIP depthwise / interleave kernels and the split-operand GEMM's
      unit mode (a LeakyReLU unit's 1x1 convolutions behind ``fused.UNIT_LEAKY``);
    * the MobileNetV3 blocks and last convolution to the same GEMM, the depthwise stencil and the squeeze-and-excitation kernels
      (behind ``fused.MBV3``);
    * the MobileNetV2 blocks and last convolution to that GEMM and that stencil with ReLU6 (behind ``fused.MBV2``);
    * the SqueezeNet Fire modules and max-pools to that GEMM, the Fire expand kernel and the ceil-mode pool (behind ``fused.FIRE``);
    * the 3x3 RGB stem of these five families to the stem kernel with the bias and the activation inside (behind ``fused.STEM``);
    * a ShuffleNetV2K's instance norms fold like batch norms; its group norms stay and run through the group-norm kernels, each with
      the activation behind it (behind ``fused.GN``)."""
    fuse_conv_bn_(model)
    for m in model.modules():
        if isinstance(m, (_Bottleneck, _BasicBlock, _InvertedResidualK, _InvertedResidual, _Fire, BaseNetwork)):
            m.enable_fused_()
    return model
