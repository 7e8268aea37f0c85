"""The route layer of the trunk: everything between the ``torch.nn`` modules of ``network.py`` and the HIP kernels under ``csrc/``.

For every kernel family it holds the predicate that says whether the kernel can run for given operands (``*_supported``: the
kernel's contract), the operands derived from the module's parameters (split, padded, transposed copies, cached on the module:
``derived``) and the launcher that hands them to the C ABI.  Where a kernel competes with another way to compute the same tensor,
the choice is made once per shape and remembered in one table (``_CHOICE``, shipped as ``conv1x1_pinned.json``): ``conv_bias_act``
and ``pick`` say what the candidates are, ``_decide`` makes the choice.  In this order: the launcher, the switches (with one ``Route16``
record per route on the 16-bit MFMA), the choice table and the decision, layouts, sizes and what else the predicates share, the
derived operands, then the routes by kernel family -- the epilogue passes, the 1x1 GEMMs, the split-operand convolutions (pair, 3x3
and dilated 3x3, stem, heads), the unit mode (ONE route with a ``UnitMode`` record per element type -- float32 on the split-operand
GEMM, bfloat16 on the bf16 MFMA -- whose callers pass tensors and name no dtype), the Fire expand, the max-pools, the grouped and the
depthwise stencils, the RGB stem, group norm, squeeze-and-excitation."""
import functools
import os
import typing

import torch

from . import _lib
from .native import _ptr, _stream

_DTYPES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
ACT_NONE, ACT_RELU, ACT_HARDSWISH = 0, 1, 2      # the activation codes of opa_dwconv_act and opa_gemm_unit_act_f32x3
# ... and the two with a parameter (``act_param``), which the opa_*_actp entry points take: LeakyReLU(slope) -- not the stencil -- and
# the ReLU clipped at a cap (ReLU6: 6)
ACT_LEAKY_RELU, ACT_RELU6 = 3, 4


# ---- the launcher ---------------------------------------------------------------------------------------------------------------

def _launch(symbol, *args):
    """Calls ``symbol`` of the library with ``args`` followed by the current stream; any status but OK raises under that name.
    ``_lib.SYMBOLS`` declares every argument's type: an address goes in as a plain integer or None (``_ptr``)."""
    _lib.check(getattr(_lib.lib(), symbol)(*args, _stream()), symbol)


def _act_code(relu, act):
    """The activation code of a launcher that takes ``relu=`` and ``act=``: ``act`` where it is given."""
    return int(bool(relu)) if act is None else int(act)


# ---- the switches (read ONCE, at import; the attributes can be set afterwards) ---------------------------------------------------

def _switch(name, default):
    return os.environ.get(name, default) != '0'


# float32 1x1 convolutions may take the split-operand kernel (choice 'gemm3'): float32 in and out, every product formed from
# the operands' three bfloat16 pieces on the bf16 MFMA pipe (csrc/gemm_f32x3.hip).  X3_TERMS = 6 leaves out the three smallest of
# the nine partial products (< 2^-23 of a product each); measured error against float64 BELOW the float32 MFMA kernel's and
# torch's own float32 convolution on every ResNet-50 shape (tools/gpu/gemm_x3_probe.py, tests/test_gpu_gemm_x3.py).
# OPA_GEMM3=0 (or fused.X3_TERMS = 0) takes the choice away.
X3_TERMS = {'0': 0, '6': 6, '9': 9}.get(os.environ.get('OPA_GEMM3', '6'), 6)
FORCE_PICK = os.environ.get('OPA_GEMM3_PICK') or None        # 'x3' | 'conv': every pick() takes that side (tests, A/B)
# ... and the block's LAST 1x1 convolution together with its downsampling convolution as one product (OPA_GEMM3_PAIR=0: off)
X3_PAIR = _switch('OPA_GEMM3_PAIR', '1')
# ... and the STRIDED 3x3 convolutions (the head of ResNet layers 2-4) as an implicit GEMM of the same kernel (OPA_GEMM3_3X3=0: off)
X3_CONV3 = _switch('OPA_GEMM3_3X3', '1')
# ... and the heads' 1x1 convolutions, whose output channels are no multiple of the kernel's 64-wide tile (OPA_GEMM3_HEAD=0: off)
X3_HEAD = _switch('OPA_GEMM3_HEAD', '1')
# ... and the 7x7 stride-2 stem (OPA_GEMM3_STEM=0: off)
X3_STEM = _switch('OPA_GEMM3_STEM', '1')
# ... and the 1x1 convolutions of the ShuffleNetV2K units and conv5, whose channel counts (k16: 24 / 174 / 348 / 696 / 1392) fit none
# of the tiles above and whose operand is a channel slice: the kernel's UNIT mode (OPA_GEMM3_UNIT=0: off)
X3_UNIT = _switch('OPA_GEMM3_UNIT', '1')
# The GROUPED 3x3 convolution of a ResNeXt bottleneck (32 groups of 4 ... 64 channels) as one HIP kernel with the bias and the ReLU
# inside (csrc/gconv.hip); OPA_GCONV=1 (or fused.GCONV = True) switches the route on.  It is never timed and makes no choice-table
# entry: where it is supported it runs.  It stays OFF by default -- torch's grouped convolution + the epilogue pass -- until the
# kernel has been timed against that route on every (group width, stride) class at 641 px (tools/gpu/gconv_times.py): no speed is
# claimed for a route nobody has measured.
GCONV = _switch('OPA_GCONV', '0')
# The MobileNetV3 blocks on the project's kernels (network._InvertedResidual._forward_unit): OPA_MBV3=1 (or fused.MBV3 = True) switches the
# route on.  It stays OFF by default -- the plain torch forward -- until both trunks have been timed against that forward at 641 px,
# batch 32 (tools/gpu/mobilenetv3_times.py): no speed is claimed for a route nobody has measured.
MBV3 = _switch('OPA_MBV3', '0')
# The SqueezeNet Fire modules and max-pools on the project's kernels (network._Fire._forward_unit: the unit-mode GEMM for the squeeze,
# csrc/fire.hip for both expands, their ReLUs and the concatenation; csrc/pool.hip in ceil mode): OPA_FIRE=1 (or fused.FIRE = True)
# switches the route on.  It ships OFF -- the plain torch forward.  Timed once against that forward at 641 px
# (tools/gpu/squeezenet_times.py, profiles/squeezenet/times.log: 3.5 against 6.7 ms at batch 32, 0.50 against 1.00 ms at batch 1,
# trunk + heads); switching the default is a change of its own that rests on that log.
FIRE = _switch('OPA_FIRE', '0')
# ... with NINE terms in both of a Fire's launches, whatever X3_TERMS says (0 still switches the route off: the squeeze is the unit
# mode's).  Nine terms are 1.5 times the MFMA work of six, which counts in the 41 x 41 layers; the times of
# profiles/squeezenet/times.log are of the route as it runs, with nine -- six terms have not been timed.  The pieces of the split
# are truncations, so they have their number's sign and the three products the six-term variant leaves out have the product's: every
# six-term layer shrinks its output by ~3e-8 of its size, and where a float32 rounding error grows with the square root of the
# depth this adds up in proportion to it.  SqueezeNet is 17 such layers in series with K as small as 16: measured
# (tools/gpu/squeezenet_terms.py, profiles/squeezenet/terms.log) the field outputs are 4e-7 ... 6e-7 of their size too small with six
# terms -- 0.9 ... 2.4 times the largest error of torch's own float32 forward -- and 0.4 ... 1.0 times that error with nine.
FIRE_TERMS = 9
# The MobileNetV2 blocks and last convolution on the project's kernels (network._InvertedResidual._forward_unit: the unit-mode GEMM with
# ReLU6 for the expanding convolution, the depthwise stencil with ReLU6, the unit-mode GEMM with the block's input as the residual):
# OPA_MBV2=1 (or fused.MBV2 = True) switches the route on.  It ships OFF -- the plain torch forward; the one timing is
# tools/gpu/mobilenetv2_times.py, profiles/mobilenetv2/times.log, and switching the default is a change of its own that rests on it.
MBV2 = _switch('OPA_MBV2', '0')
# The 1x1 convolutions of a LeakyReLU ShuffleNetV2K unit and a LeakyReLU conv5 through the unit-mode GEMM (the LeakyReLU in its
# epilogue) instead of torch: OPA_UNIT_LEAKY=1 (or fused.UNIT_LEAKY = True).  Off by default, timed by the same tool into the same log.
UNIT_LEAKY = _switch('OPA_UNIT_LEAKY', '0')
# The RGB stem of ShuffleNetV2K, ShuffleNetV2, MobileNetV2, MobileNetV3 and SqueezeNet -- a 3x3 convolution from 3 channels, its folded
# bias and its activation -- as one HIP kernel (csrc/stem.hip, network._stem_forward) instead of torch's convolution + activation:
# OPA_STEM=1 (or fused.STEM = True).  Independent of MBV2 / MBV3 / FIRE / UNIT_LEAKY; never timed, no choice-table entry: where the
# switch is on and ``stem_conv3x3_supported`` the kernel runs.  It ships OFF; the one timing is tools/gpu/stem_times.py,
# profiles/stem/times.log, and switching the default is a change of its own that rests on it.
STEM = _switch('OPA_STEM', '0')
# The group norms of a ShuffleNetV2K built with ``layer_norm='group'`` -- each with the ReLU or LeakyReLU behind it -- as three HIP
# kernels in place on the producer's output (csrc/groupnorm.hip, network._norm_act), the convolutions between them through the unit-mode
# GEMM, the depthwise stencil and (with STEM) the stem kernel without an activation: OPA_GN=1 (or fused.GN = True).  Never timed, no
# choice-table entry: where the switch is on and ``group_norm_supported`` the kernels run, else torch's ``GroupNorm``.  It ships OFF;
# the one timing is tools/gpu/shufflenetv2k_norm_times.py, profiles/shufflenetv2k_norms/times.log.
GN = _switch('OPA_GN', '0')
# The 1x1 convolutions of a ShuffleNetV2K / ShuffleNetV2 cast to bfloat16 (``model.to(torch.bfloat16)``: units, ``conv5``, and a head
# whose input channels are no multiple of 64) through the unit mode of the bf16 GEMM (csrc/gemm_unit_bf16.hip, ``conv1x1_unit_bf16``)
# instead of MIOpen: OPA_UNIT_BF16=1 (or fused.UNIT_BF16 = True).  Never timed by ``pick``, no choice-table entry (the table's 'unit'
# keys are float32's): where the switch is on and ``unit_conv_bf16_supported`` the kernel runs.  It ships OFF; the one timing is
# tools/gpu/unit_bf16_times.py, profiles/unit_bf16/times.log.
UNIT_BF16 = _switch('OPA_UNIT_BF16', '0')
# The 3x3 convolutions of a ResNet cast to bfloat16 (``model.to(torch.bfloat16)``: conv2 of a Bottleneck, both convolutions of a
# BasicBlock, strided ones and the dilated ones of block 5 under ``block5_dilation`` included) as an implicit GEMM on the bf16 MFMA with
# the folded bias, the residual and the ReLU inside (csrc/conv3x3_bf16.hip, ``conv3x3_bias_act_bf16``) instead of MIOpen's convolution
# and a separate epilogue: OPA_CONV3_BF16=1 (or fused.CONV3_BF16 = True).  Never timed by ``pick``, no choice-table entry: where the
# switch is on and ``conv3x3_bf16_supported`` the kernel runs.  It ships OFF; the one timing is tools/gpu/conv3_bf16_times.py,
# profiles/conv3_bf16/times.log, and switching the default is a change of its own that rests on it.
CONV3_BF16 = _switch('OPA_CONV3_BF16', '0')
# The 7x7 RGB stem of a ResNet cast to bfloat16, stride 1 or 2, as an implicit GEMM on the bf16 MFMA with the folded bias and the ReLU
# inside (csrc/stem7x7_bf16.hip, ``stem7x7_bias_act_bf16``) instead of MIOpen's convolution and a separate epilogue pass; the image is
# read where it lies, in any layout: OPA_STEM7_BF16=1 (or fused.STEM7_BF16 = True).  Never timed by ``pick``, no choice-table entry:
# where the switch is on and ``stem7x7_bf16_supported`` the kernel runs.  It ships OFF; the one timing is
# tools/gpu/stem7_bf16_times.py, profiles/stem7_bf16/times.log, and switching the default is a change of its own that rests on it.
STEM7_BF16 = _switch('OPA_STEM7_BF16', '0')
# The downsampling 1x1 convolution of a ResNet cast to bfloat16 -- the first block of every stage -- on the bf16 MFMA
# (csrc/gemm2_bf16.hip) instead of MIOpen: in a Bottleneck together with the block's last 1x1 convolution, the folded bias and the ReLU
# as ONE product (``conv1x1_pair_bias_act_bf16``: the identity tensor is never written, one rounding instead of two), in a BasicBlock
# as the strided 1x1 convolution alone (``conv1x1_strided_bf16``): OPA_PAIR_BF16=1 (or fused.PAIR_BF16 = True).  Never timed by
# ``pick``, no choice-table entry: where the switch is on and ``pair_bf16_supported`` / ``conv1x1_strided_bf16_supported`` the kernel
# runs.  It ships OFF; the one timing is tools/gpu/gemm2_bf16_times.py, profiles/gemm2_bf16/times.log, and switching the default is a
# change of its own that rests on it.
PAIR_BF16 = _switch('OPA_PAIR_BF16', '0')
# The GROUPED 3x3 convolution of a ResNeXt cast to bfloat16 (``model.to(torch.bfloat16)``: conv2 of every Bottleneck, 32 groups of
# 4 ... 64 channels, strided ones and the dilated ones of block 5 under ``block5_dilation`` included) as an implicit GEMM per 64-channel
# chunk on the bf16 MFMA with the folded bias and the ReLU inside (csrc/gconv3x3_bf16.hip, ``gconv3x3_bias_act_bf16``) instead of torch's
# grouped bfloat16 convolution, whose bias and ReLU the next GEMM's operand prologue then owes: OPA_GCONV_BF16=1 (or
# fused.GCONV_BF16 = True).  Never timed by ``pick``, no choice-table entry: where the switch is on and ``gconv3x3_bf16_supported`` the
# kernel runs.  It ships OFF; the one timing is tools/gpu/gconv_bf16_times.py, profiles/gconv_bf16/times.log, and switching the default
# is a change of its own that rests on it.
GCONV_BF16 = _switch('OPA_GCONV_BF16', '0')
# A ResNet cast to FLOAT16 (``model.half()``) on the same kernels, instantiated for the other 16-bit type on v_mfma_f32_32x32x16_f16
# (csrc/bf16_tile.hpp's ``TileElem<1>``): the 1x1 GEMM with the fused epilogue (``conv1x1_bias_act``, choices 'gemm' / 'pass+gemm' /
# 'conv' as for bfloat16), the 3x3 implicit GEMM (``conv3x3_bias_act_bf16``), the block tail + downsampling product and the strided
# 1x1 alone (``conv1x1_pair_bias_act_bf16`` / ``conv1x1_strided_bf16``) -- the ``opa_*_f16`` entry points: OPA_F16=1 (or
# fused.F16 = True).  ONE switch for the three routes, independent of the bfloat16 switches, which a float16 operand never asks
# (``Route16``, below); with it off every predicate declines a float16 operand and the network runs MIOpen's convolutions + ``bias_act_``.
# Never timed by ``pick``.  The 7x7 stem and the grouped 3x3 have float16 forms behind switches of their own (``STEM7_F16``,
# ``GCONV_F16``, below), the max-pool has none (the unit mode has its own switch, ``UNIT_F16``, below); the heads have a 16-bit form
# of their own behind their own switch (``HEAD16``, below), which this one does not touch.  It ships OFF; the one timing is
# tools/gpu/f16_times.py, profiles/f16/times.log, and switching the default is a change of its own that rests on it.
F16 = _switch('OPA_F16', '0')
# The heads of a network cast to bfloat16 or float16 -- the 1x1 convolution AND everything ``CompositeField4`` does behind it -- as ONE
# kernel on the 16-bit MFMA (csrc/head16.hip, ``head_conv_fields16``: ``opa_head_conv_fields_bf16`` / ``..._f16``) instead of torch's
# 16-bit ``Conv2d`` + ``opa_head_epilogue``: the float32 accumulators go through the field function straight to the float32 fields, so
# the convolution's output is neither rounded to 16 bits nor written and read back.  OPA_HEAD16=1 (or fused.HEAD16 = True).  ONE
# switch for both 16-bit types, independent of ``F16`` and the ``*_BF16`` switches (``ROUTE16_HEAD`` names no other).  Never timed by ``pick``,
# no choice-table entry: where the switch is on and ``head_conv_fields16_supported`` the kernel runs.  A head whose input width is no
# multiple of 64 (shufflenetv2k16: 1392) keeps its unit-mode route.  It ships OFF; the one timing is tools/gpu/head16_times.py,
# profiles/head16/times.log, and switching the default is a change of its own that rests on it.
HEAD16 = _switch('OPA_HEAD16', '0')
# A ShuffleNetV2K / ShuffleNetV2 cast to FLOAT16 (``model.half()``) on the kernels its bfloat16 twin takes, instantiated for the other
# 16-bit type: every 1x1 convolution of the units, ``conv5`` and a head whose input channels are no multiple of 64 through the unit mode
# of the 16-bit GEMM on v_mfma_f32_32x32x16_f16 (csrc/gemm_unit_bf16.hip, ``conv1x1_unit_f16``: ``opa_gemm_unit_actp_f16``), every
# depthwise convolution through the stencil (csrc/dwconv.hip: ``opa_dwconv_actp_f16``) instead of MIOpen's convolutions:
# OPA_UNIT_F16=1 (or fused.UNIT_F16 = True).  Independent of ``F16``, ``HEAD16``, ``UNIT_BF16`` and ``UNIT_LEAKY``; with it off
# ``unit_conv_supported`` and ``dwconv_supported`` decline a float16 operand and the network does what it did without the switch.
# Never timed by ``pick``, no choice-table entry.  It ships OFF; the one timing is tools/gpu/unit_f16_times.py,
# profiles/unit_f16/times.log, and switching the default is a change of its own that rests on it.
UNIT_F16 = _switch('OPA_UNIT_F16', '0')
# The GROUPED 3x3 convolution of a ResNeXt cast to FLOAT16 (``model.half()``: what ``GCONV_BF16`` routes for bfloat16) on the same
# kernel instantiated for v_mfma_f32_32x32x16_f16 (csrc/gconv3x3_bf16.hip, ``gconv3x3_bias_act_bf16``: ``opa_gconv3x3_act_f16``) instead
# of torch's grouped float16 convolution: OPA_GCONV_F16=1 (or fused.GCONV_F16 = True).  A switch of its own, independent of ``F16``
# (with which alone a float16 network keeps calling these convolutions), ``HEAD16``, ``UNIT_F16`` and every ``*_BF16`` switch.  Never
# timed by ``pick``, no choice-table entry.  It ships OFF; the one timing is tools/gpu/f16x_times.py, profiles/f16x/times.log, and
# switching the default is a change of its own that rests on it.
GCONV_F16 = _switch('OPA_GCONV_F16', '0')
# The 7x7 RGB stem of a ResNet or ResNeXt cast to FLOAT16 (what ``STEM7_BF16`` routes for bfloat16) on the same kernel instantiated for
# the f16 MFMA (csrc/stem7x7_bf16.hip, ``stem7x7_bias_act_bf16``: ``opa_stem7x7_act_f16``) instead of MIOpen's convolution and a separate
# epilogue pass: OPA_STEM7_F16=1 (or fused.STEM7_F16 = True).  Independent of every other switch, as ``GCONV_F16`` is; the input max-pool
# behind it stays torch's (``maxpool3x3_supported`` declines float16).  It ships OFF; timed by the same tool into the same log.
STEM7_F16 = _switch('OPA_STEM7_F16', '0')


class Route16(typing.NamedTuple):
    """One route on the 16-bit MFMA, and the only place that says which switch and which declined set an element type asks and which
    entry point it takes.  Switches and sets are held by NAME and read from the module when asked: ``fused.GCONV_F16 = True`` acts at once."""
    stem: str                           # the entry points' name without the element type's suffix
    switches: tuple                     # per element type (bfloat16, float16) the name of the switch; None: always on
    declined: tuple = (None, None)      # per element type the name of the ``*_DECLINED`` set; None: there is none
    stem_pro: str = None                # the 1x1 GEMM's second entry point: the one with the operand prologue

    def suffix(self, dtype):
        """``'_bf16'`` / ``'_f16'`` where the route is on for operands of ``dtype`` as its switch reads NOW; None: off, or another dtype.
        A float16 operand never asks a bfloat16 switch, a bfloat16 one never a float16 switch."""
        i = _ELEMENTS16.get(dtype)
        if i is None:
            return None
        return _SUFFIXES16[i] if self.switches[i] is None or globals()[self.switches[i]] else None

    def symbol(self, dtype, pro=False):
        return (self.stem_pro if pro else self.stem) + _SUFFIXES16[_ELEMENTS16[dtype]]

    def declined_set(self, dtype):
        """The keys measured slower that the route's predicate declines for ``dtype``, as the set reads NOW."""
        name = self.declined[_ELEMENTS16[dtype]]
        return globals()[name] if name else frozenset()


_ELEMENTS16, _SUFFIXES16 = {torch.bfloat16: 0, torch.float16: 1}, ('_bf16', '_f16')
ROUTE16_GEMM = Route16('opa_gemm_bias_act', (None, 'F16'), stem_pro='opa_gemm_pro_bias_act')
ROUTE16_CONV3 = Route16('opa_conv3x3_act', ('CONV3_BF16', 'F16'))
ROUTE16_PAIR = Route16('opa_gemm2_bias_act', ('PAIR_BF16', 'F16'), ('PAIR_BF16_DECLINED', 'PAIR_BF16_DECLINED'))      # the strided 1x1 too
ROUTE16_GCONV = Route16('opa_gconv3x3_act', ('GCONV_BF16', 'GCONV_F16'), ('GCONV_BF16_DECLINED', 'GCONV_F16_DECLINED'))
ROUTE16_STEM7 = Route16('opa_stem7x7_act', ('STEM7_BF16', 'STEM7_F16'), (None, 'STEM7_F16_DECLINED'))
ROUTE16_HEAD = Route16('opa_head_conv_fields', ('HEAD16', 'HEAD16'), ('HEAD16_DECLINED', 'HEAD16_DECLINED'))


# ---- the choice table and the decision ---------------------------------------------------------------------------------------------

# (dtype, M, K, N, has_residual, has_a_bias) -> 'gemm' | 'gemm3' | 'pass+gemm' | 'conv', and for ``pick``
# ('torch.float32/<kind>', M, K, N, flag, flag) -> 'x3' | 'conv'.  The paths round
# differently, so the choice is part of the result: it is made once per shape (the key holds no device index: a
# table exported on rank 0 must match the lookups of every other rank), never by timing while a stream is being
# captured (timing synchronises; the capture-time default is remembered, so a captured graph and a later eager
# run use the same kernel), can be pinned with OPA_CONV1X1=gemm|conv, and can be exported / imported
# (choices / set_choices; distributed.broadcast_conv_choices) so that every rank of a job runs the same kernels.
_CHOICE = {}
PINNED_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'conv1x1_pinned.json')


def load_pinned(path=None):
    """The table the package ships (``conv1x1_pinned.json``: measured on an MI355X by ``tools/gpu/dump_conv_choices.py`` for the
    shapes of the BASELINE configurations, float32 and bfloat16): the same choice on every rank of a multi-GPU job WITHOUT a
    collective (round 5 broadcast rank 0's wall-clock choices, ``distributed.broadcast_conv_choices``).  Loaded when this module
    is imported; entries made later (``set_choices``, timing) go on top.  -> number of entries adopted."""
    import json
    try:
        with open(path or PINNED_FILE) as f:
            table = json.load(f)['table']
    except (OSError, ValueError, KeyError):
        return 0
    for dtype, m, k, n, res, a_bias, choice in table:
        _CHOICE.setdefault((dtype, int(m), int(k), int(n), bool(res), bool(a_bias)), choice)
    return len(table)


def _in_multi_rank_job():
    try:
        import torch.distributed as dist
        return dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    except Exception:              # noqa: BLE001
        return False


def choices():
    return dict(_CHOICE)


def set_choices(table, *, replace=False):
    if replace:
        _CHOICE.clear()
    _CHOICE.update(table)


def _time_ms(fn, reps=3):
    """Best of two rounds of ``reps`` calls (one round alone flips close calls between runs: third session, batch-1 shapes)."""
    fn()
    torch.cuda.synchronize()
    best = None
    for _ in range(2):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(reps):
            fn()
        end.record()
        end.synchronize()
        ms = start.elapsed_time(end) / reps
        best = ms if best is None or ms < best else best
    return best


def _decide(key, default, timed, may_time=True):
    """The choice for ``key``: the table's entry; else ``default`` where timing is not an option -- ``may_time`` is false, a stream is
    being captured (timing synchronises), or the job has several ranks (wall clocks differ from rank to rank and the candidates
    round differently: every rank takes the SAME default, no collective needed) -- else the fastest of ``timed()``, a callable that
    times every candidate once and returns ``{name: ms}`` (the first listed wins a tie).  Whatever was chosen is remembered, so
    that a captured graph and a later eager run use the same kernel."""
    choice = _CHOICE.get(key)
    if choice is None:
        if not may_time or torch.cuda.is_current_stream_capturing() or _in_multi_rank_job():
            choice = default
        else:
            times = timed()
            choice = min(times, key=times.get)
        _CHOICE[key] = choice
    return choice


def pick(kind, m, k, n, flag_a, flag_b, run_x3, run_other, written=None, timing=True):
    """One of two ways to compute the same tensor -- a split-operand kernel (``run_x3``) or what the trunk did before
    (``run_other``: MIOpen's convolution + the fused passes) -- chosen ONCE per shape like ``conv_bias_act`` chooses its GEMM: from
    the shipped table (``conv1x1_pinned.json``, key dtype ``'torch.float32/<kind>'``), else by timing both on the first call; while
    a stream is being captured or in a job of several ranks, where timing is not an option, by size (the split-operand kernels win
    from ~16 000 output pixels: a batch of one 641-px image keeps MIOpen in layers 3-4).  Returns the chosen function's result.
    ``written``: an operand that ``run_other`` changes in place (the epilogue its producer left to this consumer); timing calls
    ``run_other`` several times, so the operand is saved before and put back after -- the winner computes from what the caller
    passed, whoever wins.  ``timing=False``: a shape the table does not know is decided by size ALWAYS -- eager or capturing, one
    rank or many -- and nothing is timed (measurements go into the table: ``tools/gpu/dump_conv_choices.py``)."""
    if FORCE_PICK in ('x3', 'conv'):
        return run_x3() if FORCE_PICK == 'x3' else run_other()

    def timed():
        saved = written.clone() if written is not None else None
        times = {'x3': _time_ms(run_x3), 'conv': _time_ms(run_other)}
        if saved is not None:
            written.copy_(saved)
        return times
    key = ('torch.float32/' + kind, int(m), int(k), int(n), bool(flag_a), bool(flag_b))
    choice = _decide(key, 'x3' if m >= 16384 else 'conv', timed, may_time=timing)
    return run_x3() if choice == 'x3' else run_other()


# ---- layouts, sizes and what else the predicates share ------------------------------------------------------------------------------

def _nhwc_rows(x):
    """(rows, channels) if ``x`` is physically [rows, channels]-contiguous, else None."""
    if x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last):
        return x.shape[0] * x.shape[2] * x.shape[3], x.shape[1]
    if x.dim() == 2 and x.is_contiguous():
        return x.shape[0], x.shape[1]
    return None


def _pixel_stride(x):
    """Elements between neighbouring pixels of a channels-innermost (NHWC in memory) 4-d tensor or channel slice of
    one; None if ``x`` is laid out differently."""
    if x.dim() != 4 or x.stride(1) != 1:
        return None
    B, C, H, W = x.shape
    ps = x.stride(3) if W > 1 else (x.stride(2) if H > 1 else C)
    if ps < C or (H > 1 and x.stride(2) != W * ps) or (B > 1 and x.stride(0) != H * W * ps):
        return None
    return ps


def _out_hw(x, stride=1):
    return (x.shape[2] - 1) // stride + 1, (x.shape[3] - 1) // stride + 1


def out_pixels(x, stride=1):
    """Pixels of the whole batch behind a convolution of ``x`` with "same" padding and this stride: the M of the choice table's keys."""
    ho, wo = _out_hw(x, stride)
    return x.shape[0] * ho * wo


def _empty_nhwc(x, channels, hw=None, dtype=None):
    """An uninitialised channels-last ``[B, channels, *hw]`` on ``x``'s device (``hw``: ``x``'s own where not given)."""
    h, w = hw or x.shape[2:]
    return torch.empty((x.shape[0], channels, h, w), dtype=dtype or x.dtype, device=x.device, memory_format=torch.channels_last)


def _autograd_follows(*tensors):
    """Grad is enabled and one of ``tensors`` (None allowed) requires grad: the kernels have no backward."""
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _folded_bias_ok(bias, n, x):
    """The folded bias a 16-bit route takes: None, or ``n`` elements in one dimension on ``x``'s device, of ``x``'s dtype or float32."""
    return bias is None or (bias.dtype in (x.dtype, torch.float32) and bias.device == x.device and bias.dim() == 1 and bias.numel() == n)


def _bias_f32(bias):
    """``bias`` as the launch takes it: float32 (a 16-bit one upcast exactly), contiguous; None stays None."""
    return None if bias is None else bias.detach().to(torch.float32).contiguous()


def _dense_bf16(t, channels, dtype):
    """``t``: a dense channels-last 16-bit ``[B, channels, H, W]`` of ``dtype`` on the GPU, 16-byte aligned?"""
    return (t.is_cuda and t.dtype == dtype and t.dim() == 4 and t.shape[1] == channels
            and t.is_contiguous(memory_format=torch.channels_last) and t.data_ptr() % 16 == 0)


# ---- derived operands -----------------------------------------------------------------------------------------------------------------

def _capturing():
    """Is the current stream being captured into a HIP graph?  False where no GPU was initialised: nothing can be capturing there,
    and asking would raise on a machine without one."""
    return torch.cuda.is_initialized() and torch.cuda.is_current_stream_capturing()


def _refreshable(kept, new):
    """Can ``_refresh_(kept, new)`` write ``new`` -- what ``make()`` returned now -- into ``kept``, what it returned before?  Tensors of
    one shape, dtype, device and layout (an inference tensor only inside inference mode), None for None, a tuple or list element
    by element, anything else where it compares equal."""
    if isinstance(kept, torch.Tensor) or isinstance(new, torch.Tensor):
        return (isinstance(kept, torch.Tensor) and isinstance(new, torch.Tensor) and kept.shape == new.shape and kept.dtype == new.dtype
                and kept.device == new.device and kept.stride() == new.stride()
                and (not kept.is_inference() or torch.is_inference_mode_enabled()))
    if isinstance(kept, (tuple, list)):
        return type(kept) is type(new) and len(kept) == len(new) and all(_refreshable(k, n) for k, n in zip(kept, new))
    return type(kept) is type(new) and kept == new


def _refresh_(kept, new):
    if isinstance(kept, torch.Tensor):
        with torch.no_grad():
            kept.copy_(new)
    elif isinstance(kept, (tuple, list)):
        for k, n in zip(kept, new):
            _refresh_(k, n)


def derived(module, name, sources, make):
    """``make()`` -- an operand derived from the tensors ``sources`` (parameters, buffers; None where there is none): a tensor, or a
    tuple of tensors and None -- computed once, kept on ``module`` as attribute ``name`` and brought up to date whenever a source was
    replaced, moved, converted or changed in place (``load_state_dict``, ``.to()``, an optimizer step): the key is (data pointer,
    device, dtype, shape) and the version counter of each.  The entry holds on to the sources' storages, so that no later tensor can
    be handed the same address while it is the key.  A HIP graph bakes the ADDRESS of whatever a launch is handed, hence:

    (i)   an operand made while a stream is being captured is NOT kept (it lives in the graph's private pool and holds nothing
          until the first replay): the graph computes it again on every replay from the parameters it read -- it follows them as
          torch's own modules do -- and an eager call makes and keeps its own;
    (ii)  where every source still has the pointer, device, dtype and shape of the key and only version counters rose, the kept
          tensors are OVERWRITTEN IN PLACE with ``make()``'s new values: an address in a graph stays valid and sees the new weights
          (outside a capture: a stale entry met while capturing is left alone, and the call goes by (i));
    (iii) where a source was replaced (``.to()``, ``.half()``, a new ``Parameter``) the entry is replaced: a graph captured over the
          old parameters must be captured again, as with any torch module."""
    where = tuple(None if t is None else (t.data_ptr(), str(t.device), t.dtype, t.shape) for t in sources)
    key = (where, tuple(None if t is None else t._version for t in sources))
    cached = getattr(module, name, None)
    if cached is not None and cached[0] == key:
        return cached[1]
    value = make()
    if _capturing():
        return value
    if cached is not None and cached[0][0] == where and _refreshable(cached[1], value):
        _refresh_(cached[1], value)
        value = cached[1]
    setattr(module, name, (key, value, [t.untyped_storage() for t in sources if t is not None]))
    return value


def split_weight(weight2d):
    """``[N, K]`` float32 -> ``[3, N, K]`` bfloat16: the three pieces of every weight (its 24-bit significand cut into 8 + 8 + 8
    bits: ``w1`` = ``w`` with the low 16 bits cleared, ``r = w - w1``, ``w2`` = ``r`` with the low 16 bits cleared, ``w3 = r - w2``;
    every step is exact and ``w1 + w2 + w3 == w`` bit for bit) -- the operand of ``opa_gemm_bias_act_f32x3`` (``csrc/gemm_f32x3.hip``)."""
    w = weight2d.detach().to(torch.float32).contiguous()

    def top(x):
        return (x.view(torch.int32) & -65536).view(torch.float32)
    w1 = top(w)
    r1 = w - w1
    w2 = top(r1)
    w3 = r1 - w2
    out = torch.stack((w1, w2, w3)).to(torch.bfloat16)          # (exact: each piece has at most 8 significant bits)
    return out.contiguous()


def split_weight_3x3(weight):
    """``[N, C, 3, 3]`` float32 -> ``split_weight`` of ``[N, (ky, kx, c)]``: the operand of ``opa_conv3x3_f32x3``."""
    n, c = weight.shape[0], weight.shape[1]
    return split_weight(weight.detach().permute(0, 2, 3, 1).reshape(n, 9 * c))


def _split_weight_of(conv, w2d):
    """``split_weight(w2d)`` for ``w2d``, the ``[N, K]`` view of ``conv.weight``: computed once per convolution and kept on the module
    (inference: the weight does not change; a weight replaced, moved or changed since is split again)."""
    return derived(conv, '_opa_w3', (conv.weight,), lambda: split_weight(w2d))


def _split_weight_3x3_of(conv):
    """``split_weight_3x3(conv.weight)``, kept on the module like ``_split_weight_of``."""
    return derived(conv, '_opa_w3_3x3', (conv.weight,), lambda: split_weight_3x3(conv.weight))


def _pair_weight_of(conv, dconv, a_bias=None):
    """The operands of ``conv1x1_pair_bias_act_x3`` derived from the current parameters: ``split_weight([W | Wd])`` and ``a_bias``
    followed by zeros for ``dconv``'s channels (None without ``a_bias``) -- kept on ``conv`` like ``_split_weight_of``."""
    k1, k2, n = conv.in_channels, dconv.in_channels, conv.out_channels

    def make():
        w1, w2 = conv.weight.detach().reshape(n, k1), dconv.weight.detach().reshape(n, k2)
        ab = None if a_bias is None else torch.cat((a_bias.detach().float(), torch.zeros(k2, device=a_bias.device)))
        return split_weight(torch.cat((w1, w2), dim=1)), ab
    return derived(conv, '_opa_w3_pair', (conv.weight, dconv.weight, a_bias), make)


def _stem_weight_of(conv):
    """The weight operand of ``stem7x7_bias_act_x3`` derived from the current ``conv.weight``: ``[N, 7, 7, 3]`` padded with zeros to
    ``[N, 8, 8, 4]`` and split -- kept on the module like ``_split_weight_of``."""
    def make():
        w = conv.weight
        n = w.shape[0]
        wp = torch.zeros((n, 8, 8, 4), dtype=torch.float32, device=w.device)
        wp[:, :7, :7, :3] = w.detach().permute(0, 2, 3, 1)
        return split_weight(wp.reshape(n, 256))
    return derived(conv, '_opa_w3_stem', (conv.weight,), make)


def _unit_operands_of(mode, conv):
    """The operands of ``conv1x1_unit`` (float32: of ``head_conv_x3`` too) derived from the current parameters: the ``[N, K]`` weight in
    ``mode``'s dtype padded with zeros to ``[N_pad, K_pad]`` (multiples of 64: the kernel's tile width and two of its K-steps) as
    ``mode.weight`` lays it out -- float32 ``split_weight``'s ``[3, N_pad, K_pad]``, bfloat16 and float16 as it is -- and the bias as FLOAT32
    ``[N_pad]`` (a 16-bit bias upcast exactly; zeros where the convolution has none and in the padding) -- kept on the module as ``mode.cache``
    like ``_split_weight_of``; the convolution keeps its parameters, and the key holds the bias tensor too (a bias REPLACED by a new
    Parameter is a new operand)."""
    def make():
        w = conv.weight
        n, k = w.shape[0], w.shape[1]
        npad, kpad = (n + 63) // 64 * 64, (k + 63) // 64 * 64
        wp = torch.zeros((npad, kpad), dtype=mode.dtype, device=w.device)
        wp[:n, :k] = w.detach().reshape(n, k)
        bp = torch.zeros(npad, dtype=torch.float32, device=w.device)
        if conv.bias is not None:
            bp[:n] = conv.bias.detach()
        return mode.weight(wp), bp
    return derived(conv, mode.cache, (conv.weight, conv.bias), make)


def gconv_weight_of(conv):
    """The operand of ``opa_gconv3x3_bias_act_f32`` derived from the CURRENT ``conv.weight`` (``[C, cg, 3, 3]``): tap-major with the
    output channel innermost, ``[9, cg, C]`` with ``wt[ky * 3 + kx][ci][co] = weight[co][ci][ky][kx]``.  Derived and cached
    (``derived``): no buffer, no part of a state dict, computed again whenever the weight was replaced, moved or changed in place."""
    def make():
        w = conv.weight.detach()
        return w.permute(2, 3, 1, 0).reshape(9, w.shape[1], w.shape[0]).contiguous()
    return derived(conv, '_opa_gconv_wt', (conv.weight,), make)


def depthwise_taps(weight):
    """``[C, 1, k, k]`` -> ``[k * k, C]``, tap-major: the weight operand of ``dwconv_bias_act``."""
    return weight.detach().reshape(weight.shape[0], -1).t().contiguous()


# ---- the epilogue passes --------------------------------------------------------------------------------------------------------------

def bias_act_(x, bias, residual=None, relu=True):
    """In place ``x = act(x + bias[c] (+ residual))`` for a channels_last activation.

    One HIP kernel on the GPU; the equivalent PyTorch ops elsewhere (CPU tests, odd layouts)."""
    rc = _nhwc_rows(x) if x.is_cuda else None
    per_vec = 4 if x.dtype == torch.float32 else 8
    ok = (rc is not None and x.dtype in _DTYPES and rc[1] % per_vec == 0 and bias.dtype == x.dtype
          and bias.is_contiguous() and x.data_ptr() % 16 == 0 and bias.data_ptr() % 16 == 0
          and (residual is None or (residual.dtype == x.dtype and residual.shape == x.shape
                                    and _nhwc_rows(residual) is not None and residual.data_ptr() % 16 == 0)))
    if not ok:
        x.add_(bias.view(1, -1, 1, 1) if x.dim() == 4 else bias)
        if residual is not None:
            x.add_(residual)
        return torch.relu_(x) if relu else x
    _launch('opa_bias_act', _ptr(x), _ptr(bias), _ptr(residual), rc[0], rc[1], _DTYPES[x.dtype], int(bool(relu)))
    return x


def channel_interleave(a, b):
    """``channel_shuffle(torch.cat((a, b), 1), groups=2)`` in one pass: out[:, 2i] = a[:, i], out[:, 2i+1] = b[:, i]."""
    pa, pb = _pixel_stride(a), _pixel_stride(b)
    if not (a.is_cuda and a.dtype in _DTYPES and a.dtype == b.dtype and a.shape == b.shape and pa and pb
            and _lib.available()):
        x = torch.cat((a, b), dim=1)
        n, c, h, w = x.shape
        return x.view(n, 2, c // 2, h, w).transpose(1, 2).reshape(n, c, h, w)
    B, half, H, W = a.shape
    out = _empty_nhwc(a, 2 * half)
    _launch('opa_channel_interleave', _ptr(a), pa, _ptr(b), pb, _ptr(out), B * H * W, half, _DTYPES[a.dtype])
    return out


def head_epilogue_supported(x, meta, training=False):
    """True if :func:`head_epilogue` can run for this convolution output and head meta."""
    us = meta.upsample_stride
    return (not training and x.is_cuda and x.dim() == 4 and x.dtype in _DTYPES and _lib.available()
            and not _autograd_follows(x)
            and x.is_contiguous(memory_format=torch.channels_last) and us in (1, 2)
            and x.shape[1] % (us ** 2) == 0 and x.data_ptr() % 16 == 0
            and 16 * us * us * (x.shape[3] + 1) * 4 <= 64 * 1024)           # the kernel's LDS row buffer (head.hip)


def head_epilogue(x, meta):
    """Everything ``CompositeField4`` does after its 1x1 convolution, in ONE kernel (reference
    ``network/heads.py:330-378``): PixelShuffle -> crop -> ``[B, F, C, H, W]`` float32 -> sigmoid / index offsets /
    softplus.  ``x``: the convolution output ``[B, F*C*us^2, hc, wc]``, channels_last."""
    B, ctot, hc, wc = x.shape
    us = meta.upsample_stride
    n_comp = 1 + meta.n_confidences + meta.n_vectors * 2 + meta.n_scales
    n_fields = ctot // (n_comp * us * us)
    low_cut = (us - 1) // 2
    high_cut = us - 1 - low_cut
    H, W = hc * us - low_cut - high_cut, wc * us - low_cut - high_cut
    out = torch.empty((B, n_fields, n_comp, H, W), dtype=torch.float32, device=x.device)
    mask = sum(1 << i for i, on in enumerate(meta.vector_offsets) if on)
    _launch('opa_head_epilogue', _ptr(x), _DTYPES[x.dtype], B, hc, wc, n_fields, n_comp, us, meta.n_confidences,
            meta.n_vectors, mask, meta.n_scales, _ptr(out))
    return out


# ---- a 16-bit head in one kernel ------------------------------------------------------------------------------------------------------

HEAD16_TILE_N = 64                        # kHead16BN: the weight's rows and the bias are padded to it
# (k, n, upsample) of heads that ``opa_head_conv_fields_bf16`` / ``..._f16`` can run but that came out SLOWER at batch 32 than what runs
# with the switch off (tools/gpu/head16_times.py, profiles/head16/times.log): the predicate declines them.
HEAD16_DECLINED = frozenset()


def head16_operands_of(conv):
    """The operands of ``head_conv_fields16`` derived from the CURRENT parameters of a head's 1x1 convolution (16-bit ``[N, K, 1, 1]``
    and ``[N]``): the weight as ``[Np][K]`` of its dtype, K-major, ``Np`` = ``N`` rounded up to ``HEAD16_TILE_N``, ZEROS in the rows from
    ``N`` on, and the bias as FLOAT32 ``[Np]`` (upcast exactly, zeros behind ``N``).  Kept on ``conv`` by ``derived``, keyed on both tensors."""
    def make():
        w = conv.weight.detach()
        n, k = w.shape[0], w.shape[1]
        npad = (n + HEAD16_TILE_N - 1) // HEAD16_TILE_N * HEAD16_TILE_N
        wp = torch.zeros((npad, k), dtype=w.dtype, device=w.device)
        wp[:n] = w.reshape(n, k)
        bp = torch.zeros(npad, dtype=torch.float32, device=w.device)
        bp[:n] = conv.bias.detach()
        return wp, bp
    return derived(conv, '_opa_head16', (conv.weight, conv.bias), make)


def _head16_shape(conv, x, meta):
    """(n_components, H, W) of the fields that ``conv`` and ``meta`` make of ``x``."""
    us = meta.upsample_stride
    return (1 + meta.n_confidences + meta.n_vectors * 2 + meta.n_scales, x.shape[2] * us - (us - 1), x.shape[3] * us - (us - 1))


def head_conv_fields16_supported(conv, x, meta, training=False):
    """Can ``head_conv_fields16(conv, x, meta)`` run?  The switch ``HEAD16`` on and the library built; not training; ``x`` a dense
    channels-last bfloat16 or float16 ``[B, K, hc, wc]`` on the GPU, 16-byte aligned, with pixels; weight and bias of ``x``'s dtype on its
    device (autocast's float32 parameters are declined), outside autocast, nothing that autograd follows; ``conv`` 1x1, stride 1, no
    padding or dilation, one group, with a bias; ``K % 64 == 0``; ``meta.upsample_stride`` 1 or 2 and ``conv.out_channels`` the
    ``n_fields * n_components * upsample^2`` of ``meta``'s counts, none negative; ``x`` and the fields fewer than 2^31 elements each;
    ``(K, N, upsample)`` not in ``HEAD16_DECLINED``.  No limit on the row width: nothing here buffers a row."""
    if not (not training and ROUTE16_HEAD.suffix(x.dtype) and x.is_cuda and not torch.is_autocast_enabled()
            and isinstance(conv, torch.nn.Conv2d) and conv.bias is not None):
        return False
    w, b = conv.weight, conv.bias
    if not (w.dtype == x.dtype == b.dtype and w.device == x.device == b.device and not _autograd_follows(x, w, b)):
        return False
    k, n, us = conv.in_channels, conv.out_channels, meta.upsample_stride
    if not (conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.padding == (0, 0) and conv.dilation == (1, 1) and conv.groups == 1
            and k % 64 == 0 and us in (1, 2) and _dense_bf16(x, k, x.dtype) and x.shape[2] > 0 and x.shape[3] > 0):
        return False
    counts = (meta.n_fields, meta.n_confidences, meta.n_vectors, meta.n_scales)
    n_comp, H, W = _head16_shape(conv, x, meta)
    if not (meta.n_fields > 0 and min(counts) >= 0 and len(meta.vector_offsets) <= 32 and n == meta.n_fields * n_comp * us * us):
        return False
    return (x.numel() < 2 ** 31 and x.shape[0] * meta.n_fields * n_comp * H * W < 2 ** 31 and _lib.available()
            and (k, n, us) not in ROUTE16_HEAD.declined_set(x.dtype))


def head_conv_fields16(conv, x, meta):
    """A 16-bit head in ONE launch (``opa_head_conv_fields_bf16`` / ``..._f16``, csrc/head16.hip): ``conv``, the head's 1x1 convolution,
    on the 16-bit MFMA with float32 accumulation and, on the float32 sums, everything ``CompositeField4`` does behind it (reference
    ``network/heads.py:330-378``: PixelShuffle -> crop -> sigmoid / index offsets / softplus; ``head_epilogue``'s arithmetic, one device
    function for both) -> ``[B, F, C, H, W]`` float32.  The convolution's output is never rounded to 16 bits and never written.
    ``head_conv_fields16_supported`` says whether this can run."""
    wp, bp = head16_operands_of(conv)
    B, k, hc, wc = x.shape
    n_comp, H, W = _head16_shape(conv, x, meta)
    out = torch.empty((B, meta.n_fields, n_comp, H, W), dtype=torch.float32, device=x.device)
    mask = sum(1 << i for i, on in enumerate(meta.vector_offsets) if on)
    _launch(ROUTE16_HEAD.symbol(x.dtype), _ptr(x), _ptr(wp), _ptr(bp), _ptr(out), B, hc, wc, k, meta.n_fields, n_comp,
            meta.upsample_stride, meta.n_confidences, meta.n_vectors, mask, meta.n_scales)
    return out


# ---- the 1x1 GEMMs --------------------------------------------------------------------------------------------------------------------

def conv1x1_supported(x, weight, bias=None, residual=None, a_bias=None):
    """True if ``conv1x1_bias_act`` can run the HIP GEMM for these operands.  The kernels read raw buffers:
    EVERY operand must have the activation's dtype, bfloat16, float32 or -- with ``F16`` -- float16 (autocast keeps
    parameters in float32 next to 16-bit activations -- those take the PyTorch path), the activation channels_last,
    the residual channels_last of the output's shape."""
    dt = x.dtype
    if not (x.is_cuda and (dt == torch.float32 or ROUTE16_GEMM.suffix(dt)) and x.dim() == 4
            and x.is_contiguous(memory_format=torch.channels_last)
            and weight.dtype == dt and weight.is_cuda
            and weight.shape[1] % (32 if dt == torch.float32 else 64) == 0 and weight.shape[0] % 64 == 0
            and weight.shape[1] == x.shape[1]):
        return False
    # (float16 asks what the other routes of its switch ask: outside autocast, nothing that autograd follows; the bfloat16 and the
    # float32 GEMM keep their contract as it was)
    if dt == torch.float16 and (torch.is_autocast_enabled() or _autograd_follows(x, weight, bias, residual, a_bias)):
        return False
    for vec, n in ((bias, weight.shape[0]), (a_bias, weight.shape[1])):
        if vec is not None and not (vec.dtype == dt and vec.is_cuda and vec.is_contiguous()
                                    and vec.numel() == n and vec.data_ptr() % 16 == 0):
            return False
    if residual is not None and not (residual.dtype == dt and residual.is_cuda
                                     and tuple(residual.shape) == (x.shape[0], weight.shape[0], x.shape[2], x.shape[3])
                                     and residual.is_contiguous(memory_format=torch.channels_last) and residual.data_ptr() % 16 == 0):
        return False
    return x.data_ptr() % 16 == 0 and weight.data_ptr() % 16 == 0


def conv1x1_bias_act(x, weight2d, bias, residual=None, relu=True, a_bias=None):
    """``act(conv1x1(x, weight) + bias (+ residual))`` as ONE MFMA GEMM kernel with fused epilogue.

    :param x: ``[B, C_in, H, W]`` bfloat16, float16 or float32, channels_last
    :param weight2d: ``[C_out, C_in]`` of the same dtype, contiguous
    :param a_bias: ``[C_in]``: ``x`` is the RAW output of the preceding convolution and
        ``relu(x + a_bias)`` -- that convolution's epilogue -- is applied while the operand is staged
    :returns: ``[B, C_out, H, W]`` of that dtype, channels_last
    """
    N, K = weight2d.shape[0], x.shape[1]
    out = _empty_nhwc(x, N)
    rest = (_ptr(weight2d), _ptr(bias), _ptr(residual), _ptr(out), out_pixels(x), N, K, int(bool(relu)))
    if x.dtype == torch.float32:
        _launch('opa_gemm_bias_act_f32', _ptr(x), _ptr(a_bias), *rest)
    elif a_bias is not None:
        _launch(ROUTE16_GEMM.symbol(x.dtype, pro=True), _ptr(x), _ptr(a_bias), *rest)
    else:
        _launch(ROUTE16_GEMM.symbol(x.dtype), _ptr(x), *rest)
    return out


def conv1x1_bias_act_x3(x, w3, bias, residual=None, relu=True, a_bias=None, terms=9):
    """``conv1x1_bias_act`` for float32 through the split-operand kernel: ``w3`` = ``split_weight(weight2d)``; ``terms`` 9 or 6."""
    N, K = w3.shape[1], x.shape[1]
    out = _empty_nhwc(x, N)
    _launch('opa_gemm_bias_act_f32x3', _ptr(x), _ptr(a_bias), _ptr(w3), _ptr(bias), _ptr(residual), _ptr(out),
            out_pixels(x), N, K, int(bool(relu)), int(terms))
    return out


def _x3_supported(x, weight):
    return X3_TERMS in (6, 9) and x.dtype == torch.float32 and weight.shape[1] % 64 == 0


def conv_bias_act(conv, x, bias, residual=None, relu=True, a_bias=None):
    """``act(conv(x) + bias (+ residual))`` for a bias-free ``conv`` module: 1x1 stride-1 convolutions go
    to the fused MFMA GEMM when it is faster than MIOpen's convolution + the fused epilogue pass
    (decided once per shape by timing both on the first call); everything else is conv + ``bias_act_``.

    With ``a_bias``, ``x`` is the raw output of the preceding convolution whose epilogue
    ``relu(x + a_bias[c])`` has not been applied yet: the GEMM applies it to its operand on the fly, the
    fallback applies it in place first."""
    w = conv.weight
    if (conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.groups == 1 and conv.padding == (0, 0)
            and conv1x1_supported(x, w, bias, residual, a_bias)):
        key = (str(x.dtype), out_pixels(x), w.shape[1], w.shape[0], residual is not None, a_bias is not None)
        w2d = w.reshape(w.shape[0], w.shape[1])
        if not w2d.is_contiguous():
            w2d = w2d.contiguous()

        def timed():
            times = {'gemm': _time_ms(lambda: conv1x1_bias_act(x, w2d, bias, residual, relu, a_bias))}
            if _x3_supported(x, w):
                w3 = _split_weight_of(conv, w2d)
                times['gemm3'] = _time_ms(lambda: conv1x1_bias_act_x3(x, w3, bias, residual, relu, a_bias, X3_TERMS))
            if a_bias is None:
                times['conv'] = _time_ms(lambda: bias_act_(conv(x), bias, residual, relu))
            else:       # timing only: the separate epilogue pass runs on a scratch copy
                scratch = x.clone()
                times['pass+gemm'] = _time_ms(
                    lambda: conv1x1_bias_act(bias_act_(scratch, a_bias), w2d, bias, residual, relu))
                times['conv'] = _time_ms(lambda: bias_act_(conv(bias_act_(scratch, a_bias)), bias, residual, relu))
            return times
        # OPA_CONV1X1=gemm|conv (read at the call) pins a shape the table does not know; the default where nothing may be timed: 'gemm'
        forced = os.environ.get('OPA_CONV1X1', 'auto')
        pinned = forced in ('gemm', 'conv')
        choice = _decide(key, forced if pinned else 'gemm', timed, may_time=not pinned)
        if choice == 'gemm3' and not _x3_supported(x, w):
            choice = 'gemm'                  # (switched off after the table was made: the float32 MFMA kernel)
        if choice == 'gemm3':
            return conv1x1_bias_act_x3(x, _split_weight_of(conv, w2d), bias, residual, relu, a_bias, X3_TERMS)
        if choice == 'gemm':
            return conv1x1_bias_act(x, w2d, bias, residual, relu, a_bias)
        if choice == 'pass+gemm':     # the prologue's VALU work is repeated per N-tile: cheaper as its own pass here
            return conv1x1_bias_act(bias_act_(x, a_bias), w2d, bias, residual, relu)
    if a_bias is not None:
        x = bias_act_(x, a_bias)
    return bias_act_(conv(x), bias, residual, relu)


# ---- the split-operand convolutions: pair, strided 3x3, stem, heads; the unit mode, float32 and bfloat16 --------------------------------

def pair_supported(conv, dconv, h, x, bias, a_bias=None):
    """Can ``conv(h) + dconv(x)`` run as ONE split-operand product (``conv1x1_pair_bias_act_x3``)?  float32, channels_last,
    both 1x1 without bias / groups / padding, ``conv`` of stride 1, ``dconv`` of any stride."""
    k1, k2 = conv.in_channels, dconv.in_channels
    ok = (X3_PAIR and X3_TERMS in (6, 9) and h.is_cuda and h.dtype == torch.float32 and x.dtype == torch.float32
          and conv.kernel_size == (1, 1) and dconv.kernel_size == (1, 1) and conv.stride == (1, 1) and dconv.stride[0] == dconv.stride[1]
          and conv.groups == 1 and dconv.groups == 1 and conv.padding == (0, 0) and dconv.padding == (0, 0)
          and conv.bias is None and dconv.bias is None and conv.out_channels == dconv.out_channels
          and k1 % 32 == 0 and (k1 + k2) % 64 == 0 and k2 % 4 == 0 and conv.out_channels % 64 == 0
          and h.dim() == 4 and x.dim() == 4 and h.is_contiguous(memory_format=torch.channels_last)
          and x.is_contiguous(memory_format=torch.channels_last) and h.shape[1] == k1 and x.shape[1] == k2
          and h.shape[0] == x.shape[0] and h.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0
          and bias.dtype == torch.float32 and bias.is_contiguous() and bias.data_ptr() % 16 == 0
          and x.shape[0] * x.shape[2] * x.shape[3] < 2 ** 31)
    if not ok:
        return False
    if (h.shape[2], h.shape[3]) != _out_hw(x, dconv.stride[0]):
        return False
    return a_bias is None or (a_bias.dtype == torch.float32 and a_bias.numel() == k1 and a_bias.is_contiguous())


def conv1x1_pair_bias_act_x3(conv, dconv, h, x, bias, relu=True, a_bias=None):
    """``act(conv(h) + dconv(x) + bias)`` -- the last 1x1 convolution of a ResNet block and the block's downsampling convolution
    (reference ``network/basenetworks.py:71-150``: torchvision's Bottleneck) -- as ONE product ``[h | x at stride] * [W ; Wd]^T`` of
    the split-operand kernel (``opa_gemm2_bias_act_f32x3``): the identity tensor is neither written nor read back.  With
    ``a_bias``, ``h`` is the raw output of the preceding convolution and ``relu(h + a_bias)`` is applied while it is staged (``x``
    gets zeros: it is non-negative).  ``pair_supported`` says whether this can run."""
    k1, k2, n = conv.in_channels, dconv.in_channels, conv.out_channels
    w3, ab = _pair_weight_of(conv, dconv, a_bias)
    B, _, H, W = x.shape
    out = _empty_nhwc(h, n, dtype=torch.float32)
    _launch('opa_gemm2_bias_act_f32x3', _ptr(h), k1, _ptr(x), k2, B, H, W, dconv.stride[0], _ptr(ab), _ptr(w3), _ptr(bias),
            _ptr(out), n, int(bool(relu)), int(X3_TERMS))
    return out


# (k1, k2, n, stride) of products that ``opa_gemm2_bias_act_bf16`` can run but that came out SLOWER at batch 32 than what runs with the
# switch off (tools/gpu/gemm2_bf16_times.py, profiles/gemm2_bf16/times.log): both predicates decline them.
PAIR_BF16_DECLINED = frozenset()


def pair_bf16_weight_of(conv, dconv, bias):
    """The operands of ``conv1x1_pair_bias_act_bf16`` derived from the CURRENT weights (``conv``: ``[N, k1, 1, 1]``, ``dconv``:
    ``[N, k2, 1, 1]``, 16-bit) and the folded ``bias`` the block keeps (``[N]`` of that dtype or float32, or None): ``Wcat`` =
    ``[W | Wd]`` as ``[N][k1 + k2]``, K-major, and the bias as FLOAT32 (upcast exactly; None stays None).  ``conv`` None: ``dconv``'s
    weight alone, ``[N][k2]`` (``conv1x1_strided_bf16``).  Kept on ``dconv`` by ``derived``, keyed on the three tensors."""
    n, k2 = dconv.out_channels, dconv.in_channels

    def make():
        wd = dconv.weight.detach().reshape(n, k2)
        w = wd.contiguous() if conv is None else torch.cat((conv.weight.detach().reshape(n, conv.in_channels), wd), dim=1).contiguous()
        return w, _bias_f32(bias)
    return derived(dconv, '_opa_w_pair_bf16', (None if conv is None else conv.weight, dconv.weight, bias), make)


def _plain_1x1_bf16(conv, like):
    """``conv``: a 1x1 ``Conv2d`` without groups, padding, dilation or a bias of its own, 16-bit weights of ``like``'s dtype on its
    device that autograd does not follow?  (The stride is the caller's to test, the dtype's route ``ROUTE16_PAIR``'s.)"""
    return (isinstance(conv, torch.nn.Conv2d) and conv.kernel_size == (1, 1) and conv.groups == 1 and conv.padding == (0, 0)
            and conv.dilation == (1, 1) and conv.bias is None and conv.weight.dtype == like.dtype
            and conv.weight.device == like.device and not _autograd_follows(conv.weight))


def pair_bf16_supported(conv, dconv, h, x, bias, a_bias=None):
    """Can ``conv1x1_pair_bias_act_bf16(conv, dconv, h, x, bias, ..., a_bias)`` run?  The switch on (bfloat16: ``PAIR_BF16``, float16:
    ``F16``); ``h`` and ``x`` dense channels-last 16-bit tensors of one dtype on the GPU of one batch, the weights of that dtype, outside
    autocast (whose parameters stay float32), nothing that autograd follows; both
    convolutions 1x1 without groups, padding or a bias of their own, ``conv`` of stride 1, ``dconv`` of square stride 1 or 2, equal
    output channels; ``conv``'s input channels, ``dconv``'s and the output channels multiples of 64; ``h``'s pixels those of ``x`` at
    ``dconv``'s stride; ``x``, ``h`` and the output fewer than 2^31 elements each; 16-byte boundaries; the folded ``bias`` of that dtype
    or float32, one element per output channel, or None; ``a_bias`` (``h``'s owed bias, a ReLU behind it) of that dtype, ``[k1]``,
    contiguous, 16-byte aligned, or None; the library built; ``(k1, k2, n, stride)`` not in ``PAIR_BF16_DECLINED``."""
    dt = x.dtype
    if not (ROUTE16_PAIR.suffix(dt) and not torch.is_autocast_enabled() and _plain_1x1_bf16(dconv, x) and _plain_1x1_bf16(conv, x)
            and not _autograd_follows(h, x, bias, a_bias)):
        return False
    k1, k2, n, s = conv.in_channels, dconv.in_channels, conv.out_channels, dconv.stride[0]
    if not (conv.stride == (1, 1) and dconv.stride == (s, s) and s in (1, 2) and dconv.out_channels == n
            and k1 % 64 == 0 and k2 % 64 == 0 and n % 64 == 0 and _dense_bf16(h, k1, dt) and _dense_bf16(x, k2, dt)
            and h.shape[0] == x.shape[0] and h.device == x.device and tuple(h.shape[2:]) == _out_hw(x, s)
            and 0 < x.numel() < 2 ** 31 and h.numel() < 2 ** 31 and out_pixels(x, s) * n < 2 ** 31 and _folded_bias_ok(bias, n, x)):
        return False
    if a_bias is not None and not (a_bias.dtype == dt and a_bias.device == x.device and a_bias.dim() == 1
                                   and a_bias.numel() == k1 and a_bias.is_contiguous() and a_bias.data_ptr() % 16 == 0):
        return False
    return _lib.available() and (k1, k2, n, s) not in ROUTE16_PAIR.declined_set(dt)


def conv1x1_pair_bias_act_bf16(conv, dconv, h, x, bias, relu=True, a_bias=None):
    """``act(conv(h) + dconv(x) + bias)`` -- the last 1x1 convolution of a 16-bit ResNet block and the block's downsampling
    convolution (reference ``network/basenetworks.py:71-150``: torchvision's Bottleneck) -- as ONE product ``[h | x at stride] *
    [W | Wd]^T`` on the 16-bit MFMA (``opa_gemm2_bias_act_bf16`` / ``..._f16``, csrc/gemm2_bf16.hip): float32 accumulation, one rounding; the identity
    tensor is neither written nor read back.  With ``a_bias``, ``h`` is the raw output of the preceding convolution and
    ``relu(h + a_bias)`` is applied while it is staged (``x`` is taken as it is).  ``pair_bf16_supported`` says whether this can run."""
    k1, k2, n = conv.in_channels, dconv.in_channels, conv.out_channels
    wcat, b32 = pair_bf16_weight_of(conv, dconv, bias)
    B, _, H, W = x.shape
    out = _empty_nhwc(h, n)
    _launch(ROUTE16_PAIR.symbol(x.dtype), _ptr(h), k1, _ptr(x), k2, B, H, W, dconv.stride[0], _ptr(a_bias), _ptr(wcat), _ptr(b32),
            _ptr(out), n, int(bool(relu)))
    return out


def conv1x1_strided_bf16_supported(dconv, x):
    """Can ``conv1x1_strided_bf16(dconv, x)`` run?  ``pair_bf16_supported``'s conditions on ``dconv`` and ``x`` alone: the product
    without a first source (k1 = 0)."""
    if not (ROUTE16_PAIR.suffix(x.dtype) and not torch.is_autocast_enabled() and _plain_1x1_bf16(dconv, x) and not _autograd_follows(x)):
        return False
    k2, n, s = dconv.in_channels, dconv.out_channels, dconv.stride[0]
    return (dconv.stride == (s, s) and s in (1, 2) and k2 % 64 == 0 and n % 64 == 0 and _dense_bf16(x, k2, x.dtype)
            and 0 < x.numel() < 2 ** 31 and out_pixels(x, s) * n < 2 ** 31 and _lib.available()
            and (0, k2, n, s) not in ROUTE16_PAIR.declined_set(x.dtype))


def conv1x1_strided_bf16(dconv, x):
    """``dconv(x)`` for the downsampling 1x1 convolution, stride 1 or 2, of a 16-bit BasicBlock (reference
    ``network/basenetworks.py:71-150``) on the 16-bit MFMA: ``opa_gemm2_bias_act_bf16`` / ``..._f16`` without a first source, a bias or a ReLU.
    ``conv1x1_strided_bf16_supported`` says whether this can run."""
    wd, _ = pair_bf16_weight_of(None, dconv, None)
    B, k2, H, W = x.shape
    s = dconv.stride[0]
    out = _empty_nhwc(x, dconv.out_channels, _out_hw(x, s))
    _launch(ROUTE16_PAIR.symbol(x.dtype), _ptr(None), 0, _ptr(x), k2, B, H, W, s, _ptr(None), _ptr(wd), _ptr(None), _ptr(out),
            dconv.out_channels, 0)
    return out


def _conv3x3_x3_ok(conv, x, bias, d):
    """What both predicates of the float32 implicit GEMM ask, for a 3x3 convolution with square dilation ``d`` and padding ``d`` (the
    kernel's buffer begins d rows + d pixels before the tensor: that share counts towards 2 GB)."""
    return (X3_CONV3 and X3_TERMS in (6, 9) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
            and x.is_contiguous(memory_format=torch.channels_last) and conv.kernel_size == (3, 3)
            and conv.dilation == (d, d) and conv.padding == (d, d)
            and conv.stride[0] == conv.stride[1] and conv.groups == 1 and conv.bias is None
            and conv.in_channels % 64 == 0 and conv.out_channels % 64 == 0 and x.shape[1] == conv.in_channels
            and x.data_ptr() % 16 == 0 and bias.dtype == torch.float32 and bias.is_contiguous() and bias.data_ptr() % 16 == 0
            and (x.shape[0] * x.shape[2] * x.shape[3] + d * (x.shape[3] + 1)) * x.shape[1] * 4 < 2 ** 31)


def _conv3x3_x3(symbol, conv, x, bias, relu, *dilation):
    """``act(conv(x) + bias)`` as an implicit GEMM of the split-operand kernel, float32 in and out, behind both launchers."""
    w3 = _split_weight_3x3_of(conv)
    B, C, H, W = x.shape
    s = conv.stride[0]
    out = _empty_nhwc(x, conv.out_channels, _out_hw(x, s), torch.float32)
    _launch(symbol, _ptr(x), _ptr(w3), _ptr(bias), _ptr(out), B, H, W, C, conv.out_channels, s, *dilation, int(bool(relu)), int(X3_TERMS))
    return out


def conv3x3_x3_supported(conv, x, bias):
    return _conv3x3_x3_ok(conv, x, bias, 1)


def conv3x3_bias_act_x3(conv, x, bias, relu=True):
    """A 3x3 convolution with padding 1 and any stride (reference ``network/basenetworks.py:71-150``: the strided one of a ResNet block)."""
    return _conv3x3_x3('opa_conv3x3_f32x3', conv, x, bias, relu)


def conv3x3_dilated_x3_supported(conv, x, bias):
    """As ``conv3x3_x3_supported``, for any square dilation d >= 1 with padding d."""
    d = conv.dilation[0]
    return (d >= 1 and conv.weight.dtype == torch.float32 and conv.weight.device == x.device and x.numel() > 0
            and _conv3x3_x3_ok(conv, x, bias, d))


def conv3x3_dilated_bias_act_x3(conv, x, bias, relu=True):
    """... with dilation d and padding d (``:121-135``: block 5 under ``--resnet-block5-dilation``): the same kernel, its taps d apart."""
    return _conv3x3_x3('opa_conv3x3_dilated_f32x3', conv, x, bias, relu, conv.dilation[0])


def conv3x3_bf16_weight_of(conv, bias=None):
    """The operands of ``conv3x3_bias_act_bf16`` derived from the CURRENT ``conv.weight`` (``[N, C, 3, 3]`` 16-bit) and the folded
    ``bias`` the block keeps (``[N]`` of that dtype or float32, or None): the weight as ``[N][9][C]`` -- ``weight.permute(0, 2, 3, 1)``, K-major with
    K = 9 C, ``split_weight_3x3``'s layout without the split -- and the bias as FLOAT32 (upcast exactly; None stays None).  Kept on
    ``conv`` by ``derived``, keyed on both tensors: no buffer, no part of a state dict, made again when either was replaced or changed."""
    def make():
        w = conv.weight.detach()
        return w.permute(0, 2, 3, 1).reshape(w.shape[0], 9, w.shape[1]).contiguous(), _bias_f32(bias)
    return derived(conv, '_opa_w_conv3_bf16', (conv.weight, bias), make)


def _conv3x3_16_ok(route, conv, x, bias, residual=None):
    """What ``conv3x3_bf16_supported`` and ``gconv3x3_bf16_supported`` both ask, ``route``'s switch first: all of the former's contract
    but the groups, the residual's layout and the library."""
    dt = x.dtype
    if not (route.suffix(dt) and x.is_cuda and x.dim() == 4 and not torch.is_autocast_enabled()
            and not _autograd_follows(x, bias, residual) and not _autograd_follows(conv.weight)):       # (``conv`` last: maybe no Conv2d)
        return False
    s, d, n = conv.stride[0], conv.dilation[0], conv.out_channels
    return (conv.kernel_size == (3, 3) and conv.bias is None and conv.stride == (s, s) and s in (1, 2)
            and conv.dilation == (d, d) and d in (1, 2, 4) and (d == 1 or s == 1) and conv.padding == (d, d)
            and conv.in_channels % 64 == 0 and n % 64 == 0 and conv.weight.dtype == dt and conv.weight.device == x.device
            and _dense_bf16(x, conv.in_channels, dt) and 0 < x.numel() < 2 ** 31 and out_pixels(x, s) * n < 2 ** 31
            and _folded_bias_ok(bias, n, x))


def conv3x3_bf16_supported(conv, x, bias, residual=None):
    """Can ``conv3x3_bias_act_bf16(conv, x, bias, residual)`` run?  The switch on (bfloat16: ``CONV3_BF16``, float16: ``F16``); a dense
    channels-last 16-bit tensor on the GPU, the weight of its dtype, outside autocast (whose parameters stay float32), nothing that
    autograd follows; a 3x3 convolution without groups or a bias of its own (the folded one arrives separately: of ``x``'s dtype or
    float32, one element per output channel, or None), square stride 1 or 2,
    square dilation 1, 2 or 4 -- above 1 with stride 1 only -- and padding equal to the dilation; input and output channels
    multiples of 64; ``residual`` a dense channels-last tensor of ``x``'s dtype and the output's shape; 16-byte boundaries; ``x`` and the
    output fewer than 2^31 elements each."""
    if not (_conv3x3_16_ok(ROUTE16_CONV3, conv, x, bias, residual) and conv.groups == 1):
        return False
    n = conv.out_channels
    if residual is not None and not (_dense_bf16(residual, n, x.dtype) and residual.device == x.device
                                     and tuple(residual.shape) == (x.shape[0], n) + _out_hw(x, conv.stride[0])):
        return False
    return _lib.available()


def conv3x3_bias_act_bf16(conv, x, bias, residual=None, relu=True):
    """``act(conv(x) + bias (+ residual))`` for a 3x3 convolution of a 16-bit ResNet (reference ``network/basenetworks.py:71-150``:
    torchvision's BasicBlock and Bottleneck; ``:121-135``: block 5 dilated) as ONE implicit GEMM on the 16-bit MFMA
    (``opa_conv3x3_act_bf16`` / ``..._f16``, csrc/conv3x3_bf16.hip): float32 accumulation, one rounding -- ``x``'s dtype in and out.
    ``conv3x3_bf16_supported`` says whether this can run."""
    w9, b32 = conv3x3_bf16_weight_of(conv, bias)
    B, C, H, W = x.shape
    s = conv.stride[0]
    out = _empty_nhwc(x, conv.out_channels, _out_hw(x, s))
    _launch(ROUTE16_CONV3.symbol(x.dtype), _ptr(x), _ptr(w9), _ptr(b32), _ptr(residual), _ptr(out), B, H, W, C, conv.out_channels, s,
            conv.dilation[0], int(bool(relu)))
    return out


GCONV_BF16_WIDTHS = (4, 8, 16, 32, 64)       # channels per group that divide the kernel's 64-channel chunk
# (C, CG, stride) of grouped convolutions that ``opa_gconv3x3_act_bf16`` can run but that came out SLOWER at batch 32 than torch's grouped
# bfloat16 convolution + ``bias_act_`` (tools/gpu/gconv_bf16_times.py, profiles/gconv_bf16/times.log): the predicate declines them.
GCONV_BF16_DECLINED = frozenset()
# ... and of those that ``opa_gconv3x3_act_f16`` can run but that came out slower than torch's grouped FLOAT16 convolution + ``bias_act_``
# (tools/gpu/f16x_times.py, profiles/f16x/times.log)
GCONV_F16_DECLINED = frozenset()


def gconv3x3_bf16_weight_of(conv, bias=None):
    """The operands of ``gconv3x3_bias_act_bf16`` derived from the CURRENT ``conv.weight`` (``[C, CG, 3, 3]`` 16-bit, CG = C / groups)
    and the folded ``bias`` the block keeps (``[C]`` of that dtype or float32, or None): the weight as ``[C][9][64]`` of the weight's
    dtype, K-major with K = 576 and BLOCK DIAGONAL per 64-channel chunk -- column ``j`` of row ``co`` is the weight of input channel
    ``64 * (co // 64) + j``: ``weight[co, j % CG, ky, kx]`` where ``j // CG == (co % 64) // CG``, exactly zero elsewhere -- and the bias as FLOAT32 (upcast
    exactly; None stays None).  Kept on ``conv`` by ``derived`` as ``conv3x3_bf16_weight_of``'s are."""
    def make():
        w = conv.weight.detach()
        c, cg = w.shape[0], w.shape[1]
        packed = w.new_zeros((c, 9, 64 // cg, cg))
        rows = torch.arange(c, device=w.device)
        packed[rows, :, (rows % 64) // cg, :] = w.permute(0, 2, 3, 1).reshape(c, 9, cg)
        return packed.reshape(c, 9, 64), _bias_f32(bias)
    return derived(conv, '_opa_w_gconv_bf16', (conv.weight, bias), make)


def gconv3x3_bf16_supported(conv, x, bias):
    """Can ``gconv3x3_bias_act_bf16(conv, x, bias)`` run?  ``conv3x3_bf16_supported`` with these differences: the switch is
    ``GCONV_BF16`` (float16: ``GCONV_F16``, not ``F16``); the convolution HAS groups; as many output as input channels C, C a multiple
    of 64, and a group width C / groups of ``GCONV_BF16_WIDTHS``; no residual; ``(C, C // groups, stride)`` not in
    ``GCONV_BF16_DECLINED`` (float16: ``GCONV_F16_DECLINED``)."""
    if not (_conv3x3_16_ok(ROUTE16_GCONV, conv, x, bias) and conv.groups > 1):
        return False
    c, cg = conv.in_channels, conv.in_channels // conv.groups
    return (c == conv.out_channels and c % conv.groups == 0 and cg in GCONV_BF16_WIDTHS and _lib.available()
            and (c, cg, conv.stride[0]) not in ROUTE16_GCONV.declined_set(x.dtype))


def gconv3x3_bias_act_bf16(conv, x, bias, relu=True):
    """``act(conv(x) + bias)`` for the grouped 3x3 convolution of a 16-bit ResNeXt (reference ``network/basenetworks.py:71-150`` with
    torchvision's grouped Bottleneck; ``:121-135``: block 5 dilated) as ONE implicit GEMM per 64-channel chunk on the 16-bit MFMA
    (``opa_gconv3x3_act_bf16`` / ``..._f16``, csrc/gconv3x3_bf16.hip): float32 accumulation, one rounding -- ``x``'s dtype in and out.
    ``gconv3x3_bf16_supported`` says whether this can run."""
    w9, b32 = gconv3x3_bf16_weight_of(conv, bias)
    B, C, H, W = x.shape
    s = conv.stride[0]
    out = _empty_nhwc(x, C, _out_hw(x, s))
    _launch(ROUTE16_GCONV.symbol(x.dtype), _ptr(x), _ptr(w9), _ptr(b32), _ptr(out), B, H, W, C, C // conv.groups, s, conv.dilation[0],
            int(bool(relu)))
    return out


def stem_x3_supported(conv, x, bias):
    return (X3_STEM and X3_TERMS in (6, 9) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and conv.kernel_size == (7, 7)
            and conv.stride == (2, 2) and conv.padding == (3, 3) and conv.dilation == (1, 1) and conv.groups == 1 and conv.bias is None
            and conv.in_channels == 3 and x.shape[1] == 3 and conv.out_channels % 64 == 0
            and bias.dtype == torch.float32 and bias.is_contiguous() and bias.data_ptr() % 16 == 0
            and x.shape[0] * (x.shape[2] + 7) * (x.shape[3] + 7) * 16 < 2 ** 31)


def stem7x7_bias_act_x3(conv, x, bias, relu=True):
    """``act(conv(x) + bias)`` for the 7x7 stride-2 padding-3 stem of a ResNet on RGB input (reference ``network/basenetworks.py:71-150``)
    as an implicit GEMM of the split-operand kernel: the image is copied once into a zero-padded 4-channel NHWC tensor (3 pixels
    before, 4 behind; ~1 % of the step), a window ROW -- 8 pixels x 4 channels = 32 contiguous floats -- is one K-step, the
    eighth row and column and the fourth channel meet zero weights.  K = 8 x 32 = 256."""
    w3 = _stem_weight_of(conv)
    B, _, H, W = x.shape
    xp = torch.nn.functional.pad(x.permute(0, 2, 3, 1), (0, 1, 3, 4, 3, 4)).contiguous()        # [B, H + 7, W + 7, 4]
    ho, wo = _out_hw(x, 2)
    out = _empty_nhwc(x, conv.out_channels, (ho, wo), torch.float32)
    _launch('opa_conv_rows_f32x3', _ptr(xp), _ptr(w3), _ptr(bias), _ptr(out), B, H + 7, W + 7, 4, ho, wo, 2, 8, 32,
            conv.out_channels, int(bool(relu)), int(X3_TERMS))
    return out


STEM7_BF16_K = 192                        # kStem7Bf16K: 8 window rows (the eighth zeros) of 8 pixels (the eighth zeros) of 3 channels
# (c_out, stride, pooled) of FLOAT16 stems that ``opa_stem7x7_act_f16`` can run but that came out SLOWER at batch 32 than torch's float16
# convolution + ``bias_act_`` (pooled: + ``F.max_pool2d`` behind either) (tools/gpu/f16x_times.py, profiles/f16x/times.log):
# ``stem7x7_bf16_supported(..., pooled=...)`` declines them.  (The bfloat16 stem has no such set: its predicate answers as it did.)
STEM7_F16_DECLINED = frozenset()


def stem7x7_bf16_weight_of(conv, bias=None):
    """The operands of ``stem7x7_bias_act_bf16`` derived from the CURRENT ``conv.weight`` (``[N, 3, 7, 7]`` 16-bit) and the folded
    ``bias`` the network keeps (``[N]`` of that dtype or float32, or None): the weight as ``[N][192]`` of the weight's dtype, K-major in
    the load plan's order
    (csrc/stem7x7_bf16_plan.hpp) -- ``w[co][ky * 24 + kx * 3 + ci] = weight[co][ci][ky][kx]``, ZEROS in the columns ``kx = 7`` and
    ``ky = 7`` that pad 147 to 192 -- and the bias as FLOAT32 (upcast exactly; None stays None).  Kept on ``conv`` by ``derived`` as
    ``conv3x3_bf16_weight_of``'s are."""
    def make():
        w = conv.weight.detach()
        wk = w.new_zeros((w.shape[0], 8, 8, 3))
        wk[:, :7, :7] = w.permute(0, 2, 3, 1)
        return wk.reshape(w.shape[0], STEM7_BF16_K), _bias_f32(bias)
    return derived(conv, '_opa_w_stem7_bf16', (conv.weight, bias), make)


def stem7x7_bf16_supported(conv, x, bias, pooled=False):
    """Can ``stem7x7_bias_act_bf16(conv, x, bias)`` run?  The switch on (bfloat16: ``STEM7_BF16``, float16: ``STEM7_F16``, not
    ``F16``); ``x`` a 16-bit ``[B, 3, H, W]`` tensor on the GPU in ANY
    layout with positive strides (channels-last, NCHW, a cropped view), outside autocast (whose parameters stay float32), nothing
    that autograd follows; a 7x7 convolution with padding 3, no dilation, no groups and no bias of its own (the folded one arrives
    separately: of ``x``'s dtype or float32, one element per output channel, or None), square stride 1 or 2, output channels a multiple of
    64, weights of ``x``'s dtype on ``x``'s device; ``x`` fewer than 2^31 elements from the first to the last addressed, the output fewer
    than 2^31 elements; for float16, ``(c_out, stride, pooled)`` not in ``STEM7_F16_DECLINED`` (``pooled``: the caller puts the input
    max-pool behind the stem)."""
    dt = x.dtype
    if not (ROUTE16_STEM7.suffix(dt) and x.is_cuda and x.dim() == 4 and x.shape[1] == 3 and not torch.is_autocast_enabled()
            and not _autograd_follows(x, bias) and not _autograd_follows(conv.weight)):                 # (``conv`` last: maybe no Conv2d)
        return False
    s = conv.stride[0]
    if not (isinstance(conv, torch.nn.Conv2d) and conv.kernel_size == (7, 7) and conv.padding == (3, 3) and conv.dilation == (1, 1)
            and conv.groups == 1 and conv.bias is None and conv.padding_mode == 'zeros' and conv.stride == (s, s) and s in (1, 2)
            and conv.in_channels == 3 and conv.out_channels % 64 == 0
            and conv.weight.dtype == dt and conv.weight.device == x.device and _folded_bias_ok(bias, conv.out_channels, x)
            and (conv.out_channels, s, bool(pooled)) not in ROUTE16_STEM7.declined_set(dt)):
        return False
    last = sum((n - 1) * st for n, st in zip(x.shape, x.stride()))               # the last element addressed
    return (min(x.shape) > 0 and min(x.stride()) > 0 and x.data_ptr() % 2 == 0 and last < 2 ** 31
            and out_pixels(x, s) * conv.out_channels < 2 ** 31 and _lib.available())


def stem7x7_bias_act_bf16(conv, x, bias, relu=True):
    """``act(conv(x) + bias)`` for the 7x7 padding-3 stem of a 16-bit ResNet on RGB input (reference ``network/basenetworks.py:71-150``),
    stride 1 or 2, as ONE implicit GEMM on the 16-bit MFMA (``opa_stem7x7_act_bf16`` / ``..._f16``, csrc/stem7x7_bf16.hip): ``x`` is read
    through its own four strides, whatever its layout -- no padded copy, no 4-channel copy --, float32 accumulation, one rounding; the
    result is a dense channels-last tensor of ``x``'s dtype.  ``stem7x7_bf16_supported`` says whether this can run."""
    wk, b32 = stem7x7_bf16_weight_of(conv, bias)
    B, _, H, W = x.shape
    s = conv.stride[0]
    out = _empty_nhwc(x, conv.out_channels, _out_hw(x, s))
    _launch(ROUTE16_STEM7.symbol(x.dtype), _ptr(x), x.stride(0), x.stride(1), x.stride(2), x.stride(3), _ptr(wk), _ptr(b32), _ptr(out),
            B, H, W, conv.out_channels, s, int(bool(relu)))
    return out


def head_conv_x3_supported(conv, x):
    return (X3_HEAD and X3_TERMS in (6, 9) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and not x.requires_grad
            and x.is_contiguous(memory_format=torch.channels_last) and conv.kernel_size == (1, 1) and conv.stride == (1, 1)
            and conv.padding == (0, 0) and conv.groups == 1 and conv.in_channels % 64 == 0 and x.shape[1] == conv.in_channels
            and conv.weight.dtype == torch.float32 and x.data_ptr() % 16 == 0)


def head_conv_x3(conv, x):
    """``conv(x)`` for a head's biased 1x1 convolution (reference ``network/heads.py:272-378``: ``CompositeField4.conv``) through the
    split-operand GEMM: the output channels are padded to the next multiple of 64 with zero weights (``_unit_weight_of``: the input
    channels are a multiple of 64 here and get no padding), the product is written with that pitch and the real channels are
    copied out (0.2 GB for both COCO heads at batch 32)."""
    n = conv.out_channels
    w3, bp = _unit_weight_of(conv)
    out = conv1x1_bias_act_x3(x, w3, bp, None, False, None, X3_TERMS)
    return out[:, :n].contiguous(memory_format=torch.channels_last) if w3.shape[1] != n else out


class UnitMode(typing.NamedTuple):
    """The unit mode for one element type: what the predicates, the derived operands and the launcher of the route read."""
    dtype: torch.dtype                  # of the weight, the bias and the activations
    align: int                          # bytes: the boundary ``x``, the partner and the residual lie on
    enabled: typing.Callable            # () -> the route's switch as it reads NOW
    declines_autocast: bool             # does ``unit_conv_supported`` itself decline under autocast (whose parameters stay float32)?
    weight: typing.Callable             # the padded ``[N_pad, K_pad]`` weight -> the kernel's weight operand
    cache: str                          # the attribute ``_unit_operands_of`` keeps the operands under
    launch: typing.Callable             # (operands, act code, act_param, terms) -> the launch
    gemm: str                           # the name ``conv1x1_unit`` calls the mode's GEMM by
    table: bool                         # is a competing torch path chosen through the choice table (``pick_unit``)?
    head: typing.Callable               # () -> may a head's convolution take the mode NOW?


def _launch_unit_x3(operands, code, act_param, terms):
    """``ACT_LEAKY_RELU`` / ``ACT_RELU6`` to ``opa_gemm_unit_actp_f32x3``, every other code to the symbol it has always gone to: one kernel."""
    terms = int(X3_TERMS if terms is None else terms)
    if code in (ACT_LEAKY_RELU, ACT_RELU6):
        _launch('opa_gemm_unit_actp_f32x3', *operands, code, float(act_param), terms)
    else:
        _launch('opa_gemm_unit_act_f32x3', *operands, code, terms)


# float32 through the split-operand GEMM (csrc/gemm_f32x3.hip); bfloat16 on the bf16 MFMA (csrc/gemm_unit_bf16.hip): one symbol, no terms
UNIT_MODE_X3 = UnitMode(torch.float32, 8, lambda: X3_UNIT and X3_TERMS in (6, 9), False, split_weight, '_opa_w3_unit', _launch_unit_x3,
                        'conv1x1_unit_x3', True, lambda: X3_HEAD)
UNIT_MODE_BF16 = UnitMode(torch.bfloat16, 4, lambda: UNIT_BF16, True, lambda wp: wp, '_opa_w_unit_bf16',
                          lambda operands, code, act_param, terms: _launch('opa_gemm_unit_actp_bf16', *operands, code, float(act_param)),
                          'conv1x1_unit_bf16', False, lambda: True)
# float16: the same kernel on the f16 MFMA behind its own switch and symbol, its operands under its own attribute
UNIT_MODE_F16 = UnitMode(torch.float16, 4, lambda: UNIT_F16, True, lambda wp: wp, '_opa_w_unit_f16',
                         lambda operands, code, act_param, terms: _launch('opa_gemm_unit_actp_f16', *operands, code, float(act_param)),
                         'conv1x1_unit_f16', False, lambda: True)
_UNIT_MODES = {mode.dtype: mode for mode in (UNIT_MODE_X3, UNIT_MODE_BF16, UNIT_MODE_F16)}


def unit_mode_of(t):
    """The unit mode for tensors of ``t``'s dtype, or None where there is none."""
    return _UNIT_MODES.get(t.dtype)


def _unit_conv_ok(mode, conv):
    """The part of ``unit_conv_supported`` that depends on the convolution alone."""
    return (mode.enabled() and conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.padding == (0, 0)
            and conv.dilation == (1, 1) and conv.groups == 1 and conv.in_channels % 2 == 0 and conv.out_channels % 2 == 0
            and conv.weight.dtype == mode.dtype and (conv.bias is None or conv.bias.dtype == mode.dtype))


def _unit_operand_ok(mode, t, channels):
    """Layout of an activation operand of the unit mode (``x``, the partner or the residual), whatever its device: ``mode``'s dtype,
    ``channels`` channels innermost with an even pitch between pixels, on ``mode``'s boundary, not followed by autograd."""
    ps = _pixel_stride(t)
    return (t.dtype == mode.dtype and not t.requires_grad and ps is not None and t.shape[1] == channels
            and ps % 2 == 0 and ps <= 2 ** 21 and t.data_ptr() % mode.align == 0)


def unit_conv_supported(conv, x, partner=None, residual=None, mode=None, head=False):
    """Can ``conv1x1_unit(conv, x, partner=partner, residual=residual)`` run?  The mode of ``x``'s dtype (``mode`` where given) switched
    on, weight and activation of that dtype on the same GPU -- bfloat16 and float16: outside autocast, whose parameters stay float32 -- a 1x1
    convolution of stride 1 without padding or groups and with EVEN channel counts, ``x`` (and ``partner`` or ``residual``, never both:
    the output's pixels, ``conv.out_channels`` channels) channels-innermost tensors or channel slices of such, on 8-byte boundaries
    (bfloat16 and float16: 4), nothing that autograd follows.  ``head``: ``conv`` is a head's, which float32 takes behind ``X3_HEAD`` only."""
    mode = mode or unit_mode_of(x)
    if not (mode is not None and x.is_cuda and conv.weight.device == x.device and (not head or mode.head())
            and not (mode.declines_autocast and torch.is_autocast_enabled()) and _unit_conv_ok(mode, conv)
            and _unit_operand_ok(mode, x, conv.in_channels) and 0 < x.shape[0] * x.shape[2] * x.shape[3] < 2 ** 31):
        return False
    if partner is not None and residual is not None:
        return False
    for third in (partner, residual):
        if third is not None and not (third.device == x.device and _unit_operand_ok(mode, third, conv.out_channels)
                                      and (third.shape[0], third.shape[2], third.shape[3]) == (x.shape[0], x.shape[2], x.shape[3])):
            return False
    return True


def _conv1x1_unit(mode, conv, x, relu=True, partner=None, residual=None, act=None, terms=None, act_param=0.0):
    """``act(conv(x))`` for a biased 1x1 convolution of ANY even channel counts on a channels-last tensor or channel slice
    (reference ``network/basenetworks.py:186-242``: the 1x1 convolutions of a ShuffleNetV2K unit, folded with their batch norms),
    through the unit mode ``mode``: float32 the split-operand GEMM's (``opa_gemm_unit_act_f32x3``),
    bfloat16 / float16 one 16-bit MFMA per product, float32 accumulation and one rounding (``opa_gemm_unit_actp_bf16`` / ``..._f16``).  With ``partner``
    (``[B, N, H, W]``, may be a slice) the result is ``channel_shuffle(cat((partner, y), 1), 2)`` -- ``[B, 2N, H, W]``, the partner's
    channels copied into the even positions by the same kernel.  channels_last ``x.dtype`` out.  ``unit_conv_supported``: can it run?

    ``act`` (``ACT_NONE`` / ``ACT_RELU`` / ``ACT_HARDSWISH``) instead of ``relu``, and ``residual`` (``[B, N, H, W]``, may be a slice,
    never together with a partner): ``act(conv(x) + residual)`` in the same launch -- the 1x1 convolutions of a MobileNetV3 block.
    ``act`` ``ACT_LEAKY_RELU`` / ``ACT_RELU6`` with ``act_param`` (the slope / the cap; never with a residual): a LeakyReLU unit, the
    expanding and the last convolution of MobileNetV2.  ``terms`` (float32 alone): 6 or 9 instead of ``X3_TERMS`` (the squeeze of a
    SqueezeNet Fire: ``FIRE_TERMS``).  ``mode.launch`` says which symbol takes which code."""
    w, bp = _unit_operands_of(mode, conv)
    n = conv.out_channels
    out = _empty_nhwc(x, n if partner is None else 2 * n, dtype=mode.dtype)
    operands = (_ptr(x), _pixel_stride(x), _ptr(w), _ptr(bp),
                _ptr(partner), _pixel_stride(partner) if partner is not None else 0,
                _ptr(residual), _pixel_stride(residual) if residual is not None else 0,
                _ptr(out), out_pixels(x), n, x.shape[1])
    mode.launch(operands, _act_code(relu, act), act_param, terms)
    return out


def conv1x1_unit(conv, x, **kwargs):
    """``_conv1x1_unit`` in the mode of ``x``'s dtype, called by the mode's public name as it reads NOW: a recorder that a test or a
    tool puts on ``conv1x1_unit_x3`` / ``conv1x1_unit_bf16`` / ``conv1x1_unit_f16`` sees every launch of the routes."""
    return globals()[unit_mode_of(x).gemm](conv, x, **kwargs)


def pick_unit(x, m, k, n, has_partner, run_unit, run_other):
    """``run_unit``, a route through the unit mode of ``x``'s dtype that the caller found supported, or ``run_other``, what the trunk did
    before.  float32: ``pick``'s decision, key ``'unit'``, never timed.  bfloat16 and float16: no table entry -- the supported route runs."""
    if unit_mode_of(x).table:
        return pick('unit', m, k, n, has_partner, False, run_unit, run_other, timing=False)
    return run_unit()


# The per-dtype names (tests, tools/gpu and the documents use them; launch recorders wrap the two GEMMs): the functions above, one mode bound
_unit_weight_of = functools.partial(_unit_operands_of, UNIT_MODE_X3)
_unit_weight_bf16_of = functools.partial(_unit_operands_of, UNIT_MODE_BF16)
unit_conv_x3_supported = functools.partial(unit_conv_supported, mode=UNIT_MODE_X3)
unit_conv_bf16_supported = functools.partial(unit_conv_supported, mode=UNIT_MODE_BF16)
conv1x1_unit_x3 = functools.partial(_conv1x1_unit, UNIT_MODE_X3)


def conv1x1_unit_bf16(conv, x, relu=True, partner=None, residual=None, act=None, act_param=0.0):          # (its signature: no ``terms``)
    return _conv1x1_unit(UNIT_MODE_BF16, conv, x, relu, partner, residual, act, None, act_param)


_unit_weight_f16_of = functools.partial(_unit_operands_of, UNIT_MODE_F16)
unit_conv_f16_supported = functools.partial(unit_conv_supported, mode=UNIT_MODE_F16)


def conv1x1_unit_f16(conv, x, relu=True, partner=None, residual=None, act=None, act_param=0.0):           # (float16: ``opa_gemm_unit_actp_f16``)
    return _conv1x1_unit(UNIT_MODE_F16, conv, x, relu, partner, residual, act, None, act_param)


# ---- the Fire expand ------------------------------------------------------------------------------------------------------------------

def _fragment_order(w3):
    """``[3, N, K]`` (``split_weight``; N a multiple of 32, K of 16) -> ``[3, N * K]`` in the order ``csrc/fire.hip`` loads it: per
    32-row block and K-step of 16 one fragment of 64 lanes x 8 elements, lane ``l`` holding row ``l % 32``, columns
    ``8 * (l // 32) ... + 8`` -- the B operand of ``v_mfma_f32_32x32x16_bf16`` as consecutive bytes."""
    n, k = w3.shape[1], w3.shape[2]
    return w3.reshape(3, n // 32, 32, k // 16, 2, 8).permute(0, 1, 3, 4, 2, 5).reshape(3, n * k)


def fire_weight_of(expand1x1, expand3x3):
    """The operands of ``fire_expand_bias_relu`` derived from the CURRENT parameters of both convolutions: the split weights in the
    kernel's fragment order, ``[3, (e1 + 9 e3) * s]`` bfloat16 (the 1x1's blocks, then the 3x3's with K = (ky, kx, c)), and both
    biases concatenated (zeros where a convolution has none).  Kept on ``expand1x1`` (``derived``): the key holds both weights and
    both biases, so ``load_state_dict``, ``.to()`` or an in-place update of any of them makes a new operand."""
    def make():
        w1, w3 = expand1x1.weight.detach(), expand3x3.weight.detach()
        blocks = (_fragment_order(split_weight(w1.reshape(w1.shape[0], w1.shape[1]))), _fragment_order(split_weight_3x3(w3)))
        biases = [torch.zeros(c.out_channels, dtype=torch.float32, device=w1.device) if c.bias is None else c.bias.detach().float()
                  for c in (expand1x1, expand3x3)]
        return torch.cat(blocks, dim=1).contiguous(), torch.cat(biases).contiguous()
    return derived(expand1x1, '_opa_w3_fire', (expand1x1.weight, expand1x1.bias, expand3x3.weight, expand3x3.bias), make)


def _fire_convs_ok(expand1x1, expand3x3):
    """The part of ``fire_expand_supported`` that depends on the two convolutions alone."""
    def ok(conv, k):
        return (conv.kernel_size == (k, k) and conv.stride == (1, 1) and conv.padding == (k // 2, k // 2) and conv.dilation == (1, 1)
                and conv.groups == 1 and conv.padding_mode == 'zeros' and conv.weight.dtype == torch.float32
                and (conv.bias is None or (conv.bias.dtype == torch.float32 and conv.bias.device == conv.weight.device)))
    s = expand1x1.in_channels
    return (ok(expand1x1, 1) and ok(expand3x3, 3) and expand3x3.in_channels == s and s % 16 == 0 and s <= 64
            and expand1x1.out_channels % 64 == 0 and expand3x3.out_channels % 64 == 0
            and expand1x1.weight.device == expand3x3.weight.device)


def fire_expand_supported(expand1x1, expand3x3, h, terms=None):
    """Can ``fire_expand_bias_relu(expand1x1, expand3x3, h, terms)`` run?  ``terms`` (``FIRE_TERMS`` where not given) 6 or 9;  A 1x1 and a 3x3 (padding 1) float32 convolution of stride 1 on the
    same 16 / 32 / 48 / 64 input channels with multiples of 64 output channels each; ``h`` a dense channels-last float32 tensor on
    their device, input and output smaller than 2 GB, outside autocast, not followed by autograd."""
    if not (h.is_cuda and h.dim() == 4 and h.dtype == torch.float32 and not torch.is_autocast_enabled() and _fire_convs_ok(expand1x1, expand3x3)):
        return False
    if _autograd_follows(h, *expand1x1.parameters(), *expand3x3.parameters()):
        return False
    return (h.shape[1] == expand1x1.in_channels and h.is_contiguous(memory_format=torch.channels_last) and h.data_ptr() % 16 == 0
            and fire_expand_shape_supported(expand1x1, expand3x3, h.device, h.shape[0] * h.shape[2] * h.shape[3], terms))


def fire_expand_shape_supported(expand1x1, expand3x3, device, pixels, terms=None):
    """The part of ``fire_expand_supported`` that needs no tensor: the convolutions, their device and the size of a dense channels-last
    float32 operand of ``pixels`` pixels (batch x rows x columns) that the caller is about to allocate (``network._Fire``)."""
    n = expand1x1.out_channels + expand3x3.out_channels
    return ((FIRE_TERMS if terms is None else terms) in (6, 9)          # (the value the launcher passes)
            and _fire_convs_ok(expand1x1, expand3x3) and expand1x1.weight.device == device and 0 < pixels
            and pixels * n * 4 < 2 ** 31 and _lib.available())


def fire_expand_bias_relu(expand1x1, expand3x3, h, terms=None):
    """``cat((relu(expand1x1(h)), relu(expand3x3(h))), 1)`` -- the second half of a SqueezeNet Fire module (reference
    ``network/basenetworks.py:461-487``: torchvision's ``Fire``) -- in one HIP kernel (``opa_fire_expand_f32x3``, ``csrc/fire.hip``):
    split-operand arithmetic with ``terms`` (6 or 9; ``FIRE_TERMS`` where not given) terms, float32 channels-last in and out.
    ``fire_expand_supported`` says whether this can run."""
    w3, bias = fire_weight_of(expand1x1, expand3x3)
    B, S, H, W = h.shape
    out = _empty_nhwc(h, expand1x1.out_channels + expand3x3.out_channels, dtype=torch.float32)
    _launch('opa_fire_expand_f32x3', _ptr(h), _ptr(w3), _ptr(bias), _ptr(out), B, H, W, S, expand1x1.out_channels,
            expand3x3.out_channels, int(FIRE_TERMS if terms is None else terms))
    return out


# ---- the max-pools, the grouped and the depthwise stencils ---------------------------------------------------------------------------------------------

GCONV_WIDTHS = (4, 8, 16, 32, 64)            # channels per group the kernel is instantiated for


def gconv3x3_supported(conv, x, bias):
    """Can ``gconv3x3_bias_act(conv, x, bias)`` run?  A grouped 3x3 convolution (padding 1, dilation 1, square stride 1 or 2, as many
    output as input channels, a group width of ``GCONV_WIDTHS``, no bias of its own: the folded one arrives separately) of a dense
    channels-last float32 tensor on the GPU, outside autocast, not followed by autograd."""
    if not (GCONV and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and not torch.is_autocast_enabled()
            and not _autograd_follows(x, bias) and not _autograd_follows(conv.weight)):             # (``conv`` last: maybe no Conv2d)
        return False
    c = conv.in_channels
    return (conv.groups > 1 and conv.kernel_size == (3, 3) and conv.padding == (1, 1) and conv.dilation == (1, 1)
            and conv.stride in ((1, 1), (2, 2)) and c == conv.out_channels and c % conv.groups == 0
            and c // conv.groups in GCONV_WIDTHS and conv.bias is None and conv.weight.dtype == torch.float32
            and conv.weight.device == x.device and x.shape[1] == c and x.is_contiguous(memory_format=torch.channels_last)
            and x.data_ptr() % 16 == 0 and 0 < x.shape[0] <= 65535                     # (grid.y of the kernel)
            and (bias is None or (bias.dtype == torch.float32 and bias.device == x.device and bias.is_contiguous()
                                  and bias.numel() == c and bias.data_ptr() % 16 == 0))
            and _lib.available())


def gconv3x3_bias_act(conv, x, bias, relu=True):
    """``act(conv(x) + bias)`` for a grouped 3x3 convolution (reference ``network/basenetworks.py:71-150`` with torchvision's grouped
    Bottleneck: ResNeXt) in one HIP kernel, float32 in and out.  ``gconv3x3_supported`` says whether this can run."""
    wt = gconv_weight_of(conv)
    B, C, H, W = x.shape
    s = conv.stride[0]
    out = _empty_nhwc(x, C, _out_hw(x, s), torch.float32)
    _launch('opa_gconv3x3_bias_act_f32', _ptr(x), C, _ptr(wt), _ptr(bias), _ptr(out), C, B, H, W, C, C // conv.groups, s,
            int(bool(relu)))
    return out


def maxpool3x3_supported(x, bias=None):
    """Can ``maxpool3x3_bias_act_(x, bias)`` run?  A dense channels-last float32 or bfloat16 tensor on the GPU with a multiple of 8
    channels, smaller than 2 GB, not followed by autograd; ``bias`` of ``x``'s dtype, one element per channel."""
    return (x.is_cuda and x.dim() == 4 and x.dtype in (torch.float32, torch.bfloat16) and not _autograd_follows(x)
            and x.is_contiguous(memory_format=torch.channels_last) and x.shape[1] % 8 == 0 and x.data_ptr() % 16 == 0
            and 0 < x.numel() * x.element_size() < 2 ** 31
            and (bias is None or (bias.dtype == x.dtype and bias.device == x.device and bias.is_contiguous()
                                  and bias.numel() == x.shape[1] and bias.data_ptr() % 16 == 0))
            and _lib.available())


def maxpool3x3_out_hw(h, w, ceil_mode=False):
    """Output rows and columns of ``max_pool2d(kernel 3, stride 2, padding 1, ceil_mode)`` for an ``h`` x ``w`` input: floor mode
    ``(h - 1) // 2 + 1``; ceil mode torch's ``ceil((h - 1) / 2) + 1``, one less if the last window would begin behind the input and its
    left padding (``(o - 1) * 2 >= h + 1``) -- the floor-mode size for odd ``h``, one more for even ``h``."""
    def one(n):
        if not ceil_mode:
            return (n - 1) // 2 + 1
        o = -((n - 1) // -2) + 1
        return o - 1 if (o - 1) * 2 >= n + 1 else o
    return one(h), one(w)


def maxpool3x3_bias_act_(x, bias=None, relu=False, out=None, ceil_mode=False):
    """``max_pool2d(act(x + bias), 3, 2, 1)`` -- the input max-pool of a ResNet (reference ``network/basenetworks.py:85-93``) with the
    stem's bias and ReLU in front of it -- in one HIP kernel (``opa_maxpool3x3_bias_act``): ``torch.equal`` to what the torch ops compute.
    ``bias`` None: no addition.  ``x`` is read only; ``out``: a dense channels-last tensor to write into (tests).
    ``ceil_mode``: torch's ``ceil_mode=True`` output sizes (``maxpool3x3_out_hw``) -- SqueezeNet's pools (reference
    ``network/basenetworks.py:461-487``) -- through ``opa_maxpool3x3_ceil_bias_act``, the same kernel.
    ``maxpool3x3_supported`` says whether this can run."""
    B, C, H, W = x.shape
    if out is None:
        out = _empty_nhwc(x, C, maxpool3x3_out_hw(H, W, ceil_mode))
    _launch('opa_maxpool3x3_ceil_bias_act' if ceil_mode else 'opa_maxpool3x3_bias_act', _ptr(x), _ptr(bias), _ptr(out),
            _DTYPES[x.dtype], B, H, W, C, 2, int(bool(relu)))
    return out


# (kernel_size, dilation) combinations the stencil can run but that came out SLOWER than torch's convolution of the same layer
# (tools/gpu/shufflenetv2k_option_times.py, profiles/shufflenetv2k_options/times.log): ``dwconv_supported`` declines them.
DW_DECLINED = frozenset()


def dwconv_out_hw(h, w, kernel_size, stride, dilation=1):
    """Output rows and columns of the depthwise convolution with padding ``(kernel_size // 2) * dilation``."""
    cut = dilation * (kernel_size - 1) - 2 * (kernel_size // 2) * dilation + 1          # (1 for an odd kernel)
    return (h - cut) // stride + 1, (w - cut) // stride + 1


def dwconv_supported(x, kernel_size, stride, dilation=1):
    """Can ``dwconv_bias_act(x, ..., kernel_size, stride, dilation=dilation)`` run?  A float32 or bfloat16 channels-innermost tensor
    or channel slice on the GPU -- or a float16 one where ``UNIT_F16`` is on, outside autocast and not followed by autograd; a 3 x 3,
    5 x 5 or 7 x 7 window; stride 1 or 2; dilation 1, or 2 or 4 at stride 1."""
    if not (x.is_cuda and x.dim() == 4):
        return False
    if not (kernel_size in (3, 5, 7) and stride in (1, 2) and (dilation == 1 or (dilation in (2, 4) and stride == 1))):
        return False
    if DW_DECLINED and (kernel_size, dilation) in DW_DECLINED:
        return False
    rows_out = dwconv_out_hw(x.shape[2], x.shape[3], kernel_size, stride, dilation)[0]
    if x.dtype == torch.float16:
        if not (UNIT_F16 and not torch.is_autocast_enabled() and not x.requires_grad):
            return False
    elif x.dtype not in (torch.float32, torch.bfloat16):
        return False
    return (x.shape[0] * rows_out <= 65535                              # grid.y of the stencil kernel (dwconv.hip)
            and _pixel_stride(x) is not None and _lib.available())


def dwconv_bias_act(x, w_taps, bias, kernel_size, stride, relu=False, act=None, dilation=1, act_param=0.0):
    """Depthwise ``kernel_size`` x ``kernel_size`` convolution (padding k//2 times the dilation) + bias (+ activation) of a
    channels-last activation or channel slice, one HIP stencil kernel.  ``w_taps``: ``[k*k, C]`` (tap-major,
    ``depthwise_taps``) in ``x``'s dtype.  ``act`` (``ACT_NONE`` / ``ACT_RELU`` / ``ACT_HARDSWISH``) instead of ``relu``.
    A 3 x 3 or 5 x 5 window without dilation goes to ``opa_dwconv_act``, a 7 x 7 window or a dilation of 2 or 4 (stride 1) to
    ``opa_dwconv_dilated_act``: the same kernel template; ``act`` ``ACT_RELU6`` with ``act_param`` (the cap) -- the depthwise
    convolution of a MobileNetV2 block -- to ``opa_dwconv_actp``, whatever the window.  A float16 ``x`` (``w_taps`` and ``bias`` float16
    too) goes to ``opa_dwconv_actp_f16``, whatever the window and the code."""
    B, C, H, W = x.shape
    out = _empty_nhwc(x, C, dwconv_out_hw(H, W, kernel_size, stride, dilation))
    if x.dtype == torch.float16:
        _launch('opa_dwconv_actp_f16', _ptr(x), _pixel_stride(x), _ptr(w_taps), _ptr(bias), _ptr(out), C, B, H, W, C, kernel_size,
                stride, dilation, _act_code(relu, act), float(act_param))
    elif _act_code(relu, act) == ACT_RELU6:
        _launch('opa_dwconv_actp', _ptr(x), _pixel_stride(x), _ptr(w_taps), _ptr(bias), _ptr(out), C, B, H, W, C, kernel_size,
                stride, dilation, _DTYPES[x.dtype], ACT_RELU6, float(act_param))
    elif kernel_size in (3, 5) and dilation == 1:
        _launch('opa_dwconv_act', _ptr(x), _pixel_stride(x), _ptr(w_taps), _ptr(bias), _ptr(out), C, B, H, W, C, kernel_size, stride,
                _DTYPES[x.dtype], _act_code(relu, act))
    else:
        _launch('opa_dwconv_dilated_act', _ptr(x), _pixel_stride(x), _ptr(w_taps), _ptr(bias), _ptr(out), C, B, H, W, C, kernel_size,
                stride, dilation, _DTYPES[x.dtype], _act_code(relu, act))
    return out


# ---- the RGB stem -----------------------------------------------------------------------------------------------------------------------

STEM_CHANNELS = (16, 24, 32, 42, 64)         # output channels the kernel is instantiated for: the stems the networks have
# output channel counts the kernel can run but that came out NO FASTER than torch's convolution + activation of the same layer
# (tools/gpu/stem_times.py, profiles/stem/times.log): ``stem_conv3x3_supported`` declines them.
STEM_DECLINED = frozenset()


def stem_weight_of(conv):
    """The weight operand of ``stem_conv3x3_bias_act`` derived from the CURRENT ``conv.weight`` (``[C, 3, 3, 3]``): ``[27, C]`` float32,
    tap-major with the output channel innermost, ``w[(ky * 3 + kx) * 3 + ci][co] = weight[co][ci][ky][kx]``.  Derived and cached
    (``derived``): no buffer, no part of a state dict, computed again whenever the weight was replaced, moved or changed in place."""
    def make():
        w = conv.weight.detach().to(torch.float32)
        return w.permute(2, 3, 1, 0).reshape(27, w.shape[0]).contiguous()
    return derived(conv, '_opa_stem3x3_w', (conv.weight,), make)


def stem_conv_out_hw(h, w, stride):
    """Output rows and columns of the 3x3 stem (padding 1) for an ``h`` x ``w`` input."""
    return (h - 1) // stride + 1, (w - 1) // stride + 1


def stem_conv3x3_supported(conv, x):
    """Can ``stem_conv3x3_bias_act(conv, x)`` run?  ``x``: a float32 ``[B, 3, H, W]`` tensor on the GPU in ANY layout with positive
    strides (NCHW, channels-last, a cropped view), outside autocast, nothing that autograd follows; ``conv``: a 3x3 convolution of
    stride 1 or 2, padding 1, no dilation, no groups, float32 weights on ``x``'s device, ``STEM_CHANNELS`` output channels (but
    ``STEM_DECLINED``), a float32 bias or none; sizes that ``opa_stem3x3_actp`` takes (32-bit indices, the batch in grid.y)."""
    if not (x.is_cuda and x.dim() == 4 and x.dtype == torch.float32 and x.shape[1] == 3 and not torch.is_autocast_enabled()):
        return False
    if x.requires_grad or (torch.is_grad_enabled() and any(p.requires_grad for p in conv.parameters())):
        return False
    if not (isinstance(conv, torch.nn.Conv2d) and conv.kernel_size == (3, 3) and conv.stride in ((1, 1), (2, 2)) and conv.padding == (1, 1)
            and conv.dilation == (1, 1) and conv.groups == 1 and conv.padding_mode == 'zeros' and conv.in_channels == 3
            and conv.out_channels in STEM_CHANNELS and conv.out_channels not in STEM_DECLINED
            and conv.weight.dtype == torch.float32 and conv.weight.device == x.device):
        return False
    bias = conv.bias
    if bias is not None and not (bias.dtype == torch.float32 and bias.device == x.device and bias.is_contiguous()
                                 and bias.data_ptr() % 16 == 0):
        return False
    B, _, H, W = x.shape
    ho, wo = stem_conv_out_hw(H, W, conv.stride[0])
    last = sum((n - 1) * s for n, s in zip(x.shape, x.stride()))                 # the last element addressed
    return (min(x.shape) > 0 and min(x.stride()) > 0 and x.data_ptr() % 4 == 0 and last < 2 ** 31
            and B * ho * wo * conv.out_channels < 2 ** 31 and B <= 65535 and _lib.available())


def stem_conv3x3_bias_act(conv, x, act=ACT_NONE, act_param=0.0):
    """``act(conv(x))`` for the 3x3 RGB stem of a ShuffleNetV2K, ShuffleNetV2, MobileNetV2, MobileNetV3 or SqueezeNet (folded with its
    batch norm: the bias is ``conv.bias``, or none) in one HIP kernel (``opa_stem3x3_actp``, ``csrc/stem.hip``): ``x`` is read through
    its own four strides, whatever its layout -- no copy --, the result is a dense channels-last float32 tensor.  ``act``:
    ``ACT_NONE`` / ``ACT_RELU`` / ``ACT_HARDSWISH`` / ``ACT_LEAKY_RELU`` / ``ACT_RELU6``, the last two with ``act_param`` (the slope / the
    cap).  ``stem_conv3x3_supported`` says whether this can run."""
    w = stem_weight_of(conv)
    B, _, H, W = x.shape
    s = conv.stride[0]
    out = _empty_nhwc(x, conv.out_channels, stem_conv_out_hw(H, W, s), torch.float32)
    _launch('opa_stem3x3_actp', _ptr(x), x.stride(0), x.stride(1), x.stride(2), x.stride(3), _ptr(w), _ptr(conv.bias), _ptr(out),
            B, H, W, conv.out_channels, s, int(act), float(act_param))
    return out


# ---- group norm ---------------------------------------------------------------------------------------------------------------------------

GN_CHUNK_PIXELS = 512                    # OPA_GN_CHUNK_PIXELS: pixels of one partial sum
GN_MAX_PIXELS = 65535 * GN_CHUNK_PIXELS  # grid.y of the moments kernel
GN_MAX_GROUP_WIDTH = 2048                # channels of one group (the coefficients kernel's LDS)
_GN_WORKSPACE = {}                       # (device, stream handle) -> the float64 tensor that holds the moments and the coefficients


def group_norm_supported(norm, x):
    """Can ``group_norm_act(norm, x)`` run?  ``norm``: a ``torch.nn.GroupNorm`` of ``x``'s channels with an EVEN number of channels per
    group, float32 affine terms on ``x``'s device or none; ``x``: float32 on the GPU, channels innermost -- a channels-last tensor or a
    channel slice of one -- with an even pitch between pixels, on an 8-byte boundary, outside autocast, nothing that autograd follows;
    sizes ``opa_groupnorm_actp`` takes; a library that has the entry point."""
    if not (isinstance(norm, torch.nn.GroupNorm) and x.is_cuda and x.dim() == 4 and x.dtype == torch.float32
            and not torch.is_autocast_enabled()):
        return False
    if x.requires_grad or (torch.is_grad_enabled() and any(p.requires_grad for p in norm.parameters())):
        return False
    B, C, H, W = x.shape
    G = norm.num_groups
    ps = _pixel_stride(x)
    if not (ps is not None and ps % 2 == 0 and x.data_ptr() % 8 == 0 and C == norm.num_channels and C % G == 0 and (C // G) % 2 == 0):
        return False
    for t in (norm.weight, norm.bias):
        if t is not None and not (t.dtype == torch.float32 and t.device == x.device and t.is_contiguous() and t.numel() == C):
            return False
    if not (0 < B <= 65535 and 0 < H * W <= GN_MAX_PIXELS and C // G <= GN_MAX_GROUP_WIDTH and H * W * (C // 2) < 2 ** 31
            and 0.0 <= norm.eps < float('inf')):
        return False
    return _lib.available() and hasattr(_lib.lib(), 'opa_groupnorm_actp')


def _gn_workspace(x, nbytes):
    """The workspace of ``group_norm_act``: one float64 tensor per device and stream, kept between calls and replaced by a larger one
    when a call needs more (the calls of a stream run in order, so they can share it; torch's allocator keeps a replaced tensor's
    memory until the stream has passed its last use).  A call inside a stream capture neither takes the kept tensor nor keeps its own:
    a graph bakes the address it was handed, and a kept tensor is freed as soon as an eager call outgrows it, so the capturing call
    always allocates -- from the graph's own pool, which lives as long as the graph -- and the table stays as it was."""
    if _capturing():
        return torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=x.device)
    key = (str(x.device), _stream())
    ws = _GN_WORKSPACE.get(key)
    if ws is None or ws.numel() * 8 < nbytes:
        ws = _GN_WORKSPACE[key] = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=x.device)
    return ws


def group_norm_act(norm, x, act=ACT_NONE, act_param=0.0, out=None):
    """``act(norm(x))`` for a ``torch.nn.GroupNorm`` (reference ``network/basenetworks.py:398-400``: the norms of a ShuffleNetV2K built
    with ``--shufflenetv2k-group-norm``) and the activation behind it, three launches of ``csrc/groupnorm.hip`` through
    ``opa_groupnorm_actp``: the moments of every 512 pixels per channel in float64, the coefficients per (image, channel), then
    ``act(fmaf(x, a, s))``.  ``x``: channels-last float32 or a channel slice; ``out``: a tensor of ``x``'s shape, channels innermost
    (``x`` itself: in place), default a new dense channels-last one; returned.  ``act``: ``ACT_NONE`` / ``ACT_RELU`` / ``ACT_HARDSWISH`` /
    ``ACT_LEAKY_RELU`` / ``ACT_RELU6``, the last two with ``act_param``.  The order of every addition depends on the shape alone.
    ``group_norm_supported`` says whether this can run."""
    B, C, H, W = x.shape
    if out is None:
        out = _empty_nhwc(x, C, dtype=torch.float32)
    nbytes = _lib.lib().opa_groupnorm_workspace_bytes(B, H * W, C)
    ws = _gn_workspace(x, nbytes)
    _launch('opa_groupnorm_actp', _ptr(x), _pixel_stride(x), _ptr(norm.weight), _ptr(norm.bias), _ptr(out), _pixel_stride(out), B, H * W, C,
            norm.num_groups, float(norm.eps), int(act), float(act_param), _ptr(ws), ws.numel() * 8)
    return out


# ---- squeeze-and-excitation ---------------------------------------------------------------------------------------------------------------

def _se_convs_ok(fc1, fc2):
    """The part of ``se_gate_supported`` that depends on the two convolutions alone."""
    def ok(conv):
        return (conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.padding == (0, 0) and conv.groups == 1
                and conv.bias is not None and conv.weight.dtype == torch.float32 and conv.bias.dtype == torch.float32
                and conv.weight.is_contiguous() and conv.bias.is_contiguous() and conv.bias.device == conv.weight.device)
    return (ok(fc1) and ok(fc2) and fc1.weight.device == fc2.weight.device and fc2.in_channels == fc1.out_channels
            and fc2.out_channels == fc1.in_channels and fc1.in_channels % 4 == 0 and fc1.in_channels <= 8192
            and fc1.out_channels <= 4096)


SE_MAX_PIXELS = 65535 * 512          # grid.y of the pool kernel x OPA_SE_POOL_PIXELS


def _se_operand_ok(x, channels):
    """Layout and size of the activation of ``se_gate`` / ``scale_channels_``: float32 on the GPU, ``channels`` channels innermost with
    a pitch between pixels that is a multiple of 4, on a 16-byte boundary, not followed by autograd."""
    ps = _pixel_stride(x) if x.dim() == 4 else None
    return (x.is_cuda and x.dtype == torch.float32 and not x.requires_grad and ps is not None and x.shape[1] == channels
            and channels % 4 == 0 and ps % 4 == 0 and x.data_ptr() % 16 == 0 and 0 < x.shape[0] <= 65535
            and 0 < x.shape[2] * x.shape[3] <= SE_MAX_PIXELS and _lib.available())


def se_gate_supported(x, fc1, fc2):
    """Can ``se_gate(x, fc1, fc2)`` run?  Two biased float32 1x1 convolutions C -> S -> C (C a multiple of 4, at most 8192; S at most
    4096) on ``x``'s device, ``x`` as ``_se_operand_ok`` says."""
    return _se_convs_ok(fc1, fc2) and _se_operand_ok(x, fc1.in_channels) and fc1.weight.device == x.device


def se_gate(x, fc1, fc2, mean_out=None):
    """The gate of a squeeze-and-excitation block: ``hardsigmoid(fc2(relu(fc1(mean of x over its pixels))))`` -> ``[B, C]`` float32
    (torchvision's ``SqueezeExcitation`` inside the reference's MobileNetV3, ``network/basenetworks.py:432-446``).  ``x``: channels-last
    float32 or a channel slice.  Two launches (``csrc/se.hip``): partial sums of 512 pixels each into a workspace, then the sums'
    reduction and the two matrix-vector products per image; the order of every addition depends on the shape alone.
    ``mean_out``: a contiguous float32 ``[B, C]`` tensor that receives the pooled mean as well (tests)."""
    B, C, H, W = x.shape
    nbytes = _lib.lib().opa_se_workspace_bytes(B, H * W, C)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=x.device)
    gate = torch.empty((B, C), dtype=torch.float32, device=x.device)
    _launch('opa_se_pool', _ptr(x), _pixel_stride(x), B, H * W, C, _ptr(ws), nbytes)
    _launch('opa_se_gate', _ptr(ws), nbytes, B, H * W, C, fc1.out_channels, _ptr(fc1.weight), _ptr(fc1.bias),
            _ptr(fc2.weight), _ptr(fc2.bias), _ptr(gate), _ptr(mean_out))
    return gate


def scale_channels_supported(x, gate):
    """Can ``scale_channels_(x, gate)`` run?  ``x`` as ``_se_operand_ok`` says, ``gate`` ``[B, C]`` float32, contiguous, on ``x``'s device."""
    return (x.dim() == 4 and _se_operand_ok(x, x.shape[1]) and gate.dtype == torch.float32 and gate.device == x.device
            and tuple(gate.shape) == (x.shape[0], x.shape[1]) and gate.is_contiguous() and gate.data_ptr() % 16 == 0)


def scale_channels_(x, gate):
    """In place ``x[b, c] *= gate[b, c]`` for a channels-last float32 activation or channel slice: one vectorised pass."""
    B, C, H, W = x.shape
    _launch('opa_se_scale', _ptr(x), _pixel_stride(x), B, H * W, C, _ptr(gate))
    return x


load_pinned()
