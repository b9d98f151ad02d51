"""MI355X-native PlainConvUNet behind the reference's network_architecture plugin surface.

Mirrors (names, constructor arguments, attributes, state_dict keys -- SURVEY.md App. C) the classes the reference
instantiates through nnUNet/nnunetv2/utilities/get_network_from_plans.py:70-83 (`PlainConvUNet` of the un-vendored
`dynamic_network_architectures`) and its fork-local decoder nnUNet/nnunetv2/training/my_network/UNetDecoder.py:13-121.
Every tensor operation is a hand-written HIP kernel reached through the C ABI (ops.py); the modules subclass the
torch.nn layer types only so that parameter registration, `state_dict()` keys, `InitWeights_He`
(network_initialization.py:4-12, which dispatches on isinstance(nn.Conv3d / nn.ConvTranspose3d)) and DDP-style
parameter handling behave exactly like the reference's modules.
"""
import os
from typing import List, Sequence, Tuple, Type, Union

import numpy as np
import torch
from torch import nn

from . import ops


# InstanceNorm-apply + LeakyReLU in the consumer conv's loader (bf16, z-marching kernel): on in inference; under autograd
# ("auto", the default) where the weight-gradient kernel has the same prologue (k_wgrad16z: the activated tensor is then
# written in neither pass), "1" = wherever the forward kernel takes it (the weight gradient of other shapes re-materialises
# the tensor), "0" = never
# gradient contributions of a tensor with two consumers summed inside the second consumer's kernel (ops._GradShare)
SHARE_GRADS = [os.environ.get("MVD_SHARE_GRADS", "1") != "0"]
FUSE_PROLOGUE = [os.environ.get("MVD_FUSE_PROLOGUE", "1") != "0"]
FUSE_PROLOGUE_TRAIN = [os.environ.get("MVD_FUSE_PROLOGUE_TRAIN", "auto")]
# the last decoder block's InstanceNorm + LeakyReLU inside the seg head that is its only consumer (ops.NormActSegHeadFn)
FUSE_SEGHEAD = [os.environ.get("MVD_FUSE_SEGHEAD", "1") != "0"]


def _tup3(v, dim=3):
    if isinstance(v, (int, np.integer)):
        return (int(v),) * dim
    return tuple(int(i) for i in v)


def _conv_dim(conv_op):
    """3 for nn.Conv3d (3d_fullres), 2 for nn.Conv2d (the 2d configuration); everything else is refused."""
    if conv_op is nn.Conv3d:
        return 3
    if conv_op is nn.Conv2d:
        return 2
    raise NotImplementedError(f"conv_op {conv_op!r}: nn.Conv3d (3d_fullres) and nn.Conv2d (2d) are built")


def _as5(t):
    return t.unsqueeze(2) if t is not None and t.dim() == 4 else t


class HipConv3d(nn.Conv3d):
    """nn.Conv3d whose forward is mvd_conv3d_fwd (NDHWC, fp32 MFMA implicit GEMM).  `x2` (optional) is a second
    input concatenated along channels without materialising the cat."""

    def forward(self, x, x2=None):
        return ops.Conv3dFn.apply(x, x2, self.weight, self.bias, self.stride)


class HipConvTranspose3d(nn.ConvTranspose3d):
    def forward(self, x):
        return ops.ConvTranspose3dFn.apply(x, self.weight, self.bias, self.stride)


class HipInstanceNorm3d(nn.InstanceNorm3d):
    """Stand-alone InstanceNorm3d is never used on the path; inside ConvDropoutNormReLU it is fused with the
    LeakyReLU (mvd_instnorm_lrelu_fwd).  Calling it alone applies slope 1 (identity activation)."""

    def forward(self, x):
        return ops.InstanceNormLeakyReLUFn.apply(x, self.weight, self.bias, self.eps, 1.0)


class HipBatchNorm3d(nn.BatchNorm3d):
    """nn.BatchNorm3d of the BN trainer variant (nnUNetTrainerBN.py:31-32); torch registers weight, bias, running_mean,
    running_var and num_batches_tracked, so the state_dict keys are the reference's.  Inside ConvDropoutNormReLU it is
    fused with the LeakyReLU (mvd_batchnorm_lrelu_fwd / _eval); calling it alone applies slope 1 (identity activation)."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True, **kwargs):
        if not affine:
            raise NotImplementedError("BatchNorm3d(affine=False) is not on the reference's path (nnUNetTrainerBN.py:32)")
        if not track_running_stats:
            raise NotImplementedError("BatchNorm3d(track_running_stats=False) is not built: the kernels keep running "
                                      "statistics")
        if momentum is None:
            raise NotImplementedError("BatchNorm3d(momentum=None), the cumulative moving average, is not built")
        super().__init__(num_features, eps=eps, momentum=momentum, affine=True, track_running_stats=True, **kwargs)

    def norm_act(self, x, slope, out_bf16=False):
        return ops.BatchNormLeakyReLUFn.apply(x, self.weight, self.bias, self.running_mean, self.running_var,
                                              self.num_batches_tracked, self.eps, self.momentum, slope, self.training,
                                              out_bf16)

    def forward(self, x):
        return self.norm_act(x, 1.0)


class HipSegLayer(nn.Conv3d):
    """1x1x1 Conv3d producing planar logits (decoder.seg_layers[s])."""

    def forward(self, x):
        return ops.SegHeadFn.apply(x, self.weight, self.bias)


# ------------------------------------------------------------------------------------------------ the 2d configuration
# The 2-D layers are torch's 2-D modules (parameter shapes, state_dict keys, InitWeights_He dispatch) whose forward is the
# 3-D autograd function on the [N,C,1,H,W] view of the activation: kernel (1,kh,kw), stride (1,s,s).  The PARAMETER itself
# goes into the function ([K,C,kh,kw] is the memory of [K,C,1,kh,kw]: ops.ks3), so the packed-weight cache, the flat
# gradient slices of optim.FlatParams and gradient sharing see the real parameter.  Called with [N,C,H,W] they return
# [N,K,H,W]; inside the network the activations stay [N,C,1,H,W] (NDHWC), so the attributes the kernels hang on their
# outputs (tile statistics, shared gradients) reach the consumer.
class HipConv2d(nn.Conv2d):
    """nn.Conv2d (kernel 3 or 1 per axis, stride 1 or 2) whose forward is ops.Conv3dFn on [N,C,1,H,W]; `x2`: a second
    input concatenated along channels without materialising the cat."""

    def forward(self, x, x2=None):
        y = ops.Conv3dFn.apply(_as5(x), _as5(x2), self.weight, self.bias, (1,) + tuple(self.stride))
        return y.squeeze(2) if x.dim() == 4 else y


class HipConvTranspose2d(nn.ConvTranspose2d):
    def forward(self, x):
        y = ops.ConvTranspose3dFn.apply(_as5(x), self.weight, self.bias, (1,) + tuple(self.stride))
        return y.squeeze(2) if x.dim() == 4 else y


class HipInstanceNorm2d(nn.InstanceNorm2d):
    """Inside ConvDropoutNormReLU it is fused with the LeakyReLU; calling it alone applies slope 1."""

    def forward(self, x):
        y = ops.InstanceNormLeakyReLUFn.apply(_as5(x), self.weight, self.bias, self.eps, 1.0)
        return y.squeeze(2) if x.dim() == 4 else y


class HipBatchNorm2d(nn.BatchNorm2d):
    """nn.BatchNorm2d of the BN trainer variant on 2-D plans (get_matching_batchnorm); refusals as HipBatchNorm3d."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True, **kwargs):
        if not affine:
            raise NotImplementedError("BatchNorm2d(affine=False) is not on the reference's path (nnUNetTrainerBN.py:32)")
        if not track_running_stats:
            raise NotImplementedError("BatchNorm2d(track_running_stats=False) is not built: the kernels keep running "
                                      "statistics")
        if momentum is None:
            raise NotImplementedError("BatchNorm2d(momentum=None), the cumulative moving average, is not built")
        super().__init__(num_features, eps=eps, momentum=momentum, affine=True, track_running_stats=True, **kwargs)

    def norm_act(self, x, slope, out_bf16=False):
        y = ops.BatchNormLeakyReLUFn.apply(_as5(x), self.weight, self.bias, self.running_mean, self.running_var,
                                           self.num_batches_tracked, self.eps, self.momentum, slope, self.training,
                                           out_bf16)
        return y.squeeze(2) if x.dim() == 4 else y

    def forward(self, x):
        return self.norm_act(x, 1.0)


class HipSegLayer2d(nn.Conv2d):
    """1x1 Conv2d producing planar logits (decoder.seg_layers[s] of a 2-D network)."""

    def forward(self, x):
        y = ops.SegHeadFn.apply(_as5(x), self.weight, self.bias)
        return y.squeeze(2) if x.dim() == 4 else y


class ConvDropoutNormReLU(nn.Module):
    """conv -> (no dropout) -> InstanceNorm3d -> LeakyReLU; kwargs as in get_network_from_plans.py:39-45.  The block of a
    BatchNorm3d network is the subclass ConvDropoutBatchNormReLU below: this class keeps refusing every other norm_op."""
    batch_norm = False                                     # (True in ConvDropoutBatchNormReLU)
    _norm_ops = (nn.InstanceNorm3d, HipInstanceNorm3d)     # what norm_op must subclass, what the block builds
    _norm_ops_2d = (nn.InstanceNorm2d, HipInstanceNorm2d)  # the same for conv_op = nn.Conv2d

    def __init__(self, conv_op, input_channels, output_channels, kernel_size, stride, conv_bias=False, norm_op=None,
                 norm_op_kwargs=None, dropout_op=None, dropout_op_kwargs=None, nonlin=None, nonlin_kwargs=None,
                 nonlin_first=False):
        super().__init__()
        self.dim = dim = _conv_dim(conv_op) if conv_op is not None else 3
        norm_ops = self._norm_ops if dim == 3 else self._norm_ops_2d
        if dropout_op is not None:
            raise NotImplementedError("dropout is not on the reference's path (get_network_from_plans.py:43)")
        if nonlin_first:
            raise NotImplementedError("nonlin_first=False on the reference's path")
        # the fused kernel IS InstanceNorm3d(affine) + LeakyReLU (get_network_from_plans.py:41-44): anything else in the
        # plans would silently compute something different, so refuse it
        if norm_op is not None and not (isinstance(norm_op, type) and issubclass(norm_op, norm_ops[0])):
            raise NotImplementedError(f"norm_op {norm_op!r}: only nn.{norm_ops[0].__name__} is on the reference's path")
        if norm_op is None:
            raise NotImplementedError("norm_op=None: the fused conv block always normalises (InstanceNorm3d)")
        if nonlin is not None and not (isinstance(nonlin, type) and issubclass(nonlin, nn.LeakyReLU)):
            raise NotImplementedError(f"nonlin {nonlin!r}: only nn.LeakyReLU is on the reference's path")
        if nonlin is None:
            raise NotImplementedError("nonlin=None: the fused conv block always applies LeakyReLU")
        if not dict(norm_op_kwargs or {'affine': True}).get('affine', False):
            raise NotImplementedError(f"{norm_ops[0].__name__}(affine=False) is not on the reference's path")
        self.input_channels, self.output_channels = input_channels, output_channels
        self.stride = _tup3(stride, dim)
        k = _tup3(kernel_size, dim)
        if len(k) != dim or len(self.stride) != dim:
            raise NotImplementedError(f"kernel size {k} / stride {self.stride} do not have the {dim} axes of {conv_op.__name__}")
        if dim == 2 and not (all(i in (1, 3) for i in k) and all(i in (1, 2) for i in self.stride)):
            raise NotImplementedError(f"2-D conv: kernel size 3 or 1 and stride 1 or 2 per axis are built (got {k}, {self.stride})")
        self.conv = (HipConv3d if dim == 3 else HipConv2d)(input_channels, output_channels, k, self.stride,
                                                           padding=[(i - 1) // 2 for i in k], dilation=1, bias=conv_bias)
        norm_op_kwargs = norm_op_kwargs or {'eps': 1e-5, 'affine': True}
        self.norm = norm_ops[1](output_channels, **norm_op_kwargs)
        nonlin_kwargs = dict(nonlin_kwargs or {'inplace': True})
        self.nonlin = nonlin(**nonlin_kwargs)
        self.all_modules = nn.Sequential(self.conv, self.norm, self.nonlin)
        self.precision = "fp32"  # "bf16": see set_precision()

    def conv_only(self, x, x2=None):
        """The block's convolution alone (raw output; in bf16 with the InstanceNorm statistics from the conv's epilogue
        attached when the kernel emits them)."""
        cw = self.conv.weight
        if (self.precision == "bf16" and x2 is None and x.dtype == torch.float32 and x.shape[1] <= 8 and
                cw.shape[0] % 32 == 0 and tuple(cw.shape[2:]) == (3, 3, 3) and self.stride == (1, 1, 1) and x.is_cuda):
            # the 4-modality input layer under mixed precision: bf16 operands like every other conv of the net
            return ops.NarrowInputConv3dBf16Fn.apply(x, cw, self.conv.bias)
        return self.conv(x, x2)

    def norm_act(self, y):
        return ops.InstanceNormLeakyReLUFn.apply(y, self.norm.weight, self.norm.bias, self.norm.eps,
                                                 self.nonlin.negative_slope, self.precision == "bf16")

    def forward(self, x, x2=None):
        return self.norm_act(self.conv_only(x, x2))

    def forward_from_raw(self, prev, y_raw):
        """This block's conv fed with the RAW conv output of the previous block `prev`: prev's InstanceNorm + LeakyReLU run
        inside this conv's loader (ops.NormActConv3dFn).  Returns this block's raw conv output."""
        return ops.NormActConv3dFn.apply(y_raw, prev.norm.weight, prev.norm.bias, prev.norm.eps,
                                         prev.nonlin.negative_slope, self.conv.weight, self.conv.bias)

    def compute_conv_feature_map_size(self, input_size):
        output_size = [i // j for i, j in zip(input_size, self.stride)]
        return np.prod([self.output_channels, *output_size], dtype=np.int64)


class ConvDropoutBatchNormReLU(ConvDropoutNormReLU):
    """conv -> BatchNorm3d -> LeakyReLU, the block of the BN trainer variant (nnUNetTrainerBN.py:31-32): its own kernels
    (mvd_batchnorm_lrelu_*), batch statistics in train(), running statistics in eval(); never an InstanceNorm fusion."""
    batch_norm = True
    _norm_ops = (nn.BatchNorm3d, HipBatchNorm3d)
    _norm_ops_2d = (nn.BatchNorm2d, HipBatchNorm2d)

    def norm_act(self, y):
        return self.norm.norm_act(y, self.nonlin.negative_slope, self.precision == "bf16")


class StackedConvBlocks(nn.Module):
    def __init__(self, num_convs, conv_op, input_channels, output_channels, kernel_size, initial_stride,
                 conv_bias=False, norm_op=None, norm_op_kwargs=None, dropout_op=None, dropout_op_kwargs=None,
                 nonlin=None, nonlin_kwargs=None, nonlin_first=False):
        super().__init__()
        if not isinstance(output_channels, (tuple, list)):
            output_channels = [output_channels] * num_convs
        # a norm_op that subclasses nn.BatchNorm3d selects the BN block; everything else goes to (and is judged by) the
        # InstanceNorm block
        dim = _conv_dim(conv_op) if conv_op is not None else 3
        block = ConvDropoutBatchNormReLU if isinstance(norm_op, type) and \
            issubclass(norm_op, nn.BatchNorm3d if dim == 3 else nn.BatchNorm2d) else ConvDropoutNormReLU
        self.convs = nn.Sequential(
            block(conv_op, input_channels, output_channels[0], kernel_size, initial_stride, conv_bias,
                  norm_op, norm_op_kwargs, dropout_op, dropout_op_kwargs, nonlin, nonlin_kwargs, nonlin_first),
            *[block(conv_op, output_channels[i - 1], output_channels[i], kernel_size, 1, conv_bias,
                    norm_op, norm_op_kwargs, dropout_op, dropout_op_kwargs, nonlin, nonlin_kwargs, nonlin_first)
              for i in range(1, num_convs)])
        self.output_channels = output_channels[-1]
        self.initial_stride = _tup3(initial_stride, dim)

    def forward(self, x, x2=None, raw_tail=False):
        """conv -> norm -> act per block.  raw_tail (the last decoder stage in front of its seg head, bf16): the LAST block's
        norm + act are left to the consumer -- returns (raw conv output, that block); None when the chain did not end fused.
        bf16 mixed precision, consecutive blocks whose second conv takes the z-marching
        kernel (3x3x3, stride 1, 32 -> 32 channels at the patch resolution): the first block's InstanceNorm + LeakyReLU is
        folded into the second conv's loader (no apply pass, the activated tensor is never written) --
        in inference and, where the weight-gradient kernel has the same prologue, in training (FUSE_PROLOGUE_TRAIN)."""
        blocks = list(self.convs)
        raw = None   # the raw conv output of the previous block when its norm + act are still pending
        for i, blk in enumerate(blocks):
            nxt = blocks[i + 1] if i + 1 < len(blocks) else None
            fuse_next = nxt is not None and self._can_fuse(blk, nxt, x if raw is None else raw)
            tail = raw_tail and nxt is None and FUSE_PROLOGUE[0] and not blk.batch_norm
            if raw is None and not fuse_next and not tail:
                x = blk(x, x2) if i == 0 else blk(x)      # the plain module call (forward hooks fire)
                continue
            y = blk.forward_from_raw(blocks[i - 1], raw) if raw is not None else \
                (blk.conv_only(x, x2) if i == 0 else blk.conv_only(x))
            if fuse_next and ops.fused_norm_conv_ok(y, nxt.conv.weight, nxt.stride):
                raw = y
                continue
            if tail:
                return y, blk
            raw = None
            x = blk.norm_act(y)
        return (x, None) if raw_tail else x

    @staticmethod
    def _can_fuse(blk, nxt, inp):
        """Shape-only test (before anything runs) whether blk's InstanceNorm + LeakyReLU can ride in nxt's conv loader."""
        if blk.batch_norm:   # batch statistics: the loader prologues carry per-sample scale / shift
            return False
        train = torch.is_grad_enabled()
        mode = str(FUSE_PROLOGUE_TRAIN[0]).lower()
        if not (blk.precision == "bf16" and FUSE_PROLOGUE[0]) or (train and mode in ("0", "false")):
            return False
        w = nxt.conv.weight
        if tuple(w.shape[2:]) != (3, 3, 3) or nxt.stride != (1, 1, 1) or w.shape[1] != blk.output_channels or not inp.is_cuda:
            return False
        sp = [(d + 2 * ((k - 1) // 2) - k) // st + 1 for d, k, st in zip(inp.shape[2:], blk.conv.kernel_size, blk.stride)]
        shape = (inp.shape[0], sp[0], sp[1], sp[2], blk.output_channels, 0, w.shape[0], ops.i3((3, 3, 3)), ops.i3((1, 1, 1)))
        if ops.query("mvd_conv3d_fwd_bf16_prologue_ok", *shape) <= 0:
            return False
        if blk.output_channels > 32 and os.environ.get("MVD_FUSE_PROLOGUE_C64", "1") == "0":   # (A/B: the 64-channel blocks)
            return False
        if train and mode not in ("1", "true"):   # "auto": only where the weight gradient has the prologue too
            return ops.WGRAD_PROLOGUE and ops.query("mvd_conv3d_wgrad_bf16_prologue_ok", *shape) > 0
        return True

    def compute_conv_feature_map_size(self, input_size):
        output = self.convs[0].compute_conv_feature_map_size(input_size)
        size_after_stride = [i // j for i, j in zip(input_size, self.initial_stride)]
        for b in self.convs[1:]:
            output += b.compute_conv_feature_map_size(size_after_stride)
        return output


class PlainConvEncoder(nn.Module):
    def __init__(self, input_channels: int, n_stages: int, features_per_stage: Union[int, Sequence[int]],
                 conv_op: Type = nn.Conv3d, kernel_sizes=3, strides=1, n_conv_per_stage: Union[int, Sequence[int]] = 2,
                 conv_bias: bool = False, norm_op=None, norm_op_kwargs=None, dropout_op=None, dropout_op_kwargs=None,
                 nonlin=None, nonlin_kwargs=None, return_skips: bool = False, nonlin_first: bool = False,
                 pool: str = 'conv'):
        super().__init__()
        dim = _conv_dim(conv_op)
        if pool != 'conv':
            raise NotImplementedError("the reference's plans use strided convolutions (pool='conv')")
        if isinstance(kernel_sizes, int):
            kernel_sizes = [kernel_sizes] * n_stages
        if isinstance(features_per_stage, int):
            features_per_stage = [features_per_stage] * n_stages
        if isinstance(n_conv_per_stage, int):
            n_conv_per_stage = [n_conv_per_stage] * n_stages
        if isinstance(strides, int):
            strides = [strides] * n_stages
        assert len(kernel_sizes) == n_stages and len(n_conv_per_stage) == n_stages
        assert len(features_per_stage) == n_stages and len(strides) == n_stages
        stages = []
        for s in range(n_stages):
            stages.append(nn.Sequential(StackedConvBlocks(
                n_conv_per_stage[s], conv_op, input_channels, features_per_stage[s], kernel_sizes[s], strides[s],
                conv_bias, norm_op, norm_op_kwargs, dropout_op, dropout_op_kwargs, nonlin, nonlin_kwargs, nonlin_first)))
            input_channels = features_per_stage[s]
        self.stages = nn.Sequential(*stages)
        self.output_channels = list(features_per_stage)
        self.strides = [_tup3(i, dim) for i in strides]
        self.return_skips = return_skips
        # read by the decoder (UNetDecoder.py:39-65)
        self.conv_op, self.norm_op, self.norm_op_kwargs = conv_op, norm_op, norm_op_kwargs
        self.nonlin, self.nonlin_kwargs = nonlin, nonlin_kwargs
        self.dropout_op, self.dropout_op_kwargs = dropout_op, dropout_op_kwargs
        self.conv_bias, self.kernel_sizes = conv_bias, [_tup3(k, dim) for k in kernel_sizes]

    def forward(self, x):
        ret = []
        last = len(self.stages) - 1
        for i, s in enumerate(self.stages):
            x = s(x)
            if self.return_skips and i != last and SHARE_GRADS[0]:
                ops.share_grad(x)   # a skip: read by the next stage AND by the decoder -> one gradient buffer (ops._GradShare)
            ret.append(x)
        return ret if self.return_skips else ret[-1]

    def compute_conv_feature_map_size(self, input_size):
        output = np.int64(0)
        for s in range(len(self.stages)):
            output += self.stages[s][-1].compute_conv_feature_map_size(input_size)
            input_size = [i // j for i, j in zip(input_size, self.strides[s])]
        return output


class UNetDecoder(nn.Module):
    """UNetDecoder.py:13-121 (without the fork's bottleneck attention insert :75-81,:91-102): per stage
    transpconv -> [cat] -> stacked convs -> 1x1x1 seg layer; outputs high-res first."""

    def __init__(self, encoder: PlainConvEncoder, num_classes: int,
                 n_conv_per_stage: Union[int, Tuple[int, ...], List[int]], deep_supervision,
                 nonlin_first: bool = False):
        super().__init__()
        self.deep_supervision = deep_supervision
        self.encoder = encoder
        self.num_classes = num_classes
        n_stages_encoder = len(encoder.output_channels)
        if isinstance(n_conv_per_stage, int):
            n_conv_per_stage = [n_conv_per_stage] * (n_stages_encoder - 1)
        assert len(n_conv_per_stage) == n_stages_encoder - 1
        stages, transpconvs, seg_layers = [], [], []
        dim3 = _conv_dim(encoder.conv_op) == 3
        HipConvTranspose, HipSeg = (HipConvTranspose3d, HipSegLayer) if dim3 else (HipConvTranspose2d, HipSegLayer2d)
        for s in range(1, n_stages_encoder):
            below = encoder.output_channels[-s]
            skip = encoder.output_channels[-(s + 1)]
            st = encoder.strides[-s]
            transpconvs.append(HipConvTranspose(below, skip, st, st, bias=encoder.conv_bias))
            stages.append(StackedConvBlocks(
                n_conv_per_stage[s - 1], encoder.conv_op, 2 * skip, skip, encoder.kernel_sizes[-(s + 1)], 1,
                encoder.conv_bias, encoder.norm_op, encoder.norm_op_kwargs, encoder.dropout_op,
                encoder.dropout_op_kwargs, encoder.nonlin, encoder.nonlin_kwargs, nonlin_first))
            seg_layers.append(HipSeg(skip, num_classes, 1, 1, 0, bias=True))
        self.stages = nn.ModuleList(stages)
        self.transpconvs = nn.ModuleList(transpconvs)
        self.seg_layers = nn.ModuleList(seg_layers)

    def forward(self, skips, return_last_feature=False):
        """Bottom-up: up-sample, fuse with the encoder feature of that resolution, refine, emit logits.  Same contract
        as UNetDecoder.py:104-121: list of logits, highest resolution first, with deep supervision; one tensor without."""
        feat = skips[-1]
        last = len(self.stages) - 1
        logits = []
        for level, (up, refine, head) in enumerate(zip(self.transpconvs, self.stages, self.seg_layers)):
            # the concatenation of (up-sampled, skip) is never materialised: the first conv reads both pointers
            head_l = head if self.deep_supervision else self.seg_layers[-1]
            if level == last and not return_last_feature and FUSE_SEGHEAD[0] and isinstance(refine, StackedConvBlocks):
                # the top stage's output feeds the seg head alone: its last InstanceNorm + LeakyReLU ride in the head's loaders
                y_raw, blk = refine(up(feat), skips[-(level + 2)], raw_tail=True)
                if blk is not None and ops.fused_norm_seghead_ok(y_raw, head_l.weight):
                    logits.append(ops.NormActSegHeadFn.apply(y_raw, blk.norm.weight, blk.norm.bias, blk.norm.eps,
                                                             blk.nonlin.negative_slope, head_l.weight, head_l.bias))
                    feat = None
                    continue
                feat = y_raw if blk is None else blk.norm_act(y_raw)
            else:
                feat = refine(up(feat), skips[-(level + 2)])
            if self.deep_supervision and level != last and SHARE_GRADS[0]:
                ops.share_grad(feat)   # two consumers (this level's seg head, the next level's up-sampling): one gradient buffer
            if self.deep_supervision:
                logits.append(head(feat))
            elif level == last:
                logits.append(self.seg_layers[-1](feat))
        out = logits[::-1] if self.deep_supervision else logits[0]
        return (out, feat) if return_last_feature else out

    def compute_conv_feature_map_size(self, input_size):
        """Number of feature-map elements the decoder produces for one sample (the planner's VRAM proxy,
        UNetDecoder.py:123-150): per resolution the refined maps, the up-sampled map and the logits that are emitted."""
        sizes, cur = [], list(input_size)
        for st in self.encoder.strides[:-1]:
            cur = [i // j for i, j in zip(cur, st)]
            sizes.append(cur)
        total = np.int64(0)
        n = len(self.stages)
        for level in range(n):
            sp = sizes[-(level + 1)]
            voxels = np.prod(sp, dtype=np.int64)
            total += self.stages[level].compute_conv_feature_map_size(sp)
            total += self.encoder.output_channels[-(level + 2)] * voxels           # transposed-conv output
            if self.deep_supervision or level == n - 1:
                total += self.num_classes * voxels
        return total


class MI355PlainConvUNet(nn.Module):
    """Drop-in for dynamic_network_architectures.architectures.unet.PlainConvUNet (same constructor signature)."""

    def __init__(self, input_channels: int, n_stages: int, features_per_stage: Union[int, Sequence[int]],
                 conv_op: Type = nn.Conv3d, kernel_sizes=3, strides=1, n_conv_per_stage: Union[int, Sequence[int]] = 2,
                 num_classes: int = 2, n_conv_per_stage_decoder: Union[int, Sequence[int]] = 2, conv_bias: bool = False,
                 norm_op=None, norm_op_kwargs=None, dropout_op=None, dropout_op_kwargs=None, nonlin=None,
                 nonlin_kwargs=None, deep_supervision: bool = False, nonlin_first: bool = False):
        super().__init__()
        if isinstance(n_conv_per_stage, int):
            n_conv_per_stage = [n_conv_per_stage] * n_stages
        if isinstance(n_conv_per_stage_decoder, int):
            n_conv_per_stage_decoder = [n_conv_per_stage_decoder] * (n_stages - 1)
        assert len(n_conv_per_stage) == n_stages
        assert len(n_conv_per_stage_decoder) == (n_stages - 1)
        self.encoder = PlainConvEncoder(input_channels, n_stages, features_per_stage, conv_op, kernel_sizes, strides,
                                        n_conv_per_stage, conv_bias, norm_op, norm_op_kwargs, dropout_op,
                                        dropout_op_kwargs, nonlin, nonlin_kwargs, return_skips=True,
                                        nonlin_first=nonlin_first)
        self.decoder = UNetDecoder(self.encoder, num_classes, n_conv_per_stage_decoder, deep_supervision,
                                   nonlin_first=nonlin_first)

    def forward(self, x, return_last_feature=False):
        if not x.is_cuda:
            raise RuntimeError("MI355PlainConvUNet runs on the MI355X only (no CPU path); move the input to cuda")
        if _conv_dim(self.encoder.conv_op) == 2:
            # the 2d configuration: [N,C,H,W] in, [N,K,h,w] logits out; inside, every tensor is the [N,C,1,H,W] view
            if x.dim() != 4:
                raise RuntimeError(f"2-D MI355PlainConvUNet: input must be [N,C,H,W], got {tuple(x.shape)}")
            out = self.decoder(self.encoder(ops.to_ndhwc(x.unsqueeze(2))), return_last_feature)
            sq = lambda o: [t.squeeze(2) for t in o] if isinstance(o, (list, tuple)) else o.squeeze(2)
            if return_last_feature:
                return sq(out[0]), (out[1].squeeze(2) if out[1] is not None else None)
            return sq(out)
        skips = self.encoder(ops.to_ndhwc(x))
        return self.decoder(skips, return_last_feature)

    def compute_conv_feature_map_size(self, input_size):
        return self.encoder.compute_conv_feature_map_size(input_size) + \
            self.decoder.compute_conv_feature_map_size(input_size)

    def parameters_in_execution_order(self):
        """Parameters in the order the forward pass first uses them: encoder stages, then per decoder level the transposed
        conv, the refining convs and the seg layer.  `parameters()` lists them by module type (all stages, all transposed
        convs, all seg layers).  optim.FlatParams lays the flat gradient buffer out in THIS order, so that a suffix of the
        buffer is complete exactly when backward has passed the corresponding part of the network: the reducer's buckets
        (contiguous slices, cut from the end) then fire in backward order while the rest of backward still runs."""
        out = list(self.encoder.parameters())
        for up, refine, head in zip(self.decoder.transpconvs, self.decoder.stages, self.decoder.seg_layers):
            out += list(up.parameters()) + list(refine.parameters()) + list(head.parameters())
        seen, uniq = set(), []
        for p in out + list(self.parameters()):   # (anything not covered above keeps its registration order at the end)
            if id(p) not in seen:
                seen.add(id(p))
                uniq.append(p)
        return uniq


# ------------------------------------------------------------------------------------------------ ResidualEncoderUNet
# The network class the ResEncUNetPlanner's plans name (resencUNet_planner.py, get_network_from_plans.py:34-37, 46-52, 61-65,
# 90-91): dynamic_network_architectures' ResidualEncoderUNet restated -- a stem, per stage a stack of BasicBlockD, the plain
# decoder.  fp32, InstanceNorm; the tail of every block (norm of conv2 + skip + LeakyReLU) is one kernel pair
# (ops.ResidualAddNormActFn), the skip branch's pool another (ops.AvgPool3dFn).  DESIGN 36.
def _refuse_resenc(what):
    raise NotImplementedError(f"ResidualEncoderUNet: {what}")


class ConvDropoutNorm(nn.Module):
    """conv -> (no dropout) -> InstanceNorm with NO nonlinearity: conv2 and the skip projection of BasicBlockD (the package
    builds them as ConvDropoutNormReLU(nonlin=None), so `all_modules` is Sequential(conv, norm)).  A sibling of
    ConvDropoutNormReLU, which keeps refusing nonlin=None.  Inside a block only `conv` runs here: the norm's parameters go
    into the block tail's kernel.  Called on its own it normalises with slope 1."""

    def __init__(self, conv_op, input_channels, output_channels, kernel_size, stride, conv_bias=False, norm_op=None,
                 norm_op_kwargs=None):
        super().__init__()
        self.dim = dim = _conv_dim(conv_op)
        norm_ops = ConvDropoutNormReLU._norm_ops if dim == 3 else ConvDropoutNormReLU._norm_ops_2d
        if not (isinstance(norm_op, type) and issubclass(norm_op, norm_ops[0])):
            _refuse_resenc(f"norm_op {norm_op!r}: only nn.{norm_ops[0].__name__} is built (no BatchNorm residual blocks)")
        if not dict(norm_op_kwargs or {'affine': True}).get('affine', False):
            _refuse_resenc(f"{norm_ops[0].__name__}(affine=False) is not on the reference's path")
        self.input_channels, self.output_channels = input_channels, output_channels
        self.stride = _tup3(stride, dim)
        k = _tup3(kernel_size, dim)
        if len(k) != dim or len(self.stride) != dim:
            _refuse_resenc(f"kernel size {k} / stride {self.stride} do not have the {dim} axes of {conv_op.__name__}")
        if not (all(i in (1, 3) for i in k) and all(i in (1, 2) for i in self.stride)):
            _refuse_resenc(f"kernel size 3 or 1 and stride 1 or 2 per axis are built (got {k}, {self.stride})")
        self.conv = (HipConv3d if dim == 3 else HipConv2d)(input_channels, output_channels, k, self.stride,
                                                           padding=[(i - 1) // 2 for i in k], dilation=1, bias=conv_bias)
        self.norm = norm_ops[1](output_channels, **(norm_op_kwargs or {'eps': 1e-5, 'affine': True}))
        self.all_modules = nn.Sequential(self.conv, self.norm)

    def forward(self, x):
        return self.norm(self.conv(x))


class HipAvgPool3d(nn.AvgPool3d):
    def forward(self, x):
        return ops.AvgPool3dFn.apply(x, _tup3(self.stride, 3))


class HipAvgPool2d(nn.AvgPool2d):
    """AvgPool2d on the [N,C,1,H,W] view of a 2-D network's activation."""

    def forward(self, x):
        y = ops.AvgPool3dFn.apply(_as5(x), (1,) + _tup3(self.stride, 2))
        return y.squeeze(2) if x.dim() == 4 else y


class BasicBlockD(nn.Module):
    """conv1 (conv, norm, LeakyReLU) -> conv2 (conv, norm) -> + skip(x) -> LeakyReLU.  skip: the identity when neither the
    stride nor the channel count changes, else nn.Sequential of an average pool (kernel = stride) when strided, then a 1x1x1
    conv (bias=False) + norm when the channels change -- so the parameter keys are skip.0.* or skip.1.*."""

    def __init__(self, conv_op, input_channels, output_channels, kernel_size, stride, conv_bias=False, norm_op=None,
                 norm_op_kwargs=None, dropout_op=None, dropout_op_kwargs=None, nonlin=None, nonlin_kwargs=None,
                 stochastic_depth_p=0.0, squeeze_excitation=False, squeeze_excitation_reduction_ratio=1. / 16):
        super().__init__()
        self.dim = dim = _conv_dim(conv_op)
        if stochastic_depth_p:
            _refuse_resenc(f"stochastic depth (p = {stochastic_depth_p}) is not built")
        if squeeze_excitation:
            _refuse_resenc("squeeze-and-excitation is not built")
        if dropout_op is not None:
            _refuse_resenc("dropout is not on the reference's path (get_network_from_plans.py:43)")
        if not (isinstance(nonlin, type) and issubclass(nonlin, nn.LeakyReLU)):
            _refuse_resenc(f"nonlin {nonlin!r}: only nn.LeakyReLU is built")
        if isinstance(norm_op, type) and issubclass(norm_op, (nn.BatchNorm2d, nn.BatchNorm3d)):
            _refuse_resenc(f"norm_op {norm_op.__name__}: BatchNorm residual blocks are not built (InstanceNorm only)")
        self.input_channels, self.output_channels = input_channels, output_channels
        self.stride = _tup3(stride, dim)
        self.conv1 = ConvDropoutNormReLU(conv_op, input_channels, output_channels, kernel_size, self.stride, conv_bias, norm_op,
                                         norm_op_kwargs, None, None, nonlin, nonlin_kwargs)
        self.conv2 = ConvDropoutNorm(conv_op, output_channels, output_channels, kernel_size, 1, conv_bias, norm_op,
                                     norm_op_kwargs)
        self.nonlin2 = nonlin(**dict(nonlin_kwargs or {'inplace': True}))
        has_stride = any(i != 1 for i in self.stride)
        requires_projection = input_channels != output_channels
        if has_stride or requires_projection:
            ops_ = []
            if has_stride:
                ops_.append((HipAvgPool3d if dim == 3 else HipAvgPool2d)(self.stride, self.stride))
            if requires_projection:
                ops_.append(ConvDropoutNorm(conv_op, input_channels, output_channels, 1, 1, False, norm_op, norm_op_kwargs))
            self.skip = nn.Sequential(*ops_)
        else:
            self.skip = nn.Identity()   # (torch's `lambda x: x` in the package: no parameters, no keys either way)
        self._pool = has_stride
        self._proj = requires_projection

    def forward(self, x):
        x = _as5(x)
        # x has two consumers here (conv1 and the skip branch): one gradient buffer (ops._GradShare).  A stage output the
        # encoder tagged already (the decoder reads it as well) keeps its tag: the skip branch's pool / the block tail add
        # into the decoder's buffer and leave it published for conv1.  The conv branch is built FIRST, so that in the backward
        # pass the skip branch's node runs before conv1's: the pool / the tail add IN PLACE into the buffer autograd holds as
        # the decoder's contribution, before any other contribution arrives and autograd sums (out of place).
        tagged = ops._share_of(x) is not None
        if tagged and self._proj and not self._pool:
            # A projection conv directly on a tagged tensor (a later stage at stride 1 that changes channels) cannot take part
            # in that: a Conv3dFn that finds a buffer it cannot join publishes its own OVER it and returns it, autograd sums
            # the two out of place, and conv1 would then join a buffer nobody reads.  This block therefore works on a view of
            # x with a share of its own (its two consumers); the view's backward hands their sum to autograd, which adds it
            # to the decoder's contribution.
            x, tagged = x.view_as(x), False
        if not tagged and SHARE_GRADS[0]:
            ops.share_grad(x)
        a = self.conv2.conv(self.conv1(x))
        r, gr, br = x, None, None
        if self._pool:
            r = ops.AvgPool3dFn.apply(r, self.stride if self.dim == 3 else (1,) + self.stride)
        if self._proj:
            p = self.skip[-1]
            r = p.conv(r)
            gr, br = p.norm.weight, p.norm.bias
        n2 = self.conv2.norm
        return ops.ResidualAddNormActFn.apply(a, n2.weight, n2.bias, r, gr, br, n2.eps, self.nonlin2.negative_slope)

    def compute_conv_feature_map_size(self, input_size):
        """Two maps of output_channels at the strided size (conv1, conv2), a third when the skip is not the identity."""
        size_after_stride = [i // j for i, j in zip(input_size, self.stride)]
        one = np.prod([self.output_channels, *size_after_stride], dtype=np.int64)
        return one * (3 if (self._pool or self._proj) else 2)


class StackedResidualBlocks(nn.Module):
    """n_blocks residual blocks: the first takes the stride and the channel change, the rest run at stride 1."""

    def __init__(self, n_blocks, conv_op, input_channels, output_channels, kernel_size, initial_stride, conv_bias=False,
                 norm_op=None, norm_op_kwargs=None, dropout_op=None, dropout_op_kwargs=None, nonlin=None, nonlin_kwargs=None,
                 block=BasicBlockD, bottleneck_channels=None, stochastic_depth_p=0.0, squeeze_excitation=False,
                 squeeze_excitation_reduction_ratio=1. / 16):
        super().__init__()
        assert n_blocks > 0, 'n_blocks must be > 0'
        if block is not BasicBlockD:
            _refuse_resenc(f"block {getattr(block, '__name__', block)!r}: only BasicBlockD is built (no BottleneckD)")
        if bottleneck_channels is not None:
            _refuse_resenc("bottleneck_channels belong to BottleneckD, which is not built")
        if not isinstance(output_channels, (tuple, list)):
            output_channels = [output_channels] * n_blocks
        dim = _conv_dim(conv_op)
        extra = (stochastic_depth_p, squeeze_excitation, squeeze_excitation_reduction_ratio)
        self.blocks = nn.Sequential(
            block(conv_op, input_channels, output_channels[0], kernel_size, initial_stride, conv_bias, norm_op, norm_op_kwargs,
                  dropout_op, dropout_op_kwargs, nonlin, nonlin_kwargs, *extra),
            *[block(conv_op, output_channels[n - 1], output_channels[n], kernel_size, 1, conv_bias, norm_op, norm_op_kwargs,
                    dropout_op, dropout_op_kwargs, nonlin, nonlin_kwargs, *extra) for n in range(1, n_blocks)])
        self.initial_stride = _tup3(initial_stride, dim)
        self.output_channels = output_channels[-1]

    def forward(self, x):
        return self.blocks(x)

    def compute_conv_feature_map_size(self, input_size):
        output = self.blocks[0].compute_conv_feature_map_size(input_size)
        size_after_stride = [i // j for i, j in zip(input_size, self.initial_stride)]
        for b in self.blocks[1:]:
            output += b.compute_conv_feature_map_size(size_after_stride)
        return output


class ResidualEncoder(nn.Module):
    def __init__(self, input_channels: int, n_stages: int, features_per_stage: Union[int, Sequence[int]],
                 conv_op: Type = nn.Conv3d, kernel_sizes=3, strides=1, n_blocks_per_stage: Union[int, Sequence[int]] = 2,
                 conv_bias: bool = False, norm_op=None, norm_op_kwargs=None, dropout_op=None, dropout_op_kwargs=None,
                 nonlin=None, nonlin_kwargs=None, block=BasicBlockD, bottleneck_channels=None, return_skips: bool = False,
                 disable_default_stem: bool = False, stem_channels: int = None, pool_type: str = 'conv',
                 stochastic_depth_p: float = 0.0, squeeze_excitation: bool = False,
                 squeeze_excitation_reduction_ratio: float = 1. / 16):
        super().__init__()
        dim = _conv_dim(conv_op)
        if pool_type != 'conv':
            _refuse_resenc(f"pool {pool_type!r}: the plans use strided convolutions (pool='conv')")
        if disable_default_stem:
            _refuse_resenc("disable_default_stem is not built (the plans keep the stem)")
        if dropout_op is not None:
            _refuse_resenc("dropout is not on the reference's path (get_network_from_plans.py:43)")
        if isinstance(norm_op, type) and issubclass(norm_op, (nn.BatchNorm2d, nn.BatchNorm3d)):
            _refuse_resenc(f"norm_op {norm_op.__name__}: BatchNorm residual blocks are not built (InstanceNorm only)")
        if isinstance(kernel_sizes, int):
            kernel_sizes = [kernel_sizes] * n_stages
        if isinstance(features_per_stage, int):
            features_per_stage = [features_per_stage] * n_stages
        if isinstance(n_blocks_per_stage, int):
            n_blocks_per_stage = [n_blocks_per_stage] * n_stages
        if isinstance(strides, int):
            strides = [strides] * n_stages
        if bottleneck_channels is None or isinstance(bottleneck_channels, int):
            bottleneck_channels = [bottleneck_channels] * n_stages
        assert len(kernel_sizes) == n_stages and len(n_blocks_per_stage) == n_stages
        assert len(features_per_stage) == n_stages and len(strides) == n_stages and len(bottleneck_channels) == n_stages
        if stem_channels is None:
            stem_channels = features_per_stage[0]
        self.stem = StackedConvBlocks(1, conv_op, input_channels, stem_channels, kernel_sizes[0], 1, conv_bias, norm_op,
                                      norm_op_kwargs, dropout_op, dropout_op_kwargs, nonlin, nonlin_kwargs)
        input_channels = stem_channels
        stages = []
        for s in range(n_stages):
            stages.append(StackedResidualBlocks(
                n_blocks_per_stage[s], conv_op, input_channels, features_per_stage[s], kernel_sizes[s], strides[s], conv_bias,
                norm_op, norm_op_kwargs, dropout_op, dropout_op_kwargs, nonlin, nonlin_kwargs, block=block,
                bottleneck_channels=bottleneck_channels[s], stochastic_depth_p=stochastic_depth_p,
                squeeze_excitation=squeeze_excitation,
                squeeze_excitation_reduction_ratio=squeeze_excitation_reduction_ratio))
            input_channels = features_per_stage[s]
        self.stages = nn.Sequential(*stages)
        self.output_channels = list(features_per_stage)
        self.strides = [_tup3(i, dim) for i in strides]
        self.return_skips = return_skips
        # read by the decoder (UNetDecoder.py:39-65)
        self.conv_op, self.norm_op, self.norm_op_kwargs = conv_op, norm_op, norm_op_kwargs
        self.nonlin, self.nonlin_kwargs = nonlin, nonlin_kwargs
        self.dropout_op, self.dropout_op_kwargs = dropout_op, dropout_op_kwargs
        self.conv_bias, self.kernel_sizes = conv_bias, [_tup3(k, dim) for k in kernel_sizes]

    def forward(self, x):
        x = self.stem(x)
        ret = []
        last = len(self.stages) - 1
        for i, s in enumerate(self.stages):
            x = s(x)
            if self.return_skips and i != last and SHARE_GRADS[0]:
                ops.share_grad(x)   # a skip: read by the next stage AND by the decoder (as PlainConvEncoder.forward)
            ret.append(x)
        return ret if self.return_skips else ret[-1]

    def compute_conv_feature_map_size(self, input_size):
        output = self.stem.compute_conv_feature_map_size(input_size)
        for s in range(len(self.stages)):
            output += self.stages[s].compute_conv_feature_map_size(input_size)
            input_size = [i // j for i, j in zip(input_size, self.strides[s])]
        return output


class MI355ResidualEncoderUNet(nn.Module):
    """Drop-in for dynamic_network_architectures.architectures.unet.ResidualEncoderUNet: the PlainConvUNet signature with
    n_blocks_per_stage in the place of n_conv_per_stage, plus block, bottleneck_channels and stem_channels.  fp32 only."""

    def __init__(self, input_channels: int, n_stages: int, features_per_stage: Union[int, Sequence[int]],
                 conv_op: Type = nn.Conv3d, kernel_sizes=3, strides=1, n_blocks_per_stage: Union[int, Sequence[int]] = 2,
                 num_classes: int = 2, n_conv_per_stage_decoder: Union[int, Sequence[int]] = 2, conv_bias: bool = False,
                 norm_op=None, norm_op_kwargs=None, dropout_op=None, dropout_op_kwargs=None, nonlin=None,
                 nonlin_kwargs=None, deep_supervision: bool = False, block=BasicBlockD, bottleneck_channels=None,
                 stem_channels: int = None, nonlin_first: bool = False, pool: str = 'conv'):
        super().__init__()
        if nonlin_first:
            _refuse_resenc("nonlin_first is not built (the plans set nonlin_first=False)")
        if isinstance(n_blocks_per_stage, int):
            n_blocks_per_stage = [n_blocks_per_stage] * n_stages
        if isinstance(n_conv_per_stage_decoder, int):
            n_conv_per_stage_decoder = [n_conv_per_stage_decoder] * (n_stages - 1)
        assert len(n_blocks_per_stage) == n_stages, "n_blocks_per_stage must have as many entries as we have resolution stages"
        assert len(n_conv_per_stage_decoder) == (n_stages - 1)
        self.encoder = ResidualEncoder(input_channels, n_stages, features_per_stage, conv_op, kernel_sizes, strides,
                                       n_blocks_per_stage, conv_bias, norm_op, norm_op_kwargs, dropout_op, dropout_op_kwargs,
                                       nonlin, nonlin_kwargs, block, bottleneck_channels, return_skips=True,
                                       disable_default_stem=False, stem_channels=stem_channels, pool_type=pool)
        self.decoder = UNetDecoder(self.encoder, num_classes, n_conv_per_stage_decoder, deep_supervision)

    def forward(self, x, return_last_feature=False):
        if not x.is_cuda:
            raise RuntimeError("MI355ResidualEncoderUNet runs on the MI355X only (no CPU path); move the input to cuda")
        if _conv_dim(self.encoder.conv_op) == 2:
            # the 2d configuration: [N,C,H,W] in, [N,K,h,w] logits out; inside, every tensor is the [N,C,1,H,W] view
            if x.dim() != 4:
                raise RuntimeError(f"2-D MI355ResidualEncoderUNet: input must be [N,C,H,W], got {tuple(x.shape)}")
            out = self.decoder(self.encoder(ops.to_ndhwc(x.unsqueeze(2))), return_last_feature)
            sq = lambda o: [t.squeeze(2) for t in o] if isinstance(o, (list, tuple)) else o.squeeze(2)
            if return_last_feature:
                return sq(out[0]), (out[1].squeeze(2) if out[1] is not None else None)
            return sq(out)
        return self.decoder(self.encoder(ops.to_ndhwc(x)), return_last_feature)

    def compute_conv_feature_map_size(self, input_size):
        return self.encoder.compute_conv_feature_map_size(input_size) + \
            self.decoder.compute_conv_feature_map_size(input_size)

    def parameters_in_execution_order(self):
        """Stem, stages, then per decoder level the transposed conv, the refining convs and the seg layer (see
        MI355PlainConvUNet.parameters_in_execution_order); every parameter exactly once."""
        out = list(self.encoder.stem.parameters()) + list(self.encoder.stages.parameters())
        for up, refine, head in zip(self.decoder.transpconvs, self.decoder.stages, self.decoder.seg_layers):
            out += list(up.parameters()) + list(refine.parameters()) + list(head.parameters())
        seen, uniq = set(), []
        for p in out + list(self.parameters()):
            if id(p) not in seen:
                seen.add(id(p))
                uniq.append(p)
        return uniq


ResidualEncoderUNet = MI355ResidualEncoderUNet  # the name get_network_from_plans.py:36-37 maps 'ResidualEncoderUNet' to


def init_last_bn_before_add_to_0(module):
    """The package's second init of a residual network: the norm in front of each block's add starts at zero (weight AND
    bias), so every block starts as the identity on its skip branch.  Restated from memory of the package."""
    if isinstance(module, BasicBlockD):
        nn.init.constant_(module.conv2.norm.weight, 0)
        nn.init.constant_(module.conv2.norm.bias, 0)


def set_precision(module: nn.Module, precision: str):
    """Mixed precision of the reference's autocast path (nnUNetTrainer.py:906; BASELINE cfg 4/5), MI355X style:
    "bf16" makes every fused InstanceNorm+LeakyReLU emit bf16, so every conv / transposed conv / seg head reads bf16
    activations and runs on the bf16 MFMA engine (fp32 accumulate); the 4-modality input conv converts its fp32 input to
    bf16 itself (ops.NarrowInputConv3dBf16Fn: channels zero-padded to 32), as autocast does.  Parameters, normalisation
    statistics, logits, losses, weight gradients and the optimizer stay fp32 -- bf16 has fp32's exponent range, so there
    is no GradScaler (the reference needs one for fp16, nnUNetTrainer.py:916-920)."""
    if precision not in ("fp32", "bf16"):
        raise ValueError(f"precision must be 'fp32' or 'bf16', got {precision!r}")
    if precision == "bf16" and any(isinstance(m, ConvDropoutNormReLU) and m.dim == 2 for m in module.modules()):
        # the generic bf16 engines take the (1,3,3) / (1,2,2) / (1,1,1) layers, but the 2-D network's forward misses the
        # project's bf16 bar against fp64: refused until the layer behind that is found
        raise NotImplementedError("bf16 mixed precision is not built for 2-D networks (the 2d configuration runs fp32)")
    if precision == "bf16" and any(isinstance(m, BasicBlockD) for m in module.modules()):
        raise NotImplementedError("bf16 mixed precision is not built for ResidualEncoderUNet: the residual block tail and the "
                                  "skip branch's pool are fp32 only")
    if precision == "bf16" and any(isinstance(m, BottleneckFusion) for m in module.modules()):
        raise NotImplementedError("bf16 mixed precision is not built for FinalNetv2: its bottleneck fusion block (LayerNorm, "
                                  "token linears, attention) is fp32 only")
    for m in module.modules():
        if isinstance(m, ConvDropoutNormReLU):
            m.precision = precision
    return module


PlainConvUNet = MI355PlainConvUNet  # the name get_network_from_plans.py:35 maps 'PlainConvUNet' to


class InitWeights_He(object):
    """network_initialization.py:4-12 (host-side, runs on whatever device the module lives on)."""

    def __init__(self, neg_slope=1e-2):
        self.neg_slope = neg_slope

    def __call__(self, module):
        if isinstance(module, (nn.Conv3d, nn.Conv2d, nn.ConvTranspose2d, nn.ConvTranspose3d)):
            module.weight = nn.init.kaiming_normal_(module.weight, a=self.neg_slope)
            if module.bias is not None:
                module.bias = nn.init.constant_(module.bias, 0)


class MVDDualBranchNet(nn.Module):
    """Dual-branch contract of the mutual-distillation trainer (HybridNetwork.py:1544-1571, MVDTrainer.py:895):
    forward -> (logits_list_1, logits_list_2, feat_1, feat_2); `do_ds` toggles deep supervision
    (MVDTrainer.py:802-806); with DS off single tensors are returned.  Each branch is a MI355PlainConvUNet; the
    feature map is the last decoder stage output (cf. UNetDecoder_return_last_fea, UNetDecoder.py:1012-1027)."""

    def __init__(self, branch1: MI355PlainConvUNet, branch2: MI355PlainConvUNet):
        super().__init__()
        self.branch1, self.branch2 = branch1, branch2

    @property
    def do_ds(self):
        return self.branch1.decoder.deep_supervision

    @do_ds.setter
    def do_ds(self, v):
        self.branch1.decoder.deep_supervision = v
        self.branch2.decoder.deep_supervision = v

    def forward(self, x):
        x = ops.to_ndhwc(x)
        o1, f1 = self.branch1(x, True)
        o2, f2 = self.branch2(x, True)
        return o1, o2, f1, f2

    def parameters_in_execution_order(self):
        return self.branch1.parameters_in_execution_order() + self.branch2.parameters_in_execution_order()


# ------------------------------------------------------------------------------------------------ FinalNetv2
# The fork's modality-fusing network (my_network/selfattnNet.py:838-947): one PlainConvEncoder per modality, cross-attention
# then self-attention over the bottleneck tokens, two decoders that start from the fused tokens.  Everything between the two
# bottlenecks runs in csrc/attention.hip, fp32.
class HipLayerNorm(nn.LayerNorm):
    """nn.LayerNorm(C), eps 1e-5, affine, over the last axis (mvd_layernorm_fwd / _bwd)."""

    def forward(self, x):
        return ops.LayerNormFn.apply(x, self.weight, self.bias, self.eps)


class HipLinear(nn.Linear):
    """nn.Linear on tokens; the kernels read torch's [O, C] parameter itself (mvd_linear_fwd / _bwd)."""

    def forward(self, x):
        return ops.TokenLinearFn.apply(x, self.weight, self.bias)


def _no_standalone_dropout(module, p):
    if module.training and p > 0:
        raise NotImplementedError(f"{type(module).__name__} called on its own in training mode with dropout {p}: the dropout "
                                  f"state lives in BottleneckFusion, which runs the whole block; call eval() or use p = 0")


class Cross_Attention(nn.Module):
    """UNetDecoder.py:1087-1126: same members and state_dict keys.  x1 queries x2's keys / values and the other way round."""

    def __init__(self, dim, num_heads=9, qkv_bias=False, attn_drop=0., proj_drop=0.):
        super().__init__()
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.qkv1 = HipLinear(dim, dim * 3, bias=qkv_bias)
        self.qkv2 = HipLinear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop1, self.attn_drop2 = nn.Dropout(attn_drop), nn.Dropout(attn_drop)
        self.proj1, self.proj2 = HipLinear(dim, dim), HipLinear(dim, dim)
        self.proj_drop1, self.proj_drop2 = nn.Dropout(proj_drop), nn.Dropout(proj_drop)

    def forward(self, x1, x2):
        _no_standalone_dropout(self, max(self.attn_drop1.p, self.proj_drop1.p))
        qkv1, qkv2 = self.qkv1(x1), self.qkv2(x2)
        return (self.proj1(ops.AttentionFn.apply(qkv1, qkv2, self.num_heads)),
                self.proj2(ops.AttentionFn.apply(qkv2, qkv1, self.num_heads)))


class Self_Attention(nn.Module):
    """UNetDecoder.py:1129-1154, with its quirk: forward returns the tensor BEFORE proj (:1151-1154 compute the projection
    and drop it), so `proj` exists for the state_dict only and proj_drop never acts."""

    def __init__(self, dim, num_heads=9, qkv_bias=False, attn_drop=0., proj_drop=0.):
        super().__init__()
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.qkv = HipLinear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = HipLinear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)

    def forward(self, x):
        _no_standalone_dropout(self, self.attn_drop.p)
        qkv = self.qkv(x)
        return ops.AttentionFn.apply(qkv, qkv, self.num_heads)


def _freeze(*items):
    """Members the reference's forward never reaches: autograd leaves their .grad None there, so torch's optimizers skip
    them, weight decay included, and they keep their initial values.  requires_grad = False keeps them out of
    optim.FlatParams (which takes parameters that require a gradient), of the reducer's buckets and of the fused update."""
    for it in items:
        for p in ([it] if isinstance(it, nn.Parameter) else it.parameters()):
            p.requires_grad_(False)


class BottleneckFusion(nn.Module):
    """The members FinalNetv2 keeps at its top level (selfattnNet.py:896-907) and the fused segment of its forward
    (:917-939): forward(x1, x2) -> (y1, y2) on two NDHWC bottlenecks [B, C, D, H, W] of N = D H W tokens.
    `mvd_dropout_state` (int64 {seed, t}) is the only key the reference does not have: the seed is drawn from torch's CPU
    generator here, t counts the training-mode forwards (ops.dropout_tick)."""
    num_heads = 8

    def __init__(self, hidden_size, num_tokens, attn_drop=0.1, proj_drop=0.1):
        super().__init__()
        C, N, H = int(hidden_size), int(num_tokens), self.num_heads
        lo, hi = ops.ATTN_HEAD_DIMS
        if C % H != 0:
            raise NotImplementedError(f"FinalNetv2: {C} bottleneck features do not split into {H} heads (C % 8 != 0)")
        dh = C // H
        if not (lo <= dh <= hi and dh % 4 == 0):
            raise NotImplementedError(f"FinalNetv2: head dimension {dh} (= {C} / {H}): the attention kernel takes "
                                      f"{lo}..{hi}, a multiple of 4")
        if not 1 <= N <= ops.ATTN_MAX_TOKENS:
            raise NotImplementedError(f"FinalNetv2: {N} bottleneck tokens: the attention kernel holds at most "
                                      f"{ops.ATTN_MAX_TOKENS} (patch size / strides of the plans)")
        self.hidden_size, self.num_tokens = C, N
        for i in range(1, 5):
            setattr(self, f"pos_embed{i}", nn.Parameter(torch.zeros(1, N, C)))
        self.crossattn = Cross_Attention(dim=C, num_heads=H, qkv_bias=False, attn_drop=attn_drop, proj_drop=proj_drop)
        self.selfattn1 = Self_Attention(dim=C, num_heads=H, qkv_bias=False, attn_drop=attn_drop, proj_drop=proj_drop)
        self.selfattn2 = Self_Attention(dim=C, num_heads=H, qkv_bias=False, attn_drop=attn_drop, proj_drop=proj_drop)
        self.norm1, self.norm2, self.norm3, self.norm4 = (HipLayerNorm(C) for _ in range(4))
        _freeze(self.pos_embed3, self.pos_embed4, self.selfattn1.proj, self.selfattn2.proj)
        seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64))
        self.register_buffer("mvd_dropout_state", torch.tensor([seed, 0], dtype=torch.int64))

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        # a checkpoint of the reference has no dropout state: keep this module's
        state_dict.setdefault(prefix + "mvd_dropout_state", self.mvd_dropout_state)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def fusion_parameters(self):
        """The parameters the fused segment uses, in ops.FUSION_PARAMS order."""
        ca = self.crossattn
        return [self.pos_embed1, self.pos_embed2, self.norm1.weight, self.norm1.bias, self.norm2.weight, self.norm2.bias,
                self.norm3.weight, self.norm3.bias, self.norm4.weight, self.norm4.bias, ca.qkv1.weight, ca.qkv2.weight,
                ca.proj1.weight, ca.proj1.bias, ca.proj2.weight, ca.proj2.bias, self.selfattn1.qkv.weight,
                self.selfattn2.qkv.weight]

    def fusion_parameters_in_execution_order(self):
        ca = self.crossattn
        return [self.pos_embed1, self.pos_embed2, *self.norm2.parameters(), *self.norm1.parameters(), ca.qkv1.weight,
                ca.qkv2.weight, *ca.proj1.parameters(), *ca.proj2.parameters(), *self.norm3.parameters(),
                *self.norm4.parameters(), self.selfattn1.qkv.weight, self.selfattn2.qkv.weight]

    def fuse(self, x1, x2):
        if tuple(x1.shape) != tuple(x2.shape) or x1.dim() != 5:
            raise RuntimeError(f"BottleneckFusion: two [B, C, D, H, W] bottlenecks of one shape, got {tuple(x1.shape)} and "
                               f"{tuple(x2.shape)}")
        if x1.shape[1] != self.hidden_size or x1[0, 0].numel() != self.num_tokens:
            raise RuntimeError(f"BottleneckFusion: built for {self.num_tokens} tokens of {self.hidden_size} features, got "
                               f"{x1[0, 0].numel()} of {x1.shape[1]}")
        ca = self.crossattn
        return ops.BottleneckFusionFn.apply(x1, x2, self.mvd_dropout_state, self.num_heads, ca.attn_drop1.p, ca.proj_drop1.p,
                                            self.training, self.norm1.eps, *self.fusion_parameters())

    def forward(self, x1, x2):
        return self.fuse(x1, x2)


class UNetDecoder6(UNetDecoder):
    """UNetDecoder.py:797-895: the plain decoder with the fused tokens in the place of skips[-1].  Its attention members
    (:859-868) are never used by its forward; they are kept, frozen, for state_dict parity."""

    def __init__(self, encoder, num_classes, n_conv_per_stage, deep_supervision, nonlin_first=False, hidden_size=256,
                 num_tokens=128):
        super().__init__(encoder, num_classes, n_conv_per_stage, deep_supervision, nonlin_first)
        for i in range(1, 4):
            setattr(self, f"pos_embed{i}", nn.Parameter(torch.zeros(1, num_tokens, hidden_size)))
        self.crossattn = Cross_Attention(dim=hidden_size, num_heads=8, qkv_bias=False, attn_drop=0.1, proj_drop=0.1)
        self.selfattn = Self_Attention(dim=hidden_size, num_heads=8, qkv_bias=False, attn_drop=0.1, proj_drop=0.1)
        self.hidden_size = hidden_size
        self.norm1, self.norm2 = nn.LayerNorm(hidden_size), nn.LayerNorm(hidden_size)
        _freeze(self.pos_embed1, self.pos_embed2, self.pos_embed3, self.crossattn, self.selfattn, self.norm1, self.norm2)

    def forward(self, skips, attn_skip, return_last_feature=False):
        return super().forward(list(skips[:-1]) + [attn_skip], return_last_feature)


class MI355FinalNetv2(BottleneckFusion):
    """selfattnNet.py:838-947 (constructor arguments in its order; `num_tokens` replaces the hard-coded 128 of :896-899,
    hidden_size is the bottleneck width).  forward: with deep supervision on, MVDDualBranchNet's (out1, out2, feat1, feat2),
    feat = the last decoder stage, so the dual-branch trainer's loss runs unchanged; with it off, (out1 + out2) / 2 (:943-945)."""

    def __init__(self, conv_bias, norm_op, norm_op_kwargs, dropout_op, dropout_op_kwargs, nonlin, nonlin_kwargs,
                 features_per_stage, kernel_sizes, strides, n_conv_per_stage, n_conv_per_stage_decoder,
                 input_channels: int = 2, out_channels: int = 4, n_stages: int = 5, conv_op=nn.Conv3d, pool: str = 'conv',
                 hidden_size: int = None, num_tokens: int = 128, do_ds=True):
        if input_channels != 2:
            raise NotImplementedError(f"FinalNetv2 takes exactly 2 input channels (one modality per encoder, "
                                      f"selfattnNet.py:911-914), got {input_channels}")
        if conv_op is not nn.Conv3d:
            raise NotImplementedError(f"FinalNetv2 on 2-D plans (conv_op {getattr(conv_op, '__name__', conv_op)}): only "
                                      f"the 3-D network is built")
        if isinstance(features_per_stage, int):
            features_per_stage = [features_per_stage] * n_stages
        hidden_size = features_per_stage[-1] if hidden_size is None else hidden_size
        if hidden_size != features_per_stage[-1]:
            raise NotImplementedError(f"FinalNetv2: hidden_size {hidden_size} must be the bottleneck width "
                                      f"{features_per_stage[-1]} (the tokens are the bottleneck voxels)")
        super().__init__(hidden_size, num_tokens)
        if isinstance(n_conv_per_stage, int):
            n_conv_per_stage = [n_conv_per_stage] * n_stages
        if isinstance(n_conv_per_stage_decoder, int):
            n_conv_per_stage_decoder = [n_conv_per_stage_decoder] * (n_stages - 1)
        assert len(n_conv_per_stage) == n_stages and len(n_conv_per_stage_decoder) == n_stages - 1
        enc = lambda: PlainConvEncoder(input_channels // 2, n_stages, features_per_stage, conv_op, kernel_sizes, strides,
                                       n_conv_per_stage, conv_bias, norm_op, norm_op_kwargs, dropout_op, dropout_op_kwargs,
                                       nonlin, nonlin_kwargs, return_skips=True, nonlin_first=False, pool=pool)
        self.encoder1, self.encoder2 = enc(), enc()
        dec = lambda e: UNetDecoder6(e, out_channels, n_conv_per_stage_decoder, do_ds, nonlin_first=False,
                                     hidden_size=hidden_size, num_tokens=num_tokens)
        self.decoder1, self.decoder2 = dec(self.encoder1), dec(self.encoder2)

    @property
    def do_ds(self):
        return self.decoder1.deep_supervision

    @do_ds.setter
    def do_ds(self, v):
        self.decoder1.deep_supervision = v
        self.decoder2.deep_supervision = v

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError("MI355FinalNetv2 runs on the MI355X only (no CPU path); move the input to cuda")
        if x.dim() != 5 or x.shape[1] != 2:
            raise RuntimeError(f"MI355FinalNetv2: input must be [B, 2, D, H, W] (one channel per modality), got {tuple(x.shape)}")
        # a one-channel volume is its own NDHWC form
        skips1 = self.encoder1(ops.to_ndhwc(x[:, 0:1].contiguous()))
        skips2 = self.encoder2(ops.to_ndhwc(x[:, 1:2].contiguous()))
        y1, y2 = self.fuse(skips1[-1], skips2[-1])
        if not self.do_ds:
            return ops.mean2(self.decoder1(skips1, y1), self.decoder2(skips2, y2))
        o1, f1 = self.decoder1(skips1, y1, True)
        o2, f2 = self.decoder2(skips2, y2, True)
        return o1, o2, f1, f2

    def unused_parameter_names(self):
        """state_dict keys of the parameters the forward never reaches (frozen, outside the flat buffer)."""
        return [n for n, p in self.named_parameters() if not p.requires_grad]

    def parameters_in_execution_order(self):
        """encoder1, encoder2, the fusion block in its order of use, decoder1, decoder2 (per level: transposed conv,
        refining convs, seg layer); used parameters only (see MI355PlainConvUNet.parameters_in_execution_order)."""
        out = list(self.encoder1.parameters()) + list(self.encoder2.parameters()) + self.fusion_parameters_in_execution_order()
        for d in (self.decoder1, self.decoder2):
            for up, refine, head in zip(d.transpconvs, d.stages, d.seg_layers):
                out += list(up.parameters()) + list(refine.parameters()) + list(head.parameters())
        return out


def finalnet_num_tokens(patch_size, strides):
    """Bottleneck voxels of a patch: the token count N (128 for the reference's plan, selfattnNet.py:896)."""
    n = 1
    for axis, size in enumerate(patch_size):
        red = int(np.prod([_tup3(s, len(patch_size))[axis] for s in strides]))
        if size % red:
            raise NotImplementedError(f"patch size {list(patch_size)} is not divisible by the strides' product along axis {axis}")
        n *= size // red
    return n


def get_finalnet_from_plans(plans_manager, dataset_json, configuration_manager, num_input_channels, deep_supervision=True):
    """get_network_from_plans.py:94-205 (get_dual_network_from_plans) with FinalNetv2 selected; InitWeights_He touches the
    convolutions only (network_initialization.py:4-12), the attention members keep torch's own initialisation."""
    num_stages = len(configuration_manager.conv_kernel_sizes)
    dim = len(configuration_manager.conv_kernel_sizes[0])
    if dim != 3:
        raise NotImplementedError(f"FinalNetv2 on {dim}-D plans: only the 3-D network is built")
    label_manager = plans_manager.get_label_manager(dataset_json)
    features = [min(configuration_manager.UNet_base_num_features * 2 ** i, configuration_manager.unet_max_num_features)
                for i in range(num_stages)]
    model = MI355FinalNetv2(
        conv_bias=True, norm_op=nn.InstanceNorm3d, norm_op_kwargs={'eps': 1e-5, 'affine': True}, dropout_op=None,
        dropout_op_kwargs=None, nonlin=nn.LeakyReLU, nonlin_kwargs={'inplace': True}, features_per_stage=features,
        kernel_sizes=configuration_manager.conv_kernel_sizes, strides=configuration_manager.pool_op_kernel_sizes,
        n_conv_per_stage=configuration_manager.n_conv_per_stage_encoder,
        n_conv_per_stage_decoder=configuration_manager.n_conv_per_stage_decoder, input_channels=num_input_channels,
        out_channels=label_manager.num_segmentation_heads, n_stages=num_stages, conv_op=nn.Conv3d,
        hidden_size=features[-1],
        num_tokens=finalnet_num_tokens(configuration_manager.patch_size, configuration_manager.pool_op_kernel_sizes),
        do_ds=deep_supervision)
    model.apply(InitWeights_He(1e-2))
    return model
