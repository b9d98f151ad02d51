"""Host-side mirrors of the reference's loss classes for the hot path; every evaluation is a HIP kernel.

Class / function names and constructor arguments follow the reference so that a trainer's `_build_loss`
(nnUNet/nnunetv2/training/nnUNetTrainer/nnUNetTrainer.py:351-375) reads the same:
RobustCrossEntropyLoss (training/loss/robust_ce_loss.py:6-16), MemoryEfficientSoftDiceLoss / DC_and_CE_loss /
DeepSupervisionWrapper (files missing from the fork: upstream nnU-Net 2.1.1 semantics),
distill_kl / l2_loss (training/loss/other_loss.py:51-78), soft_erode / soft_dilate / soft_open / soft_skel
(training/loss/soft_skeleton.py:6-37), clDice formula (training/metrics/clDice_metric.py:7-36).
"""
import numpy as np
import torch
from torch import nn

from . import ops


class _FusedDCCE(nn.Module):
    """One level of w_ce*CE + w_dice*Dice, evaluated by mvd_dcce_{fwd,finalize,bwd}."""

    def __init__(self, batch_dice=False, do_bg=False, smooth=1e-5, ddp=False, weight_ce=1.0, weight_dice=1.0):
        super().__init__()
        self.batch_dice, self.do_bg, self.smooth, self.ddp = batch_dice, do_bg, smooth, ddp
        self.weight_ce, self.weight_dice = weight_ce, weight_dice

    def _cfg(self):
        return (self.batch_dice, self.do_bg, self.smooth, self.weight_ce, self.weight_dice)

    def _gather(self):
        if not (self.ddp and self.batch_dice):
            return None
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return None
        from .parallel import gather_dice_stats
        return gather_dice_stats

    def _fused_apply(self, weights, targets, outputs):
        """All levels as one autograd node; the label modes of DESIGN 17 override this.  (Not named `_apply`: that is
        nn.Module's own method behind .to() / .float() / .cuda().)"""
        return ops.DeepSupervisedDCCEFn.apply(weights, self._cfg(), self._gather(), targets, *outputs)

    def forward(self, net_output, target):
        return self._fused_apply([1.0], [target], [net_output])


class RobustCrossEntropyLoss(_FusedDCCE):
    """robust_ce_loss.py:6-16: float target with a singleton channel, mean over voxels.  ignore_index other than torch's
    default -100 (nnUNetTrainerCELoss.py:10-11 passes the ignore label) takes the masked kernels of DESIGN 17 with
    weight_dice = 0: the mean over the valid voxels, and 0 where torch's 0 / 0 gives NaN (no voxel valid)."""

    def __init__(self, weight=None, ignore_index: int = -100):
        if weight is not None:
            raise NotImplementedError("RobustCrossEntropyLoss: class weights are not built (weight=None at every call site)")
        super().__init__(weight_ce=1.0, weight_dice=0.0)
        self.ignore_index = int(ignore_index)

    def _fused_apply(self, weights, targets, outputs):
        if self.ignore_index == -100:
            return super()._fused_apply(weights, targets, outputs)
        return ops.DeepSupervisedMaskedFn.apply(weights, ('ce', *self._cfg(), self.ignore_index), None, targets, *outputs)


class MemoryEfficientSoftDiceLoss(_FusedDCCE):
    """App. B; apply_nonlin is always softmax over dim 1 on this path (nnUNetTrainer.py:359-361).  The sigmoid form of
    nnUNetTrainerDiceLoss's region case is DC_and_BCE_loss with weight_ce = 0 (trainer.nnUNetTrainerDiceLossMI355)."""

    def __init__(self, apply_nonlin=None, batch_dice: bool = False, do_bg: bool = True, smooth: float = 1.,
                 ddp: bool = True):
        super().__init__(batch_dice, do_bg, smooth, ddp, weight_ce=0.0, weight_dice=1.0)


class DC_and_CE_loss(_FusedDCCE):
    def __init__(self, soft_dice_kwargs, ce_kwargs, weight_ce=1, weight_dice=1, ignore_label=None,
                 dice_class=MemoryEfficientSoftDiceLoss):
        if ce_kwargs:
            raise NotImplementedError("ce_kwargs is {} at the reference call site (nnUNetTrainer.py:360)")
        kw = dict(batch_dice=False, do_bg=True, smooth=1., ddp=True)
        kw.update(soft_dice_kwargs)
        super().__init__(kw['batch_dice'], kw['do_bg'], kw['smooth'], kw['ddp'], float(weight_ce), float(weight_dice))
        self.ignore_label = None if ignore_label is None else int(ignore_label)

    def _fused_apply(self, weights, targets, outputs):
        if self.ignore_label is None:
            return super()._fused_apply(weights, targets, outputs)
        # upstream 2.1.1 DC_and_CE_loss(ignore_label=L): mask = target != L for both terms (parity unpinned)
        return ops.DeepSupervisedMaskedFn.apply(weights, ('ce', *self._cfg(), self.ignore_label), self._gather(), targets,
                                                *outputs)


class DC_and_BCE_loss(_FusedDCCE):
    """Upstream 2.1.1 DC_and_BCE_loss for region-based training (nnUNetTrainer.py:352-357): sigmoid heads, BCE-with-logits
    + soft Dice over the R regions; with use_ignore_label both terms are masked and the BCE sum is divided by the number
    of valid VOXELS (upstream's own normalisation).  The class is missing from the fork: parity unpinned, semantics pinned
    by tests/region_loss_ref.py.
    Targets: `regions` given (a list of labels / label tuples, one per head) -> the float label map [N,1,...] the feed
    produces, converted per voxel through a label table (`ignore_label` marks the ignored voxels); `regions` absent -> the
    reference's binary planes [N,R(+1),...] from ConvertSegmentationToRegionsTransform, the ignore plane last."""

    def __init__(self, bce_kwargs, soft_dice_kwargs, weight_ce=1, weight_dice=1, use_ignore_label: bool = False,
                 dice_class=MemoryEfficientSoftDiceLoss, regions=None, ignore_label=None):
        if bce_kwargs:
            raise NotImplementedError("bce_kwargs is {} at the reference call site (nnUNetTrainer.py:353)")
        kw = dict(batch_dice=False, do_bg=True, smooth=1., ddp=True)
        kw.update(soft_dice_kwargs)
        super().__init__(kw['batch_dice'], kw['do_bg'], kw['smooth'], kw['ddp'], float(weight_ce), float(weight_dice))
        self.use_ignore_label = bool(use_ignore_label)
        if regions is not None:
            if self.use_ignore_label != (ignore_label is not None):
                raise ValueError("label-map targets: use_ignore_label and ignore_label must be given together")
            if len(regions) > ops.REGION_KMAX:
                raise NotImplementedError(f"{len(regions)} regions: the fused loss kernels hold at most {ops.REGION_KMAX}")
            self._extra = (0, ops.region_label_table(regions, ignore_label), self.use_ignore_label)
        else:
            if ignore_label is not None:
                raise ValueError("plane targets carry the ignore label as their last plane; ignore_label needs `regions`")
            self._extra = (2 if self.use_ignore_label else 1, None, self.use_ignore_label)

    def _fused_apply(self, weights, targets, outputs):
        return ops.DeepSupervisedMaskedFn.apply(weights, ('bce', *self._cfg(), self._extra), self._gather(), targets,
                                                *outputs)


class TopKLoss(_FusedDCCE):
    """robust_ce_loss.py:19-32: per-voxel cross entropy (reduction='none': ignored voxels count with the value 0), then
    the mean of its largest int(num_voxels * k / 100) values, selected exactly on the device.  Elements that
    tie with the threshold share the remaining weight equally; k == 0 (fewer than 100 / k voxels) is refused."""

    def __init__(self, weight=None, ignore_index: int = -100, k: float = 10, label_smoothing: float = 0):
        if weight is not None:
            raise NotImplementedError("TopKLoss: class weights are not built (weight=None at every reference call site)")
        if not 0 < k <= 100:
            raise ValueError(f"TopKLoss: k is a percentage in (0, 100], got {k}")
        if not 0 <= label_smoothing <= 1:
            raise ValueError(f"TopKLoss: label_smoothing must lie in [0, 1], got {label_smoothing}")
        super().__init__(weight_ce=1.0, weight_dice=0.0)
        self.k, self.ignore_index, self.label_smoothing = k, int(ignore_index), float(label_smoothing)

    def _fused_apply(self, weights, targets, outputs):
        return ops.DeepSupervisedTopKFn.apply(weights, (self.k, self.label_smoothing, self.ignore_index, None), None, targets,
                                              *outputs)


class DC_and_topk_loss(_FusedDCCE):
    """Upstream 2.1.1 DC_and_topk_loss (the class is missing from the fork: parity unpinned, semantics pinned by
    tests/topk_ref.py): weight_ce * TopKLoss(**ce_kwargs) + weight_dice * soft Dice over softmax.  ignore_label goes into
    ce_kwargs['ignore_index'], masks the Dice by target != ignore_label and relabels the ignored voxels 0 for it."""

    def __init__(self, soft_dice_kwargs, ce_kwargs, weight_ce=1, weight_dice=1, ignore_label=None):
        kw = dict(batch_dice=False, do_bg=True, smooth=1., ddp=True)
        kw.update(soft_dice_kwargs)
        super().__init__(kw['batch_dice'], kw['do_bg'], kw['smooth'], kw['ddp'], float(weight_ce), float(weight_dice))
        ce_kwargs = dict(ce_kwargs)
        if ignore_label is not None:
            ce_kwargs['ignore_index'] = int(ignore_label)
        self.ce = TopKLoss(**ce_kwargs)
        self.ignore_label = None if ignore_label is None else int(ignore_label)

    def _fused_apply(self, weights, targets, outputs):
        ce = self.ce
        return ops.DeepSupervisedTopKFn.apply(weights, (ce.k, ce.label_smoothing, ce.ignore_index,
                                                        (*self._cfg(), self.ignore_label)), self._gather(), targets, *outputs)


class DeepSupervisionWrapper(nn.Module):
    """sum_i w_i * loss(x_i, t_i) (nnUNetTrainer.py:374) as ONE autograd node over all levels."""

    def __init__(self, loss: _FusedDCCE, weight_factors=None):
        super().__init__()
        if not isinstance(loss, _FusedDCCE):
            raise TypeError("DeepSupervisionWrapper wraps the fused DC/CE losses of this package")
        self.loss = loss
        self.weight_factors = weight_factors

    def forward(self, net_output, target):
        assert isinstance(net_output, (tuple, list)) and isinstance(target, (tuple, list))
        w = [1.0] * len(net_output) if self.weight_factors is None else [float(i) for i in self.weight_factors]
        return self.loss._fused_apply(w, list(target), list(net_output))


def ds_weights(n_scales):
    """nnUNetTrainer.py:366-372."""
    w = np.array([1 / (2 ** i) for i in range(n_scales)])
    w[-1] = 0
    return w / w.sum()


# ------------------------------------------------------------------------------------------------ distillation
def distill_kl(y_s, y_t, T=1):
    """other_loss.py:51-64."""
    pad = y_s.shape[1] == 1
    return ops.DistillKLFn.apply(y_s, y_t, T, 1e-40, pad)


def l2_loss(input, target, channel_wise=False, T=1):
    """other_loss.py:67-78: channel_wise=True is the feature-distillation KL used on the path, channel_wise=False the
    plain mean squared difference (:77-78)."""
    if not channel_wise:
        return ops.MseFn.apply(ops.widen(input), ops.widen(target))
    return ops.DistillKLFn.apply(input, target, T, 0.0, False)


def kl_loss_compute1(vessel1, vessel2, T=1):
    """Unpinned wrapper (imported at MVDTrainer.py:74, defined nowhere): KL between the branches' vessel maps."""
    return distill_kl(vessel1[:, None], vessel2[:, None], T)


# ------------------------------------------------------------------------------------------------ soft skeleton
def soft_erode(img):
    return ops.SoftErodeFn.apply(img)


def soft_dilate(img):
    return ops.SoftDilateFn.apply(img)


def soft_open(img):
    return soft_dilate(soft_erode(img))


def soft_skel(img, iter_):
    """soft_skeleton.py:29-37: one fused launch for the step in front of the loop and one per iteration
    (erode -> erode -> dilate -> skeleton update walk an LDS tile; csrc/topo.hip::k_skel_iter_fwd)."""
    skel = ops.SkelInitFn.apply(img)
    for _ in range(iter_):
        img, skel = ops.SkelIterFn.apply(img, skel)
    return skel


def soft_skel_unfused(img, iter_):
    """The same chain one primitive per launch (the round-1 path; kept as the cross-check of the fused kernels)."""
    img1 = soft_open(img)
    skel = ops.SkelUpdateFn.apply(img, img1, None)
    for _ in range(iter_):
        img = soft_erode(img)
        img1 = soft_open(img)
        skel = ops.SkelUpdateFn.apply(img, img1, skel)
    return skel


def soft_cldice(pred, target, iter_=3, smooth=1.0):
    """1 - clDice on soft skeletons (see oracle/loss_oracle.py::soft_cldice for the unpinned choices)."""
    skel_pred = soft_skel(pred, iter_)
    with torch.no_grad():
        skel_true = soft_skel(target, iter_)
    return ops.ClDiceFn.apply(skel_pred, target, skel_true, pred, smooth)


# ------------------------------------------------------------------------------------ persistence topological loss (2-D)
class LevelSetLayer2D(nn.Module):
    """LevelSetLayer2D of the vendored TopologyLayer (nn/levelset.py:137-163) on the Freudenthal triangulation
    (init_freudenthal_2d, :64-93).  size = (width, height) as in the reference; forward(f [H,W]) returns
    (dgms, issublevel) with dgms = (dgm0 [V,2], dgm1 [T,2]) DEVICE tensors (dgm0 alone for maxdim 0), differentiable
    (ops.LevelSetDiagram2DFn).  `alg` is accepted and ignored: 'hom', 'hom2' and 'cohom' give the same diagram."""

    def __init__(self, size, maxdim=1, sublevel=True, complex="freudenthal", alg='hom'):
        super().__init__()
        if complex != "freudenthal":
            raise NotImplementedError(f"LevelSetLayer2D(complex='{complex}'): only the 'freudenthal' triangulation is built; "
                                      f"'grid' is no triangulated disc and 'delaunay' has no fixed diagonals, so the "
                                      f"dual-graph pairing of dimension 1 does not apply to them")
        if maxdim not in (0, 1):
            raise ValueError("LevelSetLayer2D: maxdim must be 0 or 1")
        self.size, self.maxdim, self.sublevel, self.alg = tuple(int(s) for s in size), int(maxdim), bool(sublevel), alg

    def forward(self, f):
        width, height = self.size
        if f.numel() != width * height:
            raise RuntimeError(f"LevelSetLayer2D(size={self.size}): the input has {f.numel()} values")
        dgms = ops.LevelSetDiagram2DFn.apply(f.reshape(1, 1, height, width), [0], self.sublevel, self.maxdim)
        return tuple(d[0] for d in dgms), self.sublevel


class TopKBarcodeLengths(nn.Module):
    """nn/features.py:128-150: the k longest bars of dimension `dim` of (dgms, issublevel), end - start with the
    sub-/super-level swap of get_start_end, infinite and NaN lengths 0, descending, truncated or zero padded to k.
    dgms[dim] may be one diagram [n,2] (-> [k]) or a batch [P,n,2] (-> [P,k]); selected on the device."""

    def __init__(self, dim, k):
        super().__init__()
        if not 1 <= int(k) <= ops.LS2D_MAX_K:
            raise ValueError(f"TopKBarcodeLengths: k must be in 1..{ops.LS2D_MAX_K} (got {k})")
        self.dim, self.k = int(dim), int(k)

    def forward(self, dgminfo):
        dgms, issublevel = dgminfo
        dgm = dgms[self.dim]
        if dgm.dim() == 2:
            return ops.TopKBarLengths2DFn.apply(dgm[None], self.dim, self.k, issublevel)[0]
        return ops.TopKBarLengths2DFn.apply(dgm, self.dim, self.k, issublevel)


class TopoLoss(nn.Module):
    """TopoLoss of the reference (training/loss/Topo_Loss.py:16-85): per sample and class of interest the super-level
    diagram of y_pred[b, idx+1], its max_k longest bars per dimension squared, the first beta0 / beta1 of them (topo_label
    [B,C,2], read on the device) signed -1 and the rest +1, the mean over the batch, the sum over idx;
    topo_weight * l_topo / len(idx) + sqdiff_weight * MSE(y_raw, y_pred).  All samples and classes are ONE batch of
    persistence problems (one host round trip per forward, ops.TopoLossFn).  y_raw = None leaves the MSE term out (the
    reference defines it for fine-tuning against a frozen first network)."""

    def __init__(self, img_size, topo_weight=1, sqdiff_weight=10, max_k=20):
        super().__init__()
        if not 1 <= int(max_k) <= ops.LS2D_MAX_K:
            raise ValueError(f"TopoLoss: max_k must be in 1..{ops.LS2D_MAX_K} (got {max_k})")
        self.img_size = tuple(int(s) for s in img_size)
        self.sqdiff_weight, self.topo_weight, self.max_k = sqdiff_weight, topo_weight, int(max_k)

    def forward(self, y_pred, y_raw, topo_label, idx=[1]):
        width, height = self.img_size
        if tuple(y_pred.shape[2:]) != (height, width):
            raise RuntimeError(f"TopoLoss(img_size={self.img_size}) takes [B,C,{height},{width}] probabilities, got "
                               f"{tuple(y_pred.shape)}")
        l = self.topo_weight * ops.TopoLossFn.apply(y_pred, topo_label, list(idx), self.max_k) / len(idx)
        if y_raw is not None:
            l = l + self.sqdiff_weight * ops.MseFn.apply(y_raw, y_pred)
        return l


def betti_topo_label(target, num_classes):
    """The topo_label TopoLoss expects, from a label map [B,1,H,W] / [B,H,W]: int32 [B, num_classes, 2] = (beta0, beta1)
    of every class's binary mask on the Freudenthal triangulation -- components joined along the grid axes and the
    (+1,+1) diagonal, and the holes they enclose -- counted as the bars of non-zero length of the mask's super-level
    diagram, the essential component included (an empty mask has none)."""
    return ops.ls2d_betti_numbers(target, num_classes)


# ------------------------------------------------------------------------ 3-D cubical persistence loss (dual-branch trainer)
class CubicalComplex3D(nn.Module):
    """CubicalComplex(dim=3, superlevel=False) of MVDTrainer.py:94-97 restricted to one homology dimension: forward(field
    [N,D,H,W] fp32) returns per sample the differentiable diagram [n,2] of (birth, death) rows of dimension `dim`, gathered
    from the field (ops.CubicalDiagram3DFn).  Voxels are closed top-dimensional cells; bars of zero length and essential
    bars are dropped.  dim 0 and dim 2 (the trainer's topo_feat_d) reduce to union-find; dim 1 is not built."""

    def __init__(self, dim=2):
        super().__init__()
        self.dim = ops.cub3d_check_dim(dim)

    def forward(self, field):
        dgm, offsets = ops.CubicalDiagram3DFn.apply(field, self.dim)
        return list(torch.split(dgm, [int(c) for c in (offsets[1:] - offsets[:-1])]))


class CubicalWassersteinLoss(nn.Module):
    """The topological term of MVDTrainer.py:907-925 / training/loss/TopoLoss.py as one fused path: the q-Wasserstein
    distance (L-inf ground metric, the diagonal allowed) between the dimension-`dim` cubical diagram of field [N,D,H,W] and
    that of the binary target mask [N,D,H,W], averaged over the batch.  `last_m` holds the target's point counts (device)."""

    def __init__(self, dim=2, q=2):
        super().__init__()
        self.dim = ops.cub3d_check_dim(dim)
        if not float(q) >= 1.0:
            raise ValueError(f"CubicalWassersteinLoss: q must be >= 1 (got {q})")
        self.q = float(q)
        self.last_m = None

    def forward(self, field, target_mask):
        if bool(((target_mask != 0) & (target_mask != 1)).any()):
            raise ValueError("CubicalWassersteinLoss: the target must be a binary mask (its diagram is m copies of (0, 1))")
        loss, self.last_m = ops.CubicalWassersteinFn.apply(field, target_mask, self.dim, self.q)
        return loss
