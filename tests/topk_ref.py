"""fp64 torch restatement of the top-k cross entropy and the loss trainer variants of DESIGN 29 that the device path is
tested against (test_topk_ref_host.py pins it to the reference's own TopKLoss through tests/golden/topk_loss.npz, the GPU
tests compare the kernels with it).

TopKLoss (training/loss/robust_ce_loss.py:19-32): ce = cross_entropy(reduction='none', ignore_index, label_smoothing) over
all n = N * V voxels (an ignored voxel counts, with the value 0), k = int(n * k_percent / 100), loss = mean of the k largest.
Selection by sort.  Tie rule (the project's decision; torch.topk leaves the choice among ties open): with t the k-th
largest value, every element above t has weight 1 / k and the cnt_eq elements equal to t share the remaining
(k - cnt_gt) / k equally.  The loss is torch's whichever elements it picks; the gradient is a convex combination of the
gradients torch could return.  DC_and_topk_loss and the Dice-only / CE-only compositions follow upstream nnU-Net 2.1.1
(compound_losses.py is missing from the fork: parity unpinned)."""
import numpy as np
import torch
import torch.nn.functional as F

from region_loss_ref import dc_and_bce_labelmap, dc_and_ce_masked, soft_dice


def topk_count(n, k_percent=10):
    return int(np.int64(n) * k_percent / 100)


def ce_per_voxel(z, target, ignore_index=-100, label_smoothing=0.0):
    """[N, *spatial] fp64; target [N,1,*spatial] float labels"""
    return F.cross_entropy(z.double(), target[:, 0].long(), ignore_index=ignore_index, reduction='none',
                           label_smoothing=label_smoothing)


def select(ce, k):
    """ce: any shape, fp64, no grad needed -> (t, cnt_gt, cnt_eq, weights like ce) for the k-th largest by sort"""
    flat = ce.detach().reshape(-1)
    if not 1 <= k <= flat.numel():
        raise ValueError(f"k = {k} of {flat.numel()} values")
    t = torch.sort(flat, descending=True).values[k - 1]
    gt, eq = ce.detach() > t, ce.detach() == t
    cnt_gt, cnt_eq = int(gt.sum()), int(eq.sum())
    w = gt.double() / k + eq.double() * ((k - cnt_gt) / cnt_eq / k)
    return t, cnt_gt, cnt_eq, w


def topk_loss(z, target, k_percent=10, ignore_index=-100, label_smoothing=0.0, parts=False):
    """differentiable in z: sum_v w_v ce_v with the weights of select() held constant = (S_gt + (k - cnt_gt) t) / k"""
    ce = ce_per_voxel(z, target, ignore_index, label_smoothing)
    k = topk_count(ce.numel(), k_percent)
    if k < 1:
        raise ValueError("k == 0: the reference's mean over an empty selection is NaN")
    t, cnt_gt, cnt_eq, w = select(ce, k)
    loss = (w * ce).sum()
    return (loss, ce.detach(), t, cnt_gt, cnt_eq, w) if parts else loss


def dc_and_topk(z, target, ignore_label=None, batch_dice=False, do_bg=False, smooth=1e-5, w_ce=1.0, w_dice=1.0, k_percent=10,
                label_smoothing=0.0, dice_z=None, dice_target=None):
    """DC_and_topk_loss: ignore_label -> ce ignore_index; Dice masked by target != ignore_label, ignored voxels relabelled 0.
    dice_z / dice_target: another sample set for the Dice half (the all-gathered batch of DDP batch-dice)."""
    zd = (z if dice_z is None else dice_z).double()
    td = target if dice_target is None else dice_target
    lab = td[:, 0].long()
    if ignore_label is None:
        m = None
    else:
        m = (td != ignore_label).double()
        lab = torch.where(lab == ignore_label, torch.zeros_like(lab), lab)
    onehot = F.one_hot(lab, zd.shape[1]).movedim(-1, 1).double()
    dice = soft_dice(torch.softmax(zd, 1), onehot, m, batch_dice, do_bg, smooth)
    ce = topk_loss(z, target, k_percent, -100 if ignore_label is None else ignore_label, label_smoothing)
    return w_ce * ce + w_dice * dice


def dice_only(z, target, batch_dice=False, do_bg=False, smooth=1e-5):
    """MemoryEfficientSoftDiceLoss over softmax, no mask"""
    onehot = F.one_hot(target[:, 0].long(), z.shape[1]).movedim(-1, 1).double()
    return soft_dice(torch.softmax(z.double(), 1), onehot, None, batch_dice, do_bg, smooth)


def ce_only(z, target, ignore_index=-100):
    """RobustCrossEntropyLoss; with an ignore label the mean over the valid voxels, 0 when there is none (the device's
    choice where torch's 0 / 0 is NaN)"""
    if ignore_index == -100:
        return F.cross_entropy(z.double(), target[:, 0].long())
    return dc_and_ce_masked(z, target, ignore_index, w_ce=1.0, w_dice=0.0)


def variant_weights(n_levels):
    """variants/loss/*.py: 1 / 2^i over all levels, normalised; no zeroed tail"""
    w = np.array([1 / (2 ** i) for i in range(n_levels)])
    return w / w.sum()


def variant_level_loss(name, batch_dice=False, ignore_label=None, regions=None):
    """the per-level loss each of the six trainers' _build_loss composes, as fn(z, target) in fp64"""
    ign = -100 if ignore_label is None else ignore_label
    if name == "nnUNetTrainerDiceLossMI355":
        if ignore_label is not None:
            raise NotImplementedError("the reference's Dice-only loss has no mask")
        if regions is not None:
            return lambda z, t: dc_and_bce_labelmap(z, t, regions, None, batch_dice=batch_dice, do_bg=True, smooth=1e-5,
                                                    w_ce=0.0, w_dice=1.0)
        return lambda z, t: dice_only(z, t, batch_dice, False, 1e-5)
    if name == "nnUNetTrainerDiceCELoss_noSmoothMI355":
        if regions is not None:
            return lambda z, t: dc_and_bce_labelmap(z, t, regions, ignore_label, batch_dice=batch_dice, do_bg=True, smooth=0.0)
        return lambda z, t: dc_and_ce_masked(z, t, ignore_label, batch_dice=batch_dice, do_bg=False, smooth=0.0)
    assert regions is None, 'regions not supported by this trainer'
    if name == "nnUNetTrainerCELossMI355":
        return lambda z, t: ce_only(z, t, ign)
    if name == "nnUNetTrainerTopk10LossMI355":
        return lambda z, t: topk_loss(z, t, 10, ign, 0.0)
    if name == "nnUNetTrainerTopk10LossLS01MI355":
        return lambda z, t: topk_loss(z, t, 10, ign, 0.1)
    if name == "nnUNetTrainerDiceTopK10LossMI355":
        return lambda z, t: dc_and_topk(z, t, ignore_label, batch_dice=batch_dice, do_bg=False, smooth=1e-5, k_percent=10)
    raise KeyError(name)


def variant_loss(name, outputs, targets, **kw):
    fn = variant_level_loss(name, **kw)
    return sum(float(w) * fn(o, t) for w, o, t in zip(variant_weights(len(outputs)), outputs, targets))


VARIANTS = ("nnUNetTrainerDiceLossMI355", "nnUNetTrainerDiceCELoss_noSmoothMI355", "nnUNetTrainerCELossMI355",
            "nnUNetTrainerTopk10LossMI355", "nnUNetTrainerTopk10LossLS01MI355", "nnUNetTrainerDiceTopK10LossMI355")
