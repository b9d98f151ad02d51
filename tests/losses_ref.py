"""TEST INFRASTRUCTURE -- float64 evaluation of the plain (label, no ignore) losses for tests/test_gpu_losses.py and
tests/test_losses_ref_host.py.  Everything the oracle (oracle/loss_oracle.py) states is evaluated THROUGH the oracle on
.double() inputs with autograd; plain torch fp64 expressions stand in only where the oracle has no function (softmax
channel, clDice formula on given skeletons, argmax counts, the single-process form of the DDP batch-dice gather)."""
import numpy as np
import torch

from oracle import loss_oracle as LO


def grads_of(loss, inputs):
    """(loss.detach(), [d loss / d input or None])"""
    gs = torch.autograd.grad(loss, [t for t in inputs if t.requires_grad], allow_unused=True)
    it = iter(gs)
    return loss.detach(), [next(it) if t.requires_grad else None for t in inputs]


def leaf(t, grad=True):
    return t.detach().double().requires_grad_(grad)


def dc_ce(z, target, batch_dice, do_bg, smooth, w_ce=1.0, w_dice=1.0, scale=1.0):
    """oracle DC_and_CE_loss in fp64 on the float label map `target` [N,1,...]; gradient of scale * loss."""
    zz = leaf(z)
    fn = LO.DC_and_CE_loss({'batch_dice': batch_dice, 'smooth': smooth, 'do_bg': do_bg, 'ddp': False}, {},
                           weight_ce=w_ce, weight_dice=w_dice)
    l = fn(zz, target)
    _, g = grads_of(l * scale, [zz])
    return l.detach(), g


def ce_only(z, target):
    zz = leaf(z)
    return grads_of(LO.RobustCrossEntropyLoss()(zz, target), [zz])


def dice_only(z, target, **kw):
    zz = leaf(z)
    return grads_of(LO.MemoryEfficientSoftDiceLoss(apply_nonlin=LO.softmax_helper_dim1, **kw)(zz, target), [zz])


def deep_supervised(zs, ts, weights, batch_dice, do_bg, smooth):
    zz = [leaf(z) for z in zs]
    base = LO.DC_and_CE_loss({'batch_dice': batch_dice, 'smooth': smooth, 'do_bg': do_bg, 'ddp': False}, {})
    return grads_of(LO.DeepSupervisionWrapper(base, weights)(zz, ts), zz)


def dc_ce_gathered(z, target, z_other, target_other, do_bg, smooth, w_ce, w_dice, mult):
    """DDP batch-dice seen from one rank: loss = w_ce * CE(local) + w_dice * Dice_batch(other ++ local); the local
    gradient is d(w_ce * CE)/dz + mult * d(w_dice * Dice)/dz (AllGatherGrad.backward sums the identical gradients of
    `mult` ranks).  Returns (loss, grad, (ce, dice, d ce/dz, d dice/dz)) -- the parts feed the finite-difference check."""
    zz = leaf(z)
    ce = LO.RobustCrossEntropyLoss()(zz, target)
    dice_fn = LO.MemoryEfficientSoftDiceLoss(apply_nonlin=LO.softmax_helper_dim1, batch_dice=True, do_bg=do_bg, smooth=smooth)
    dice = dice_fn(torch.cat([z_other.double(), zz]), torch.cat([target_other, target]))
    gce, = torch.autograd.grad(ce, zz, retain_graph=True)
    gdc, = torch.autograd.grad(dice, zz)
    loss = (w_ce * ce + w_dice * dice).detach()
    return loss, [w_ce * gce + mult * w_dice * gdc], (ce.detach(), dice.detach(), gce, gdc)


def kl(ys, yt, T, which="distill", need=(True, True)):
    """oracle distill_kl (pads the 1-channel branch itself) / l2_loss(channel_wise=True) in fp64"""
    a, b = leaf(ys, need[0]), leaf(yt, need[1])
    l = LO.distill_kl(a, b, T) if which == "distill" else LO.l2_loss(a, b, True, T)
    return grads_of(l, [a, b])


def mse(a, b, need=(True, True)):
    x, y = leaf(a, need[0]), leaf(b, need[1])
    return grads_of(LO.l2_loss(x, y, False), [x, y])


def cldice_tail(skel_pred, target, skel_true, pred, smooth):
    """the formula of loss_oracle.soft_cldice on GIVEN skeletons"""
    sp, pr = leaf(skel_pred), leaf(pred)
    tg, st = target.double(), skel_true.double()
    tprec = (torch.sum(sp * tg) + smooth) / (torch.sum(sp) + smooth)
    tsens = (torch.sum(st * pr) + smooth) / (torch.sum(st) + smooth)
    return grads_of(1.0 - 2.0 * (tprec * tsens) / (tprec + tsens), [sp, pr])


def argmax_counts(logits, target):
    """int64 [K,3] = (tp, fp, fn) per class, background included; numpy.argmax: the first maximum wins"""
    x = logits.numpy()
    K = x.shape[1]
    pred = x.argmax(1).reshape(-1)
    y = target.numpy().reshape(-1).astype(np.int64)
    out = np.zeros((K, 3), dtype=np.int64)
    for k in range(K):
        p, t = pred == k, y == k
        out[k] = (np.count_nonzero(p & t), np.count_nonzero(p & ~t), np.count_nonzero(~p & t))
    return out
