"""fp64 torch restatement of the label modes of DESIGN 17 that the device path is tested against (test_region_loss_host.py
pins it, the GPU tests compare the kernels with it).  Semantics: upstream nnU-Net 2.1.1 `DC_and_BCE_loss` and
`DC_and_CE_loss(ignore_label=)` with `MemoryEfficientSoftDiceLoss` (classes missing from the fork: parity unpinned), built
on torch.nn.functional.binary_cross_entropy_with_logits and cross_entropy(ignore_index=).

Notation: z logits [N,R,...]; y planes (0/1); m = 1 where the voxel is not ignored; s = smooth."""
import numpy as np
import torch
import torch.nn.functional as F


def seg_to_regions(seg, regions, ignore_label=None):
    """numpy model of ConvertSegmentationToRegionsTransform: seg [N,1,...] -> [N,R(+1),...] in seg's dtype, the ignore
    label's plane last."""
    regs = list(regions) + ([ignore_label] if ignore_label is not None else [])
    out = np.zeros((seg.shape[0], len(regs), *seg.shape[2:]), dtype=seg.dtype)
    for r, labels in enumerate(regs):
        for l in (labels if isinstance(labels, (list, tuple)) else (labels,)):
            out[:, r][seg[:, 0] == l] = 1
    return out


def label_table(regions, ignore_label=None):
    """host model of ops.region_label_table"""
    lut = np.zeros(256, dtype=np.uint32)
    for r, labels in enumerate(regions):
        for l in (labels if isinstance(labels, (list, tuple)) else (labels,)):
            lut[int(l)] |= np.uint32(1 << r)
    if ignore_label is not None:
        lut[int(ignore_label)] |= np.uint32(1 << 31)
    return lut


def soft_dice(p, y, m, batch_dice, do_bg, smooth):
    """-mean dc, dc = (2I + s) / clip(G + P + s, 1e-8) with I, P, G masked by m; p, y [N,C,...], m [N,1,...] or None"""
    if not do_bg:
        p, y = p[:, 1:], y[:, 1:]
    axes = tuple(range(2, p.dim()))
    mm = 1.0 if m is None else m
    I, P, G = (p * y * mm).sum(axes), (p * mm).sum(axes), (y * mm).sum(axes)
    if batch_dice:
        I, P, G = I.sum(0), P.sum(0), G.sum(0)
    return -((2 * I + smooth) / torch.clip(G + P + smooth, 1e-8)).mean()


def dc_and_bce(z, planes, use_ignore_label=False, batch_dice=False, do_bg=True, smooth=1e-5, w_ce=1.0, w_dice=1.0,
               parts=False):
    """DC_and_BCE_loss: `planes` [N,R(+1),...] (the ignore plane last when use_ignore_label)"""
    z, planes = z.double(), planes.double()
    if use_ignore_label:
        m = 1 - planes[:, -1:]
        y = planes[:, :-1]
    else:
        m, y = None, planes
    dice = soft_dice(torch.sigmoid(z), y, m, batch_dice, do_bg, smooth)
    if m is not None:
        bce = (F.binary_cross_entropy_with_logits(z, y, reduction='none') * m).sum() / torch.clip(m.sum(), min=1e-8)
    else:
        bce = F.binary_cross_entropy_with_logits(z, y)
    total = w_ce * bce + w_dice * dice
    return (total, bce, dice) if parts else total


def dc_and_bce_labelmap(z, seg, regions, ignore_label=None, **kw):
    planes = torch.from_numpy(seg_to_regions(seg.detach().cpu().numpy(), regions, ignore_label))
    return dc_and_bce(z, planes, use_ignore_label=ignore_label is not None, **kw)


def dc_and_ce_masked(z, target, ignore_label, batch_dice=False, do_bg=False, smooth=1e-5, w_ce=1.0, w_dice=1.0,
                     parts=False):
    """DC_and_CE_loss(ignore_label=L): target [N,1,...] float labels; L may be None (no voxel ignored)"""
    z = z.double()
    t = target[:, 0].long()
    if ignore_label is None:
        m = torch.ones_like(target, dtype=torch.float64)
        td = t
        ce = F.cross_entropy(z, t)
    else:
        m = (target != ignore_label).double()
        td = torch.where(t == ignore_label, torch.zeros_like(t), t)
        ce = F.cross_entropy(z, t, ignore_index=ignore_label) if m.sum() > 0 else torch.zeros((), dtype=torch.float64)
    onehot = F.one_hot(td, z.shape[1]).movedim(-1, 1).double()
    dice = soft_dice(torch.softmax(z, 1), onehot, m, batch_dice, do_bg, smooth)
    total = w_ce * ce + w_dice * dice
    return (total, ce, dice) if parts else total


def deep_supervised(fn, outputs, targets, weights):
    return sum(w * fn(o, t) for w, o, t in zip(weights, outputs, targets))


def region_grad_formula(z, planes, use_ignore_label=False, batch_dice=False, do_bg=True, smooth=1e-5, w_ce=1.0, w_dice=1.0):
    """The analytic gradient the backward kernel evaluates: dz = m (w_ce c (s - y) + s (1 - s) (coefI y + coefP))"""
    z, planes = z.double(), planes.double()
    N, R = z.shape[:2]
    if use_ignore_label:
        m, y = 1 - planes[:, -1:], planes[:, :-1]
        c = 1.0 / torch.clip(m.sum(), min=1e-8)
    else:
        m, y = torch.ones_like(z[:, :1]), planes
        c = 1.0 / z.numel()
    s = torch.sigmoid(z)
    axes = tuple(range(2, z.dim()))
    I, P, G = (s * y * m).sum(axes), (s * m).sum(axes), (y * m).sum(axes)
    k0 = 0 if do_bg else 1
    if batch_dice:
        I, P, G = I.sum(0, keepdim=True), P.sum(0, keepdim=True), G.sum(0, keepdim=True)
        cnt = R - k0
    else:
        cnt = N * (R - k0)
    den = G + P + smooth
    clipped = den < 1e-8
    den = torch.clip(den, 1e-8)
    num = 2 * I + smooth
    cI = (-2.0 / den / cnt).expand(N, R).clone()
    cP = torch.where(clipped, torch.zeros_like(den), num / den ** 2 / cnt).expand(N, R).clone()
    cI[:, :k0] = 0
    cP[:, :k0] = 0
    shp = (N, R) + (1,) * len(axes)
    return m * (w_ce * c * (s - y) + s * (1 - s) * (w_dice * cI.reshape(shp) * y + w_dice * cP.reshape(shp)))


def sigmoid_counts(z, planes, has_ignore_plane=False):
    """validation_step :969-1002, region branch: int64 [R,3] tp, fp, fn.  A head is on where z > 0."""
    z, planes = np.asarray(z), np.asarray(planes)
    m = (planes[:, -1:] < 0.5) if has_ignore_plane else np.ones_like(planes[:, :1], dtype=bool)
    y = (planes[:, :-1] if has_ignore_plane else planes) >= 0.5
    p = z > 0
    ax = (0,) + tuple(range(2, z.ndim))
    return np.stack([(p & y & m).sum(ax), (p & ~y & m).sum(ax), (~p & y & m).sum(ax)], 1).astype(np.int64)


def argmax_counts_masked(z, target, ignore_label):
    """validation_step :973-1002, label branch with an ignore label: int64 [K,3] (background row included)"""
    z, t = np.asarray(z), np.asarray(target)[:, 0].astype(np.int64)
    K = z.shape[1]
    m = t != ignore_label
    t = np.where(m, t, 0)
    best = z.argmax(1)
    out = np.zeros((K, 3), np.int64)
    for k in range(K):
        out[k] = [((best == k) & (t == k) & m).sum(), ((best == k) & (t != k) & m).sum(), ((best != k) & (t == k) & m).sum()]
    return out


def regions_to_segmentation(prob, regions_class_order):
    """label_handling.py:163-171 on [R, ...] probabilities"""
    seg = np.zeros(prob.shape[1:], dtype=np.uint16)
    for i, c in enumerate(regions_class_order):
        seg[prob[i] > 0.5] = c
    return seg
