"""numpy / scipy restatement of nnU-Net's three cascade transforms (custom_transforms/cascade_transforms.py):
MoveSegAsOneHotToData, ApplyRandomBinaryOperatorTransform and RemoveRandomConnectedComponentFromOneHotEncodingTransform.

skimage, acvl_utils and batchgenerators are absent, so their parts are restated over scipy.ndimage and parity with those
packages themselves is unpinned:
  ball(r)                      skimage.morphology.ball with a float radius
  binary_dilation / _erosion   skimage (<= 0.22): ndi.binary_dilation(image, structure=ball),
                               ndi.binary_erosion(image, structure=ball, border_value=True); closing = erosion of the
                               dilation, opening = dilation of the erosion, same element
  label_with_component_sizes   skimage.measure.label at full connectivity == ndi.label(structure=np.ones((3, 3, 3)))
The glue of the two random transforms -- which draws, in which order, what is written where -- is pinned to the reference's
own class bodies through tests/golden/cascade_transforms.npz (tools/make_golden.py executes them over these stand-ins).
"""
import math

import numpy as np
from scipy import ndimage as ndi

OPS = ('dilation', 'erosion', 'closing', 'opening')  # the order of the transform's any_of_these


def ball(radius):
    n = int(2 * radius + 1)
    z, y, x = np.meshgrid(*([np.linspace(-radius, radius, n)] * 3), indexing='ij')
    return np.array(x ** 2 + y ** 2 + z ** 2 <= radius ** 2, dtype=np.uint8)


def binary_dilation(image, footprint):
    return ndi.binary_dilation(image, structure=footprint)


def binary_erosion(image, footprint):
    return ndi.binary_erosion(image, structure=footprint, border_value=True)


def binary_closing(image, footprint):
    return binary_erosion(binary_dilation(image, footprint), footprint)


def binary_opening(image, footprint):
    return binary_dilation(binary_erosion(image, footprint), footprint)


OPERATORS = (binary_dilation, binary_erosion, binary_closing, binary_opening)


def label_with_component_sizes(mask):
    lab, n = ndi.label(mask, structure=np.ones((3, 3, 3)))
    sizes = np.bincount(lab.ravel(), minlength=n + 1)
    return lab, {i: int(sizes[i]) for i in range(1, n + 1)}


def element_rows(radius):
    """The element as the kernel takes it: rows (dz, dy, lo, hi) of READ offsets of the erosion, offset = index - n // 2
    (scipy centres an even-sided element at n // 2); the dilation reads the negated offsets."""
    b = ball(radius)
    n = b.shape[0]
    c = n // 2
    rows = []
    for iz in range(n):
        for iy in range(n):
            xs = np.flatnonzero(b[iz, iy])
            if len(xs) == 0:
                continue
            if xs[-1] - xs[0] + 1 != len(xs):
                raise ValueError("ball row is not one interval")
            rows.append((iz - c, iy - c, int(xs[0]) - c, int(xs[-1]) - c))
    return rows


def morph_from_rows(image, rows, erode):
    """What the kernel computes from a row table, in numpy: the host-side check that the table reproduces scipy."""
    image = np.asarray(image, dtype=bool)
    D, H, W = image.shape
    p = 8
    pad = np.pad(image, p, constant_values=bool(erode))
    out = np.ones_like(image) if erode else np.zeros_like(image)
    for dz, dy, lo, hi in rows:
        if not erode:
            dz, dy, lo, hi = -dz, -dy, -hi, -lo
        for dx in range(lo, hi + 1):
            v = pad[p + dz:p + dz + D, p + dy:p + dy + H, p + dx:p + dx + W]
            out = (out & v) if erode else (out | v)
    return out


def morph_op(image, op, radius):
    return OPERATORS[op](np.asarray(image, dtype=bool), ball(radius))


def apply_operator(planes, c, op, radius):
    """One channel step of ApplyRandomBinaryOperatorTransform on bool planes [K,D,H,W], in place: the operator on
    channel c (skipped when it is empty), then every other channel loses the voxels that were added."""
    workon = planes[c].copy()
    if not workon.any():
        return
    res = morph_op(workon, op, radius)
    planes[c] = res
    added = res & ~workon
    for oc in range(planes.shape[0]):
        if oc != c:
            planes[oc][added] = False


def move_seg_as_onehot(seg_channel, labels, dtype=np.float32):
    return np.stack([(seg_channel == l) for l in labels]).astype(dtype)


def draw_binary_operator(nsamples, channel_order, p_per_sample=0.4, strel_size=(1, 8), p_per_label=1):
    """ApplyRandomBinaryOperatorTransform's draws for a batch: per sample a uniform; np.random.shuffle of the channel list
    IN PLACE (the order persists from call to call); per channel a uniform, a choice among the four operators and
    uniform(*strel_size).  Returns per sample None or a list of (channel, op index, radius); a channel whose p_per_label
    uniform fails is left out."""
    out = []
    for _ in range(nsamples):
        if np.random.uniform() < p_per_sample:
            np.random.shuffle(channel_order)
            steps = []
            for c in channel_order:
                if np.random.uniform() < p_per_label:
                    op = int(np.random.choice(len(OPS)))
                    radius = float(np.random.uniform(*strel_size))
                    steps.append((int(c), op, radius))
            out.append(steps)
        else:
            out.append(None)
    return out


def binary_operator_transform(data, channel_idx, p_per_sample=0.4, strel_size=(1, 8), p_per_label=1):
    """The whole transform on data [B,C,D,H,W] (float), in place, drawing from np.random as the reference does;
    channel_idx is shuffled in place.  Returns the channel order after each shuffle."""
    orders = []
    for b in range(data.shape[0]):
        steps = draw_binary_operator(1, channel_idx, p_per_sample, strel_size, p_per_label)[0]
        if steps is None:
            continue
        orders.append(list(channel_idx))
        for c, op, radius in steps:
            workon = data[b, c].astype(bool)
            if not workon.any():
                continue
            res = morph_op(workon, op, radius)
            data[b, c] = res.astype(data.dtype)
            added = res & ~workon
            for oc in channel_idx:
                if oc != c:
                    data[b, oc][added] = 0
    return orders


def removal_threshold(num_voxels, fraction=0.15):
    """The integer T with (size < T) == (size < num_voxels * fraction), the reference's fp64 test, for every integer size."""
    return int(math.ceil(float(np.uint64(num_voxels) * fraction)))


def remove_component(chan, u=None, ordinal=None, other=None, fraction=0.15):
    """The removal on one channel (float or bool [D,H,W]) in place with a forced pick: valid component number
    floor(u n_valid), or `ordinal`, in scipy.ndimage.label's order.  Returns (ordinal or None, n_valid)."""
    workon = np.asarray(chan).astype(bool)
    if not workon.any():
        return None, 0
    num_voxels = np.prod(workon.shape, dtype=np.uint64)
    lab, sizes = label_with_component_sizes(workon)
    valid = [i for i, j in sizes.items() if j < num_voxels * fraction]
    if not valid:
        return None, 0
    if ordinal is None:
        ordinal = min(len(valid) - 1, int(u * len(valid)))
    sel = lab == valid[ordinal]
    chan[sel] = 0
    if other is not None:
        other[sel] = 1
    return ordinal, len(valid)
