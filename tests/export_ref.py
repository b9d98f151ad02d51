"""fp64 scipy / numpy restatement of the export and evaluation tail that the device path is tested against
(test_export_host.py, test_gpu_export.py).  skimage is not a dependency: `resize(order=1, mode='edge',
anti_aliasing=False)` is stood in for by scipy.ndimage.zoom(order=1, mode='nearest', grid_mode=True), and the
separate-z branch of default_resampling.py:150-195 by per-slice 2-D zooms followed by map_coordinates(order=0,
mode='nearest') on the pixel-centre coordinate map."""
import numpy as np
import scipy.ndimage as ndi


def smooth_logits(K, shape, seed=0, sigma=2.0, std=8.0, clip=64.0):
    """Gaussian-smoothed noise per channel, scaled to `std`, clipped to +-clip, float32."""
    rng = np.random.default_rng(seed)
    x = np.stack([ndi.gaussian_filter(rng.standard_normal(shape), sigma, mode='nearest') for _ in range(K)])
    x = x / x.std() * std
    return np.clip(x, -clip, clip).astype(np.float32)


def _zoom1(x, out_shape):
    if tuple(x.shape) == tuple(out_shape):
        return x.astype(np.float64)
    return ndi.zoom(x.astype(np.float64), [o / i for o, i in zip(out_shape, x.shape)], order=1, mode='nearest',
                    grid_mode=True)


def resample_logits(logits, new_shape, separate_z_axis=None):
    """[K, d, h, w] -> fp64 [K, *new_shape]"""
    new_shape = tuple(int(v) for v in new_shape)
    out = []
    for c in logits:
        if tuple(c.shape) == new_shape:
            out.append(c.astype(np.float64))
        elif separate_z_axis is None:
            out.append(_zoom1(c, new_shape))
        else:
            ax = separate_z_axis
            shape2d = tuple(n for a, n in enumerate(new_shape) if a != ax)
            slices = [_zoom1(np.take(c, s, axis=ax), shape2d) for s in range(c.shape[ax])]
            r = np.stack(slices, ax)
            if r.shape[ax] != new_shape[ax]:
                grids = np.mgrid[:new_shape[0], :new_shape[1], :new_shape[2]]
                coord = np.array([(float(r.shape[a]) / new_shape[a]) * (grids[a] + 0.5) - 0.5 for a in range(3)])
                r = ndi.map_coordinates(r, coord, order=0, mode='nearest')
            out.append(r)
    return np.stack(out)


def softmax_f32(res):
    import torch
    return torch.softmax(torch.from_numpy(res.astype(np.float32)), 0).numpy()


def margin(res):
    """top-1 minus top-2 of the fp64 resampled logits"""
    s = np.sort(res, 0)
    return s[-1] - s[-2] if res.shape[0] > 1 else np.full(res.shape[1:], np.inf)


def paste_transpose(vol, full, lo, transpose_backward, fill=0):
    """vol [..., D, H, W] -> pre-crop volume `full` with vol at `lo`, last three axes permuted"""
    lead = vol.shape[:-3]
    out = np.full(lead + tuple(full), fill, dtype=vol.dtype)
    sl = tuple(slice(l, l + n) for l, n in zip(lo, vol.shape[-3:]))
    out[(Ellipsis,) + sl] = vol
    n = len(lead)
    return np.ascontiguousarray(out.transpose(list(range(n)) + [n + a for a in transpose_backward]))


def export(logits, new_shape, full, lo, transpose_backward, separate_z_axis=None):
    """-> (uint8 segmentation, float32 probabilities [K, ...], fp64 margin) in the original axis order; outside the
    bbox: label 0, probability 1 in channel 0, margin inf."""
    res = resample_logits(logits, new_shape, separate_z_axis)
    prob = softmax_f32(res)
    seg = prob.argmax(0).astype(np.uint8)
    segf = paste_transpose(seg, full, lo, transpose_backward)
    probf = paste_transpose(prob, full, lo, transpose_backward)
    inside = paste_transpose(np.ones(seg.shape, bool), full, lo, transpose_backward)
    probf[0][~inside] = 1
    mar = paste_transpose(margin(res), full, lo, transpose_backward, fill=np.inf)
    return segf, probf, mar


def counts(ref, pred, labels_or_regions, ignore_label=None):
    """int64 [R, 4] TP, FP, FN, TN as evaluate_predictions.compute_metrics counts them"""
    use = np.ones(ref.shape, bool) if ignore_label is None else ref != ignore_label
    out = []
    for r in labels_or_regions:
        ls = list(r) if isinstance(r, (tuple, list)) else [r]
        mr, mp = np.isin(ref, ls), np.isin(pred, ls)
        out.append([np.sum(mr & mp & use), np.sum(~mr & mp & use), np.sum(mr & ~mp & use), np.sum(~mr & ~mp & use)])
    return np.array(out, dtype=np.int64)
