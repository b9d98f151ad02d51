"""fp64 scipy / numpy restatement of medpy's surface distances (`medpy.metric.binary.__surface_distances`, `hd`, `hd95`,
`asd`, `assd`) and of the reference's NaN rule around them (evaluation/metrics.py:312-382), which the device path is
tested against (test_surface_host.py, test_gpu_surface.py).  medpy is not a dependency: parity is pinned to THIS
restatement.  `brute_force_sds` is the definition itself, min_q sqrt(sum_i ((p_i - q_i) s_i)^2) in fp64 with the axes
added in the order 0, 1, 2; scipy's transform was found to agree with it bit for bit."""
import numpy as np
import scipy.ndimage as ndi


def blob_mask(shape, seed=0, sigma=3.0, fill=0.2):
    """Gaussian-smoothed seeded normal noise, thresholded so that about `fill` of the volume is set."""
    rng = np.random.default_rng(seed)
    x = ndi.gaussian_filter(rng.standard_normal(shape), sigma, mode='nearest')
    return x > np.quantile(x, 1.0 - fill)


def blob_pair(shape, seed=0, sigma=3.0, fill=0.2, shift=(1, -2, 2), extra=0.02):
    """(a, b): b is a shifted copy of a joined with sparse extra blobs, so that the two directions differ."""
    a = blob_mask(shape, seed, sigma, fill)
    b = ndi.shift(a.astype(np.uint8), [min(s, n - 1) if n > 1 else 0 for s, n in zip(shift, shape)], order=0,
                  mode='constant', cval=0).astype(bool)
    b |= blob_mask(shape, seed + 1000, sigma * 0.7, extra)
    return a, b


def footprint(connectivity):
    return ndi.generate_binary_structure(3, connectivity)


def border(mask, connectivity=1):
    mask = np.asarray(mask).astype(bool)
    return mask ^ ndi.binary_erosion(mask, structure=footprint(connectivity), iterations=1)


def _spacing(voxelspacing):
    return None if voxelspacing is None else tuple(float(v) for v in voxelspacing)


def surface_distances(result, reference, voxelspacing=None, connectivity=1):
    result = np.atleast_1d(np.asarray(result).astype(bool))
    reference = np.atleast_1d(np.asarray(reference).astype(bool))
    if 0 == np.count_nonzero(result):
        raise RuntimeError('The first supplied array does not contain any binary object.')
    if 0 == np.count_nonzero(reference):
        raise RuntimeError('The second supplied array does not contain any binary object.')
    dt = ndi.distance_transform_edt(~border(reference, connectivity), sampling=_spacing(voxelspacing))
    return dt[border(result, connectivity)]


def hd(result, reference, voxelspacing=None, connectivity=1):
    return float(max(surface_distances(result, reference, voxelspacing, connectivity).max(),
                     surface_distances(reference, result, voxelspacing, connectivity).max()))


def hd95(result, reference, voxelspacing=None, connectivity=1):
    return float(np.percentile(np.hstack((surface_distances(result, reference, voxelspacing, connectivity),
                                          surface_distances(reference, result, voxelspacing, connectivity))), 95))


def asd(result, reference, voxelspacing=None, connectivity=1):
    return float(surface_distances(result, reference, voxelspacing, connectivity).mean())


def assd(result, reference, voxelspacing=None, connectivity=1):
    return float(np.mean((asd(result, reference, voxelspacing, connectivity),
                          asd(reference, result, voxelspacing, connectivity))))


def _nonexisting(test, reference):
    test, reference = np.asarray(test) != 0, np.asarray(reference) != 0
    return (not test.any()) or test.all() or (not reference.any()) or reference.all()


def _wrapped(fn):
    def wrapper(test, reference, nan_for_nonexisting=True, voxel_spacing=None, connectivity=1):
        if _nonexisting(test, reference):
            return float("NaN") if nan_for_nonexisting else 0
        return fn(np.asarray(test) != 0, np.asarray(reference) != 0, voxel_spacing, connectivity)
    return wrapper


hausdorff_distance = _wrapped(hd)
hausdorff_distance_95 = _wrapped(hd95)
avg_surface_distance = _wrapped(asd)
avg_surface_distance_symmetric = _wrapped(assd)


def surface_metrics(seg_ref, seg_pred, labels_or_regions, spacing=None, connectivity=1):
    """{label_or_region: {'HD', 'HD95', 'ASSD'}} on label volumes; the prediction is medpy's `result`."""
    out = {}
    for r in labels_or_regions:
        ls = list(r) if isinstance(r, (tuple, list)) else [r]
        a, b = np.isin(seg_pred, ls), np.isin(seg_ref, ls)
        key = tuple(int(v) for v in r) if isinstance(r, (tuple, list)) else int(r)
        out[key] = {'HD': hausdorff_distance(a, b, True, spacing, connectivity),
                    'HD95': hausdorff_distance_95(a, b, True, spacing, connectivity),
                    'ASSD': avg_surface_distance_symmetric(a, b, True, spacing, connectivity)}
    return out


def brute_force_sds(result, reference, voxelspacing=None, connectivity=1, chunk=256):
    s = np.ones(3) if voxelspacing is None else np.asarray(voxelspacing, dtype=np.float64)
    q = np.argwhere(border(reference, connectivity)).astype(np.float64)
    p = np.argwhere(border(result, connectivity)).astype(np.float64)
    out = np.empty(len(p))
    for i in range(0, len(p), chunk):
        d = p[i:i + chunk, None, :] - q[None, :, :]
        d2 = ((d[..., 0] * s[0]) ** 2 + (d[..., 1] * s[1]) ** 2) + (d[..., 2] * s[2]) ** 2
        out[i:i + chunk] = np.sqrt(d2.min(1))
    return out
