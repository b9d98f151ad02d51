"""Surface distances of two segmentations on the MI355X: exact Euclidean distance transform, Hausdorff
distance, its 95th percentile and the average (symmetric) surface distance.

Mirrors what the reference's evaluation/Hausdorff.py and evaluation/metrics.py:312-382 get from medpy
(`metric.hd`, `hd95`, `asd`, `assd`, all through `__surface_distances`): border(m) = m ^ binary_erosion(m, footprint),
dt = distance_transform_edt(~border(reference), sampling), sds = dt[border(result)].  The border pass, the three passes
of the transform, the gather and the sums are HIP kernels (csrc/surface.hip); the transform runs on the bounding box
of both masks, which the host reads (with the voxel counts) in one synchronisation before it sizes the launches; the
results cost a second one.  torch.sort orders the surface-sized vectors; numpy's percentile interpolation is restated
on the host in fp64.  Device tensors in (numpy volumes are uploaded), host torch tensors are refused: no CPU path.
"""
import ctypes
import math
from typing import Optional, Sequence

import numpy as np
import torch

from ._lib import call, query

MAX_EXTENT = 1024          # 3 * 1023^2 < 2^31: squared voxel distances stay in int32
_FORCE_FULL_BOX = False    # cross-check only (tests): transform the whole volume instead of the masks' bounding box


def footprint_offsets(connectivity: int):
    """Offsets (dz, dy, dx) of scipy's generate_binary_structure(3, connectivity), the centre included."""
    if connectivity not in (1, 2, 3):
        raise ValueError(f"connectivity {connectivity} not in 1..3")
    r = (-1, 0, 1)
    return [(dz, dy, dx) for dz in r for dy in r for dx in r if abs(dz) + abs(dy) + abs(dx) <= connectivity]


# ------------------------------------------------------------------------------------------------ numpy.percentile
def percentile_indices(n: int, q: float = 95.0):
    """(lo, hi, gamma) of numpy.percentile's default 'linear' method on n sorted values: the result is
    lerp(x[lo], x[hi], gamma)."""
    if n < 1:
        raise ValueError("percentile of an empty vector")
    virtual = (n - 1) * (q / 100.0)
    previous = math.floor(virtual)
    gamma = virtual - previous
    if virtual >= n - 1:
        return n - 1, n - 1, gamma
    return int(previous), int(previous) + 1, gamma


def lerp(a: float, b: float, t: float) -> float:
    """numpy's _lerp in fp64: a + (b - a) t, and b - (b - a)(1 - t) from t = 0.5 on."""
    a, b, t = float(a), float(b), float(t)
    d = b - a
    return b - d * (1 - t) if t >= 0.5 else a + d * t


def percentile(values, q: float = 95.0) -> float:
    """numpy.percentile(values, q) of a host vector, bit for bit (the device path sorts with torch.sort instead)."""
    x = np.sort(np.asarray(values, dtype=np.float64).ravel())
    lo, hi, g = percentile_indices(len(x), q)
    return lerp(x[lo], x[hi], g)


# ------------------------------------------------------------------------------------------------------ arguments
def _check_shape(shape, what):
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError(f"{what}: a non-empty 3-D volume is needed, not {tuple(shape)} (2-D inputs are out of scope)")
    if max(shape) > MAX_EXTENT:
        raise NotImplementedError(f"{what}: extents above {MAX_EXTENT} are not built ({tuple(shape)})")


def _check_spacing(spacing) -> Optional[Sequence[float]]:
    """None for unit spacing (the integer path), else three positive floats."""
    if spacing is None:
        return None
    s = [float(v) for v in (spacing.tolist() if hasattr(spacing, "tolist") else spacing)]
    if len(s) != 3 or not all(v > 0 and math.isfinite(v) for v in s):
        raise ValueError(f"voxelspacing must be three positive numbers, not {spacing}")
    return None if s == [1.0, 1.0, 1.0] else s


def _check_connectivity(connectivity):
    if connectivity not in (1, 2, 3):
        raise ValueError(f"connectivity {connectivity} not in 1..3")


def _volume(x, device, what, labels=False):
    """contiguous device volume: uint8 / int16 labels, or a 0/1 uint8 mask of any input dtype"""
    if isinstance(x, np.ndarray):
        _check_shape(x.shape, what)
        x = torch.from_numpy(np.ascontiguousarray(x)).to(device or "cuda:0")
    if not isinstance(x, torch.Tensor):
        raise RuntimeError(f"{what}: pass a device tensor or a numpy array")
    _check_shape(x.shape, what)
    if not x.is_cuda:
        raise RuntimeError(f"{what}: surface distances are computed on the GPU, pass a device tensor or a numpy array "
                           f"(there is no CPU fallback)")
    if labels:
        if x.dtype == torch.bool:
            x = x.to(torch.uint8)
        if x.dtype not in (torch.uint8, torch.int16):
            raise RuntimeError(f"{what} must be uint8 or int16, not {x.dtype}")
        return x.contiguous()
    return (x != 0).to(torch.uint8).contiguous()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


# ------------------------------------------------------------------------------------------------------- launches
def _border(a, b, label_set, connectivity):
    """uint8 border volume (bit 0: border of {a in set}, bit 1: of {b in set}) and the int32[10] statistics."""
    if a.shape != b.shape or a.device != b.device:
        raise ValueError(f"volumes differ in shape or device: {tuple(a.shape)} and {tuple(b.shape)}")
    D, H, W = a.shape
    border = torch.empty((D, H, W), dtype=torch.uint8, device=a.device)
    stats = torch.empty((10,), dtype=torch.int32, device=a.device)
    ls = (ctypes.c_int32 * len(label_set))(*[int(v) for v in label_set])
    call("mvd_surf_border", _p(a), int(a.dtype == torch.int16), _p(b), int(b.dtype == torch.int16), D, H, W,
         ctypes.cast(ls, ctypes.c_void_p), len(label_set), int(connectivity), _p(border), _p(stats), _stream())
    return border, stats


def _edt_squared(vol, bit, zero_is_site, box, spacing):
    """(workspace, squared distances over the box): int32 at unit spacing, fp64 otherwise.  The second is a view of the
    first."""
    D, H, W = vol.shape
    bd, bh, bw = box[3:]
    spaced = spacing is not None
    nbytes = query("mvd_edt_workspace_bytes", bd, bh, bw, int(spaced))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=vol.device)
    cbox = (ctypes.c_int * 6)(*box)
    csp = (ctypes.c_double * 3)(*spacing) if spaced else None
    call("mvd_edt_squared", _p(vol), int(bit), int(zero_is_site), D, H, W, ctypes.cast(cbox, ctypes.c_void_p),
         ctypes.cast(csp, ctypes.c_void_p) if spaced else None, _p(ws), nbytes, _stream())
    n = bd * bh * bw
    sq = ws[:n * (8 if spaced else 4)].view(torch.float64 if spaced else torch.int32).view(bd, bh, bw)
    return ws, sq


def _gather(sq, spaced, border, bit, box, out, counter):
    D, H, W = border.shape
    cbox = (ctypes.c_int * 6)(*box)
    call("mvd_surf_gather", _p(sq), int(spaced), _p(border), int(bit), D, H, W, ctypes.cast(cbox, ctypes.c_void_p),
         _p(out), out.numel(), _p(counter), _stream())


class _Stats:
    """host copy of the border pass's statistics"""

    def __init__(self, st, shape):
        st = [int(v) for v in st]
        self.n_a, self.n_b, self.nb_a, self.nb_b = st[:4]
        self.voxels = shape[0] * shape[1] * shape[2]
        if self.n_a + self.n_b > 0 and not _FORCE_FULL_BOX:
            lo = [MAX_EXTENT - v for v in st[4:7]]
            self.box = lo + [h - l for h, l in zip(st[7:10], lo)]
        else:
            self.box = [0, 0, 0] + list(shape)

    @property
    def nonexisting(self):
        """the reference's test_empty / test_full / reference_empty / reference_full rule"""
        return self.n_a == 0 or self.n_b == 0 or self.n_a == self.voxels or self.n_b == self.voxels


def _queue_distances(border, st, spacing):
    """fp64 device vector of nb_a + nb_b values: sds(a, b) then sds(b, a), each in an unspecified order."""
    vals = torch.empty((st.nb_a + st.nb_b,), dtype=torch.float64, device=border.device)
    counter = torch.empty((2,), dtype=torch.int32, device=border.device)
    for site_bit, query_bit, out, cnt in ((2, 1, vals[:st.nb_a], counter[0:1]), (1, 2, vals[st.nb_a:], counter[1:2])):
        ws, sq = _edt_squared(border, site_bit, 0, st.box, spacing)
        _gather(sq, spacing is not None, border, query_bit, st.box, out, cnt)
        del ws, sq
    return vals


def _queue_reduce(vals, st, out_row):
    """sorts (torch.sort: surface-sized plumbing) and the fixed-order reduction into out_row (fp64[6]); returns gamma"""
    s0 = torch.sort(vals[:st.nb_a]).values
    s1 = torch.sort(vals[st.nb_a:]).values
    al = torch.sort(vals).values
    lo, hi, gamma = percentile_indices(st.nb_a + st.nb_b, 95.0)
    call("mvd_surf_reduce", _p(s0), st.nb_a, _p(s1), st.nb_b, _p(al), lo, hi, _p(out_row), _stream())
    return gamma


def _finish(row, st, gamma):
    sum0, sum1, max0, max1, qlo, qhi = (float(v) for v in row)
    asd_ab, asd_ba = sum0 / st.nb_a, sum1 / st.nb_b
    return {'HD': max(max0, max1), 'HD95': lerp(qlo, qhi, gamma), 'ASD': asd_ab, 'ASD_reverse': asd_ba,
            'ASSD': float(np.mean((asd_ab, asd_ba)))}


def _binary_metrics(result, reference, voxelspacing, connectivity):
    spacing = _check_spacing(voxelspacing)
    _check_connectivity(connectivity)
    a = _volume(result, None, "result")
    b = _volume(reference, a.device, "reference")
    border, stats = _border(a, b, [1], connectivity)
    st = _Stats(stats.cpu().numpy(), a.shape)                     # synchronisation 1: counts and bounding box
    if st.n_a == 0:
        raise RuntimeError('The first supplied array does not contain any binary object.')
    if st.n_b == 0:
        raise RuntimeError('The second supplied array does not contain any binary object.')
    row = torch.empty((6,), dtype=torch.float64, device=a.device)
    gamma = _queue_reduce(_queue_distances(border, st, spacing), st, row)
    return _finish(row.cpu().numpy(), st, gamma)                  # synchronisation 2


# ------------------------------------------------------------------------------------------------ public interface
def distance_transform_edt(mask, sampling=None, return_squared: bool = False):
    """scipy.ndimage.distance_transform_edt(mask, sampling) on the device: the distance of every nonzero voxel to the
    nearest zero voxel (0 on zero voxels), fp64.  return_squared: the squared distance, int32 when sampling is None."""
    spacing = _check_spacing(sampling)
    m = _volume(mask, None, "mask")
    ws, sq = _edt_squared(m, 1, 1, [0, 0, 0] + list(m.shape), spacing)
    if return_squared:
        return sq.clone()
    out = torch.empty(sq.shape, dtype=torch.float64, device=m.device)
    call("mvd_edt_root", _p(sq), int(spacing is not None), sq.numel(), _p(out), _stream())
    return out


def surface_border(mask, connectivity: int = 1):
    """uint8 volume: mask ^ binary_erosion(mask, generate_binary_structure(3, connectivity)), border_value 0."""
    _check_connectivity(connectivity)
    m = _volume(mask, None, "mask")
    border, _ = _border(m, m, [1], connectivity)
    return border & 1


def surface_distances(result, reference, voxelspacing=None, connectivity: int = 1):
    """medpy's __surface_distances(result, reference): the distances of the border voxels of `result` to the border of
    `reference`, a 1-D fp64 device tensor in an unspecified order."""
    spacing = _check_spacing(voxelspacing)
    _check_connectivity(connectivity)
    a = _volume(result, None, "result")
    b = _volume(reference, a.device, "reference")
    border, stats = _border(a, b, [1], connectivity)
    st = _Stats(stats.cpu().numpy(), a.shape)
    if st.n_a == 0:
        raise RuntimeError('The first supplied array does not contain any binary object.')
    if st.n_b == 0:
        raise RuntimeError('The second supplied array does not contain any binary object.')
    out = torch.empty((st.nb_a,), dtype=torch.float64, device=a.device)
    counter = torch.empty((1,), dtype=torch.int32, device=a.device)
    ws, sq = _edt_squared(border, 2, 0, st.box, spacing)
    _gather(sq, spacing is not None, border, 1, st.box, out, counter)
    return torch.sort(out).values


def hd(result, reference, voxelspacing=None, connectivity: int = 1) -> float:
    return _binary_metrics(result, reference, voxelspacing, connectivity)['HD']


def hd95(result, reference, voxelspacing=None, connectivity: int = 1) -> float:
    return _binary_metrics(result, reference, voxelspacing, connectivity)['HD95']


def asd(result, reference, voxelspacing=None, connectivity: int = 1) -> float:
    return _binary_metrics(result, reference, voxelspacing, connectivity)['ASD']


def assd(result, reference, voxelspacing=None, connectivity: int = 1) -> float:
    return _binary_metrics(result, reference, voxelspacing, connectivity)['ASSD']


def _wrapped(key):
    def wrapper(test=None, reference=None, confusion_matrix=None, nan_for_nonexisting=True, voxel_spacing=None,
                connectivity=1, **kwargs):
        if confusion_matrix is not None:
            raise NotImplementedError("the reference's ConfusionMatrix object is not built; pass test and reference")
        spacing = _check_spacing(voxel_spacing)
        _check_connectivity(connectivity)
        a = _volume(test, None, "test")
        b = _volume(reference, a.device, "reference")
        border, stats = _border(a, b, [1], connectivity)
        st = _Stats(stats.cpu().numpy(), a.shape)
        if st.nonexisting:
            return float("NaN") if nan_for_nonexisting else 0
        row = torch.empty((6,), dtype=torch.float64, device=a.device)
        gamma = _queue_reduce(_queue_distances(border, st, spacing), st, row)
        return _finish(row.cpu().numpy(), st, gamma)[key]
    return wrapper


hausdorff_distance = _wrapped('HD')                  # evaluation/metrics.py:312-327
hausdorff_distance_95 = _wrapped('HD95')             # :330-345
avg_surface_distance = _wrapped('ASD')               # :348-363
avg_surface_distance_symmetric = _wrapped('ASSD')    # :366-381


def compute_surface_metrics(seg_ref, seg_pred, labels_or_regions, spacing=None, connectivity: int = 1,
                            ignore_label: Optional[int] = None) -> dict:
    """{label_or_region: {'HD', 'HD95', 'ASSD'}} between two label volumes (uint8 / int16; the prediction is medpy's
    `result`), NaN where either mask is empty or full.  The border passes of all labels are queued, the host reads
    their counts and boxes once, queues everything else and reads the results once: two synchronisations per case."""
    from .evaluation import _label_sets, _region_key
    if ignore_label is not None:
        raise NotImplementedError("surface metrics with an ignore label are not built (the reference's functions do "
                                  "not know one)")
    sp = _check_spacing(spacing)
    _check_connectivity(connectivity)
    sets = _label_sets(labels_or_regions)
    pred = _volume(seg_pred, None, "seg_pred", labels=True)
    ref = _volume(seg_ref, pred.device, "seg_ref", labels=True)
    borders, stats = zip(*[_border(pred, ref, s, connectivity) for s in sets])
    stats = torch.stack(stats).cpu().numpy()                      # synchronisation 1
    rows = torch.zeros((len(sets), 6), dtype=torch.float64, device=pred.device)
    sts, gammas = [], []
    for r in range(len(sets)):
        st = _Stats(stats[r], pred.shape)
        sts.append(st)
        gammas.append(None if st.nonexisting else _queue_reduce(_queue_distances(borders[r], st, sp), st, rows[r]))
    rows = rows.cpu().numpy()                                     # synchronisation 2
    out = {}
    for r, key in enumerate(labels_or_regions):
        if gammas[r] is None:
            m = {'HD': float("NaN"), 'HD95': float("NaN"), 'ASSD': float("NaN")}
        else:
            f = _finish(rows[r], sts[r], gammas[r])
            m = {'HD': f['HD'], 'HD95': f['HD95'], 'ASSD': f['ASSD']}
        out[_region_key(key)] = m
    return out
