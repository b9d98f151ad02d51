"""Per-label TP/FP/FN/TN, Dice and IoU of predicted against reference segmentations, counted on the MI355X.

Mirrors nnunetv2/evaluation/evaluate_predictions.py: `region_or_label_to_mask` :70-78, `compute_tp_fp_fn_tn` :81-90,
`compute_metrics` :93-121 and the aggregation of `compute_metrics_on_folder` :123-175, on tensors instead of files (no
image reader / writer here).  The counts come from one HIP kernel (mvd_seg_confusion_counts: integer sums, exact and
run-to-run identical) and cost one host synchronisation per case; the ratios are formed on the host.  Numpy volumes are
uploaded, host torch tensors are refused: there is no CPU path.
"""
import ctypes
import warnings
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import call

MAX_LABEL_SETS = 32
MAX_LABELS_PER_SET = 16


def labels_to_list_of_regions(labels: List[int]):
    return [(i,) for i in labels]


def _region_key(r):
    return tuple(int(v) for v in r) if isinstance(r, (tuple, list)) else int(r)


def _label_sets(labels_or_regions) -> List[List[int]]:
    sets = []
    for r in labels_or_regions:
        s = [int(v) for v in r] if isinstance(r, (tuple, list)) else [int(r)]
        if not 1 <= len(s) <= MAX_LABELS_PER_SET:
            raise ValueError(f"a label set holds 1..{MAX_LABELS_PER_SET} labels")
        if min(s) < 0 or max(s) > 255:
            raise NotImplementedError("labels outside 0..255 (uint16 segmentations) are not built")
        sets.append(s)
    if not sets:
        raise ValueError("labels_or_regions is empty")
    return sets


def _device_volume(x, dtypes, device, what):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x)).to(device or "cuda:0")
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError(f"{what}: metrics are counted on the GPU, pass a device tensor or a numpy array (there is no "
                           f"CPU fallback)")
    if x.dtype == torch.bool:
        x = x.to(torch.uint8)
    if x.dtype not in dtypes:
        raise RuntimeError(f"{what} must be one of {[str(d) for d in dtypes]}, not {x.dtype}")
    x = x.contiguous()
    if x.data_ptr() % 16:
        x = x.clone()
    return x


def confusion_counts(seg_ref, seg_pred, labels_or_regions, ignore_label: Optional[int] = None, device=None) \
        -> torch.Tensor:
    """int64 [R, 4] device tensor {TP, FP, FN, TN} per label or region, over the voxels whose reference label is not
    `ignore_label`.  seg_pred: uint8; seg_ref: uint8 or int16 (same number of voxels)."""
    sets = _label_sets(labels_or_regions)
    pred = _device_volume(seg_pred, (torch.uint8,), device, "seg_pred")
    ref = _device_volume(seg_ref, (torch.uint8, torch.int16), pred.device, "seg_ref")
    if ref.device != pred.device:
        raise RuntimeError("seg_ref and seg_pred live on different devices")
    if ref.numel() != pred.numel() or ref.numel() == 0:
        raise ValueError(f"seg_ref {tuple(ref.shape)} and seg_pred {tuple(pred.shape)} differ in size")
    counts = torch.empty((len(sets), 4), dtype=torch.int64, device=pred.device)
    for r0 in range(0, len(sets), MAX_LABEL_SETS):
        chunk = sets[r0:r0 + MAX_LABEL_SETS]
        flat = (ctypes.c_int32 * (16 * len(chunk)))()
        for r, s in enumerate(chunk):
            flat[16 * r:16 * r + len(s)] = s
        sizes = (ctypes.c_int * len(chunk))(*[len(s) for s in chunk])
        call("mvd_seg_confusion_counts", ctypes.c_void_p(pred.data_ptr()), ctypes.c_void_p(ref.data_ptr()),
             int(ref.dtype == torch.int16), pred.numel(), ctypes.cast(flat, ctypes.c_void_p),
             ctypes.cast(sizes, ctypes.c_void_p), len(chunk), int(ignore_label is not None),
             int(ignore_label) if ignore_label is not None else 0, ctypes.c_void_p(counts[r0:].data_ptr()),
             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return counts


def compute_tp_fp_fn_tn(mask_ref, mask_pred, ignore_mask=None) -> Tuple[int, int, int, int]:
    """evaluate_predictions.py:81-90 for boolean (or 0/1) masks on the device."""
    dev = mask_pred.device if isinstance(mask_pred, torch.Tensor) else None
    ref = _device_volume(mask_ref, (torch.uint8,), dev, "mask_ref")
    if ignore_mask is not None:
        ign = _device_volume(ignore_mask, (torch.uint8,), ref.device, "ignore_mask")
        ref = torch.where(ign != 0, torch.full_like(ref, 2), (ref != 0).to(torch.uint8))
    c = confusion_counts(ref, _device_volume(mask_pred, (torch.uint8,), ref.device, "mask_pred"), [1],
                         2 if ignore_mask is not None else None).cpu().numpy()
    return tuple(int(v) for v in c[0])


def metrics_from_counts(counts, labels_or_regions) -> dict:
    """The 'metrics' dict of compute_metrics (:104-120) from integer counts [R][4] = TP, FP, FN, TN."""
    counts = np.asarray(counts)
    assert counts.shape == (len(labels_or_regions), 4), counts.shape
    metrics = {}
    for r, row in zip(labels_or_regions, counts):
        tp, fp, fn, tn = (int(v) for v in row)
        m = {}
        if tp + fp + fn == 0:
            m['Dice'] = np.nan
            m['IoU'] = np.nan
        else:
            m['Dice'] = 2 * tp / (2 * tp + fp + fn)
            m['IoU'] = tp / (tp + fp + fn)
        m['FP'], m['TP'], m['FN'], m['TN'] = fp, tp, fn, tn
        m['n_pred'] = fp + tp
        m['n_ref'] = fn + tp
        metrics[_region_key(r)] = m
    return metrics


def compute_metrics(seg_ref, seg_pred, labels_or_regions, ignore_label: Optional[int] = None, counts=None) -> dict:
    """evaluate_predictions.py:93-121 on volumes instead of files: {'metrics': {label_or_region: {'Dice', 'IoU', 'FP',
    'TP', 'FN', 'TN', 'n_pred', 'n_ref'}}}; Dice and IoU are nan where TP + FP + FN is 0.  `counts` ([R][4], e.g. from
    confusion_counts) skips the counting."""
    if counts is None:
        counts = confusion_counts(seg_ref, seg_pred, labels_or_regions, ignore_label).cpu().numpy()  # the host sync
    return {'metrics': metrics_from_counts(counts, labels_or_regions)}


def aggregate_metrics(results: Sequence[dict], regions_or_labels) -> dict:
    """compute_metrics_on_folder :150-172: nanmean per label over the cases, then the mean over the labels but 0."""
    keys = [_region_key(r) for r in regions_or_labels]
    metric_list = list(results[0]['metrics'][keys[0]].keys())
    means = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)   # a label absent from every case: nanmean of nans is nan
        for r in keys:
            means[r] = {m: float(np.nanmean([i['metrics'][r][m] for i in results])) for m in metric_list}
    foreground_mean = {}
    for m in metric_list:
        values = [means[k][m] for k in means.keys() if not (k == 0 or k == '0')]
        foreground_mean[m] = float(np.mean(values))
    return {'metric_per_case': list(results), 'mean': means, 'foreground_mean': foreground_mean}


def compute_metrics_on_cases(cases: Iterable[Tuple], regions_or_labels, ignore_label: Optional[int] = None) -> dict:
    """`cases`: (seg_ref, seg_pred) pairs.  Returns {'metric_per_case', 'mean', 'foreground_mean'} as
    compute_metrics_on_folder does."""
    results = [compute_metrics(ref, pred, regions_or_labels, ignore_label) for ref, pred in cases]
    if not results:
        raise ValueError("no cases")
    return aggregate_metrics(results, regions_or_labels)


def compute_surface_metrics(seg_ref, seg_pred, labels_or_regions, spacing=None, connectivity: int = 1,
                            ignore_label: Optional[int] = None) -> dict:
    """{label_or_region: {'HD', 'HD95', 'ASSD'}}: the surface distances of evaluation/Hausdorff.py and
    evaluation/metrics.py:312-382 (medpy's hd, hd95, assd with the reference's NaN rule) per label or region of two label
    volumes, on the device (surface.py).  Opt-in: nothing else in this module calls it."""
    from . import surface
    return surface.compute_surface_metrics(seg_ref, seg_pred, labels_or_regions, spacing, connectivity, ignore_label)
