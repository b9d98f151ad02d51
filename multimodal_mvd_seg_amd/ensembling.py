"""Model ensembling on the MI355X.

Mirrors nnunetv2/ensembling/ensemble.py (`average_probabilities` :17-29, `merge_files` :32-46,
`ensemble_crossvalidations` :128-206) without the files and worker pools: every function takes device tensors, like
export.py.  Two routes lead to an ensembled segmentation:

* stored probabilities -- `average_probabilities` / `merge_probabilities` / `ensemble_crossvalidations`: the members'
  softmax volumes at the original image shape are averaged in the reference's order (avg = p_0; avg += p_m; avg /= M)
  and arg-maxed by one streaming kernel (mvd_ensemble_mean_argmax);
* logits -- `ensemble_predictions`: every member's logits are interpolated to the original shape, soft-maxed and
  accumulated in registers by ONE launch (mvd_export_ensemble_argmax_u8); the members' K x D x H x W probability volumes
  are never written.  Bit-identical to the first route fed by export.resize_logits_to_segmentation(return_probabilities=
  True) per member.

Plain labels only.  There is no CPU path.
"""
import ctypes
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import export
from ._lib import call, i3

MAX_MEMBERS = 8   # ENS_MMAX of csrc/export.hip
MAX_HEADS = 8     # ENS_KMAX: the per-lane accumulators are K floats in registers (the cap of REGION_KMAX)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _refuse_regions(label_manager, what):
    if label_manager is not None and bool(getattr(label_manager, 'has_regions', False)):
        raise NotImplementedError(
            f"{what} with region-based labels: merge_files pushes the MEAN PROBABILITIES through the sigmoid again and "
            f"thresholds at 0.5, which turns every head with a positive mean on; there is nothing sane to be faithful to, "
            f"so ensembling is built for plain labels only")


def _check_counts(M, K, what):
    if M < 1:
        raise ValueError(f"{what}: at least one member must be given")
    if M > MAX_MEMBERS:
        raise NotImplementedError(f"{what}: {M} members: the device ensemble holds at most {MAX_MEMBERS}")
    if K - 1 >= 255:
        raise NotImplementedError("255 or more foreground labels need a uint16 segmentation, which is not built")
    if K > MAX_HEADS:
        raise NotImplementedError(f"{what}: {K} heads: the device ensemble keeps K accumulators per lane in registers and "
                                  f"holds at most {MAX_HEADS}")


def _device_probabilities(list_of_probabilities, what) -> List[torch.Tensor]:
    members = list(list_of_probabilities)
    assert len(members), 'At least one volume must be given in list_of_probabilities'
    shape0 = tuple(members[0].shape)
    for m, x in enumerate(members):
        if len(x.shape) < 2:
            raise RuntimeError(f"{what}: member {m} must be [K, ...]")
        if x.shape[0] != shape0[0]:
            raise ValueError(f"{what}: member {m} has {x.shape[0]} channels, member 0 has {shape0[0]}: members whose K "
                             f"differ cannot be averaged")
        if tuple(x.shape) != shape0:
            raise ValueError(f"{what}: member {m} has shape {tuple(x.shape)}, member 0 {shape0}")
    _check_counts(len(members), int(shape0[0]), what)
    out = []
    for m, x in enumerate(members):
        if isinstance(x, np.ndarray) or not torch.is_tensor(x) or not x.is_cuda:
            raise RuntimeError(f"{what} runs on the GPU: member {m} must be a device tensor (there is no CPU fallback)")
        if x.device != members[0].device:
            raise ValueError(f"{what}: member {m} is on {x.device}, member 0 on {members[0].device}")
        out.append(x.to(torch.float32).contiguous())   # ensemble.py:24-25: other dtypes are raised to fp32 first
    return out


def _mean_argmax(members: List[torch.Tensor], want_mean: bool):
    K = int(members[0].shape[0])
    n = members[0].numel() // K
    if n < 1:
        raise ValueError("ensemble: empty volume")
    seg = torch.empty(tuple(members[0].shape[1:]), dtype=torch.uint8, device=members[0].device)
    mean = torch.empty_like(members[0]) if want_mean else None
    ptrs = (ctypes.c_void_p * len(members))(*[x.data_ptr() for x in members])
    call("mvd_ensemble_mean_argmax", ptrs, len(members), K, n, _p(seg), _p(mean) if want_mean else None, _stream())
    return seg, mean


def average_probabilities(list_of_probabilities: Sequence[torch.Tensor]) -> torch.Tensor:
    """ensemble.py:17-29 for device tensors [K, ...] instead of .npz files: avg = p_0 (raised to fp32 when it is not),
    avg += p_m for m ascending, avg /= M, in fp32 and in that order.  Returns a new float32 tensor."""
    return _mean_argmax(_device_probabilities(list_of_probabilities, "average_probabilities"), True)[1]


def merge_probabilities(list_of_probabilities: Sequence[torch.Tensor], label_manager, save_probabilities: bool = False):
    """`merge_files` (ensemble.py:32-46) without the files: the uint8 segmentation of the averaged probabilities and,
    with save_probabilities, the float32 mean itself.  The reference calls `convert_logits_to_segmentation` on the
    averaged probabilities, i.e. a second softmax before the argmax; a softmax is monotone, so that product is the
    argmax of the mean, which is what is computed here (the first index wins an exact tie, as argmax does)."""
    _refuse_regions(label_manager, "merge_probabilities")
    members = _device_probabilities(list_of_probabilities, "merge_probabilities")
    heads = getattr(label_manager, 'num_segmentation_heads', None)
    if heads is not None and int(heads) != int(members[0].shape[0]):
        raise ValueError(f"merge_probabilities: the volumes have {members[0].shape[0]} channels, the label manager "
                         f"{heads} segmentation heads")
    seg, mean = _mean_argmax(members, save_probabilities)
    return (seg, mean) if save_probabilities else seg


def ensemble_predictions(members, plans_manager, label_manager, properties_dict: dict,
                         return_probabilities: bool = False):
    """The fused ensemble export.  `members` is a list of (logits [K, d, h, w], configuration_manager); the members may
    come from different configurations (2d, 3d_fullres, cascade) and so have different extents and spacings.  Per member
    the property and kwargs checks and the separate-z decision are those of
    export.convert_predicted_logits_to_segmentation_with_correct_shape; the output geometry (shape before resampling,
    bbox, pre-crop volume, transpose_backward) is the case's and is shared.  One launch then gives the uint8
    segmentation in the original axis order and, when asked, the float32 mean probabilities [K, ...] (channel 0 is 1
    outside the bbox) -- what export per member with return_probabilities followed by merge_probabilities gives, bit
    for bit."""
    _refuse_regions(label_manager, "ensemble_predictions")
    members = list(members)
    if not members:
        raise ValueError("ensemble_predictions: at least one member must be given")
    heads = int(label_manager.num_segmentation_heads)
    _check_counts(len(members), heads, "ensemble_predictions")
    shape_after = [int(v) for v in properties_dict['shape_after_cropping_and_before_resampling']]
    if len(shape_after) != 3:
        raise NotImplementedError("3-D cases only")
    bbox = properties_dict['bbox_used_for_cropping']
    for (lo, hi), n in zip(bbox, shape_after):
        if int(hi) - int(lo) != n:
            raise ValueError(f"bbox_used_for_cropping {bbox} does not span shape_after_cropping_and_before_resampling "
                             f"{shape_after}")
    xs, axes = [], []
    for m, (logits, configuration_manager) in enumerate(members):
        if len(logits.shape) != 4:
            raise RuntimeError(f"ensemble_predictions: member {m}'s logits must be [K, d, h, w]")
        if int(logits.shape[0]) != heads:
            raise ValueError(f"ensemble_predictions: member {m} has {logits.shape[0]} heads, the label manager {heads}: "
                             f"members whose K differ cannot be averaged")
        spacing = list(configuration_manager.spacing)
        current_spacing = spacing if len(spacing) == len(shape_after) else [properties_dict['spacing'][0], *spacing]
        kwargs = dict(configuration_manager.resampling_fn_probabilities_kwargs)
        export._check_resampling_kwargs(kwargs.get('is_seg', False), kwargs.get('order', 1), kwargs.get('order_z', 0))
        _, axis = export.determine_separate_z(current_spacing, properties_dict['spacing'], kwargs.get('force_separate_z'),
                                              kwargs.get('separate_z_anisotropy_threshold', export.ANISO_THRESHOLD))
        xs.append(logits)
        axes.append(axis)
    for m, logits in enumerate(xs):
        if isinstance(logits, np.ndarray) or not torch.is_tensor(logits) or not logits.is_cuda:
            raise RuntimeError(f"ensemble_predictions runs on the GPU: member {m}'s logits must be a device tensor (there "
                               f"is no CPU fallback)")
    return ensemble_logits_to_segmentation(xs, shape_after, properties_dict['shape_before_cropping'],
                                           [b[0] for b in bbox], plans_manager.transpose_backward, axes,
                                           return_probabilities)


def ensemble_logits_to_segmentation(list_of_logits: Sequence[torch.Tensor], new_shape: Sequence[int],
                                    shape_before_cropping: Sequence[int], bbox_lower: Sequence[int],
                                    transpose_backward: Sequence[int] = (0, 1, 2),
                                    separate_z_axes: Optional[Sequence[Optional[int]]] = None,
                                    return_probabilities: bool = False):
    """The fused core under `ensemble_predictions` (export.resize_logits_to_segmentation for M members): member m's logits
    [K, d_m, h_m, w_m] are resized to new_shape with its own tables (separate_z_axes[m]: its nearest-neighbour axis or
    None), soft-maxed and averaged; the argmax is pasted at bbox_lower into shape_before_cropping and the axes permuted."""
    members = list(list_of_logits)
    if not members:
        raise ValueError("ensemble: at least one member must be given")
    K = int(members[0].shape[0])
    for m, x in enumerate(members):
        if len(x.shape) != 4:
            raise RuntimeError(f"ensemble: member {m}'s logits must be [K, d, h, w]")
        if int(x.shape[0]) != K:
            raise ValueError(f"ensemble: member {m} has {x.shape[0]} heads, member 0 has {K}: members whose K differ "
                             f"cannot be averaged")
    _check_counts(len(members), K, "ensemble")
    if K < 2:
        raise ValueError("ensemble: a softmax ensemble needs at least 2 heads")
    for m, x in enumerate(members):
        if isinstance(x, np.ndarray) or not torch.is_tensor(x) or not x.is_cuda:
            raise RuntimeError(f"the ensemble export runs on the GPU: member {m}'s logits must be a device tensor (there "
                               f"is no CPU fallback)")
        if x.device != members[0].device:
            raise ValueError(f"ensemble: member {m} is on {x.device}, member 0 on {members[0].device}")
    xs = [export._device_logits(x) for x in members]
    M = len(xs)
    axes = [None] * M if separate_z_axes is None else list(separate_z_axes)
    if len(axes) != M:
        raise ValueError(f"ensemble: {len(axes)} separate-z axes for {M} members")
    new_shape = [int(v) for v in new_shape]
    full = [int(v) for v in shape_before_cropping]
    lo = [int(v) for v in bbox_lower]
    tb = [int(v) for v in transpose_backward]
    if sorted(tb) != [0, 1, 2]:
        raise ValueError(f"transpose_backward {tb} is not a permutation of the three axes")
    for a in range(3):
        if lo[a] < 0 or lo[a] + new_shape[a] > full[a]:
            raise ValueError(f"bbox [{lo[a]}, {lo[a] + new_shape[a]}) leaves axis {a} of the volume {full}")
    dev = xs[0].device
    tables = [export._device_tables(x.shape[1:], new_shape, export._axis_modes(ax), dev) for x, ax in zip(xs, axes)]
    out_shape = [full[a] for a in tb]
    seg = torch.empty(out_shape, dtype=torch.uint8, device=dev)
    mean = torch.empty((K, *out_shape), dtype=torch.float32, device=dev) if return_probabilities else None
    arr = ctypes.c_void_p * M
    dims = (ctypes.c_int * (3 * M))(*[int(v) for x in xs for v in x.shape[1:]])
    call("mvd_export_ensemble_argmax_u8", arr(*[x.data_ptr() for x in xs]), arr(*[t[0].data_ptr() for t in tables]),
         arr(*[t[1].data_ptr() for t in tables]), arr(*[t[2].data_ptr() for t in tables]), dims, M, K, *new_shape,
         i3(full), i3(lo), i3(tb), _p(seg), _p(mean) if return_probabilities else None, _stream())
    return (seg, mean) if return_probabilities else seg


def ensemble_crossvalidations(per_model_predictions: Sequence, label_manager, save_probabilities: bool = False) -> Dict:
    """`ensemble_crossvalidations` (ensemble.py:128-206) over in-memory predictions.  `per_model_predictions` has one
    entry per trained model: either a dict {case: probabilities [K, ...]} or, as the reference walks fold_0 ...
    fold_4/validation, a list of such dicts, one per fold.  The checks of :139-179: every model must hold every case that
    any model holds (RuntimeError naming what is missing), and no case may appear in more than one fold of a model
    (AssertionError).  Then `merge_probabilities` per case, members in model order.  Returns {case: segmentation}, or
    {case: (segmentation, mean)} with save_probabilities."""
    _refuse_regions(label_manager, "ensemble_crossvalidations")
    models = list(per_model_predictions)
    if not models:
        raise ValueError("ensemble_crossvalidations: at least one model must be given")
    if len(models) > MAX_MEMBERS:
        raise NotImplementedError(f"ensemble_crossvalidations: {len(models)} models: the device ensemble holds at most "
                                  f"{MAX_MEMBERS}")
    folds_per_model = [[m] if isinstance(m, dict) else list(m) for m in models]
    unique_cases = []
    for folds in folds_per_model:
        for fold in folds:
            if len(fold) == 0:
                raise RuntimeError("a fold without predictions: every requested fold of every model must be validated "
                                   "with its probabilities kept")
            for case in fold:
                if case not in unique_cases:
                    unique_cases.append(case)
    for i, folds in enumerate(folds_per_model):
        here = set()
        for fold in folds:
            here.update(fold.keys())
        missing = [c for c in unique_cases if c not in here]
        if missing:
            raise RuntimeError(f"model {i} does not seem to contain all predictions. Missing: {missing}")
    mapping = []
    for i, folds in enumerate(folds_per_model):
        mapping.append({})
        for fold in folds:
            for case, prob in fold.items():
                assert case not in mapping[-1], f"Duplicate detected. Case {case} is present in more than one fold of " \
                                                f"model {i}."
                mapping[-1][case] = prob
    return {case: merge_probabilities([fm[case] for fm in mapping], label_manager, save_probabilities)
            for case in unique_cases}
