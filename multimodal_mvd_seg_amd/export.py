"""Segmentation export after sliding-window inference, on the MI355X.

Mirrors nnunetv2/inference/export_prediction.py:15-67 (`convert_predicted_logits_to_segmentation_with_correct_shape`) and
the part of nnunetv2/preprocessing/resampling/default_resampling.py it calls (`get_do_separate_z`, `get_lowres_axis`,
`compute_new_shape`, `resample_data_or_seg_to_shape` :13-30, :84-214) for the default plans' probabilities resampling:
is_seg=False, order=1, order_z=0.  The reference moves the logits to the host and resizes each of the K channels in fp64
with skimage; here one HIP kernel (csrc/export.hip) interpolates the K channels per output voxel, takes the argmax and
stores the uint8 label at its place in the pre-crop volume, already in the original axis order -- resampling, softmax /
argmax, bbox paste and transpose_backward in a single pass.  There is no CPU path.

Interpolation is pinned to scipy.ndimage (zoom(order=1, mode='nearest', grid_mode=True); for the separate-z axis
map_coordinates(order=0, mode='nearest')), which is what skimage.transform.resize(order=1, mode='edge',
anti_aliasing=False) is understood to call; skimage itself is not available to check against.
"""
import ctypes
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import call, i3

ANISO_THRESHOLD = 3  # nnunetv2/configuration.py

LINEAR, NEAREST = 1, 0


# ------------------------------------------------------------------------------------- default_resampling.py:13-30
def get_do_separate_z(spacing, anisotropy_threshold=ANISO_THRESHOLD) -> bool:
    return bool((np.max(spacing) / np.min(spacing)) > anisotropy_threshold)


def get_lowres_axis(new_spacing) -> np.ndarray:
    return np.where(max(new_spacing) / np.array(new_spacing) == 1)[0]  # the axis (axes) with the largest spacing


def compute_new_shape(old_shape, old_spacing, new_spacing) -> np.ndarray:
    assert len(old_spacing) == len(old_shape)
    assert len(old_shape) == len(new_spacing)
    return np.array([int(round(i / j * k)) for i, j, k in zip(old_spacing, new_spacing, old_shape)])


def determine_separate_z(current_spacing, new_spacing, force_separate_z: Optional[bool] = None,
                         separate_z_anisotropy_threshold: float = ANISO_THRESHOLD) -> Tuple[bool, Optional[int]]:
    """The separate-z decision of resample_data_or_seg_to_shape (:96-124): (do_separate_z, axis).  The out-of-plane axis
    is resampled on its own (order_z) only when exactly one axis carries the largest spacing."""
    if force_separate_z is not None:
        do_separate_z = bool(force_separate_z)
        axis = get_lowres_axis(current_spacing) if force_separate_z else None
    elif get_do_separate_z(current_spacing, separate_z_anisotropy_threshold):
        do_separate_z, axis = True, get_lowres_axis(current_spacing)
    elif get_do_separate_z(new_spacing, separate_z_anisotropy_threshold):
        do_separate_z, axis = True, get_lowres_axis(new_spacing)
    else:
        do_separate_z, axis = False, None
    if axis is not None and len(axis) != 1:
        # 3: every axis has the same spacing; 2: spacings like (0.24, 1.25, 1.25) -- no separate out-of-plane axis
        do_separate_z = False
    return (True, int(axis[0])) if do_separate_z else (False, None)


# ------------------------------------------------------------------------------------- per-axis interpolation tables
def axis_table(n_in: int, n_out: int, mode: int = LINEAR) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(idx0, idx1, weight) of one axis, in fp64: out[o] = (1 - weight[o]) x[idx0[o]] + weight[o] x[idx1[o]].
    Source coordinate c = (o + 0.5) (n_in / n_out) - 0.5 (pixel centres aligned, the scale rounded first as scipy does).
    LINEAR: c clamped to [0, n_in - 1], taps floor(c) and min(floor(c) + 1, n_in - 1).  NEAREST: the single tap
    clamp(floor(c + 0.5), 0, n_in - 1).  n_in == n_out is the identity under both."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError("axis_table: empty axis")
    if mode not in (LINEAR, NEAREST):
        raise NotImplementedError(f"interpolation order {mode}: only order 1 (linear) and order 0 (nearest)")
    o = np.arange(n_out, dtype=np.float64)
    if n_in == n_out:
        idx = np.arange(n_out, dtype=np.int32)
        return idx, idx.copy(), np.zeros(n_out)
    c = (o + 0.5) * (float(n_in) / n_out) - 0.5
    if mode == NEAREST:
        idx = np.clip(np.floor(c + 0.5), 0, n_in - 1).astype(np.int32)
        return idx, idx.copy(), np.zeros(n_out)
    c = np.clip(c, 0.0, n_in - 1.0)
    f = np.floor(c)
    idx0 = f.astype(np.int32)
    idx1 = np.minimum(idx0 + 1, n_in - 1).astype(np.int32)
    return idx0, idx1, c - f


_TABLES = {}


def _device_tables(in_shape, out_shape, modes, device):
    """The three axes' tables concatenated (axis 0 first) as device tensors; weights rounded to fp32 once, here."""
    key = (tuple(in_shape), tuple(out_shape), tuple(modes), str(device))
    hit = _TABLES.get(key)
    if hit is None:
        t = [axis_table(i, o, m) for i, o, m in zip(in_shape, out_shape, modes)]
        hit = tuple(torch.from_numpy(np.ascontiguousarray(np.concatenate([a[j] for a in t]).astype(dt))).to(device)
                    for j, dt in ((0, np.int32), (1, np.int32), (2, np.float32)))
        if len(_TABLES) > 64:
            _TABLES.clear()
        _TABLES[key] = hit
    return hit


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _device_logits(x) -> torch.Tensor:
    if isinstance(x, np.ndarray):
        raise RuntimeError("export runs on the GPU: pass the predictor's device tensor (there is no CPU fallback)")
    if not x.is_cuda:
        raise RuntimeError("export runs on the GPU: the logits must be a device tensor (there is no CPU fallback)")
    if x.dim() != 4:
        raise RuntimeError("logits must be [K, d, h, w]")
    return x.to(torch.float32).contiguous()


def _axis_modes(separate_z_axis: Optional[int]) -> List[int]:
    return [NEAREST if a == separate_z_axis else LINEAR for a in range(3)]


def _check_resampling_kwargs(is_seg, order, order_z):
    if is_seg or order != 1 or order_z != 0:
        raise NotImplementedError(
            f"resample_data_or_seg_to_shape(is_seg={is_seg}, order={order}, order_z={order_z}): the device export covers "
            f"the default plans' probabilities resampling only (is_seg=False, order=1, order_z=0)")


def resample_data_or_seg_to_shape(data: torch.Tensor, new_shape: Sequence[int], current_spacing, new_spacing,
                                  is_seg: bool = False, order: int = 1, order_z: int = 0,
                                  force_separate_z: Optional[bool] = None,
                                  separate_z_anisotropy_threshold: float = ANISO_THRESHOLD) -> torch.Tensor:
    """default_resampling.py:84-130 for a device tensor [K, d, h, w] -> float32 [K, *new_shape] (the input itself when
    the shape does not change, as the reference returns it)."""
    _check_resampling_kwargs(is_seg, order, order_z)
    x = _device_logits(data)
    new_shape = [int(v) for v in new_shape]
    assert len(new_shape) == 3, "new_shape must be 3-D"
    if list(x.shape[1:]) == new_shape:
        return x
    _, axis = determine_separate_z(current_spacing, new_spacing, force_separate_z, separate_z_anisotropy_threshold)
    i0, i1, w = _device_tables(x.shape[1:], new_shape, _axis_modes(axis), x.device)
    out = torch.empty((x.shape[0], *new_shape), dtype=torch.float32, device=x.device)
    call("mvd_export_resize_softmax_f32", _p(x), _p(out), _p(i0), _p(i1), _p(w), x.shape[0], *x.shape[1:], *new_shape,
         i3(new_shape), i3((0, 0, 0)), i3((0, 1, 2)), 0, _stream())
    return out


def resize_logits_to_segmentation(logits: torch.Tensor, new_shape: Sequence[int], shape_before_cropping: Sequence[int],
                                  bbox_lower: Sequence[int], transpose_backward: Sequence[int] = (0, 1, 2),
                                  separate_z_axis: Optional[int] = None, return_probabilities: bool = False,
                                  regions_class_order: Optional[Sequence[int]] = None):
    """The fused core: logits [K, d, h, w] -> uint8 labels of shape shape_before_cropping[transpose_backward] (resized to
    new_shape, argmax, pasted at bbox_lower, axes permuted), and with return_probabilities the float32 [K, ...] softmax
    volume laid out the same way (channel 0 is 1 outside the bbox).
    regions_class_order given (region-based labels, label_handling.py:163-171, :199-205): the K channels are sigmoid heads;
    the label starts at 0 and head i, where its interpolated logit is > 0, writes regions_class_order[i] -- the last
    matching head wins; the probabilities are the sigmoid planes, all 0 outside the bbox."""
    x = _device_logits(logits)
    K = int(x.shape[0])
    if regions_class_order is not None:
        order = [int(c) for c in regions_class_order]
        if len(order) != K:
            raise ValueError(f"regions_class_order has {len(order)} entries for {K} heads")
        if K > 8:
            raise NotImplementedError(f"{K} region heads: the device export holds at most 8")
        if min(order) < 0 or max(order) > 255:
            raise NotImplementedError("region labels outside 0..255 need a uint16 segmentation, which is not built")
    if K > 255:
        raise NotImplementedError("255 or more foreground labels need a uint16 segmentation, which is not built")
    new_shape = [int(v) for v in new_shape]
    full = [int(v) for v in shape_before_cropping]
    lo = [int(v) for v in bbox_lower]
    tb = [int(v) for v in transpose_backward]
    if sorted(tb) != [0, 1, 2]:
        raise ValueError(f"transpose_backward {tb} is not a permutation of the three axes")
    for a in range(3):
        if lo[a] < 0 or lo[a] + new_shape[a] > full[a]:
            raise ValueError(f"bbox [{lo[a]}, {lo[a] + new_shape[a]}) leaves axis {a} of the volume {full}")
    i0, i1, w = _device_tables(x.shape[1:], new_shape, _axis_modes(separate_z_axis), x.device)
    out_shape = [full[a] for a in tb]
    seg = torch.empty(out_shape, dtype=torch.uint8, device=x.device)
    if regions_class_order is not None:
        call("mvd_export_resize_regions_u8", _p(x), _p(seg), _p(i0), _p(i1), _p(w), K, *x.shape[1:], *new_shape, i3(full),
             i3(lo), i3(tb), (ctypes.c_int * K)(*order), _stream())
        if not return_probabilities:
            return seg
        prob = torch.empty((K, *out_shape), dtype=torch.float32, device=x.device)
        call("mvd_export_resize_sigmoid_f32", _p(x), _p(prob), _p(i0), _p(i1), _p(w), K, *x.shape[1:], *new_shape, i3(full),
             i3(lo), i3(tb), _stream())
        return seg, prob
    call("mvd_export_resize_argmax_u8", _p(x), _p(seg), _p(i0), _p(i1), _p(w), K, *x.shape[1:], *new_shape, i3(full),
         i3(lo), i3(tb), _stream())
    if not return_probabilities:
        return seg
    prob = torch.empty((K, *out_shape), dtype=torch.float32, device=x.device)
    call("mvd_export_resize_softmax_f32", _p(x), _p(prob), _p(i0), _p(i1), _p(w), K, *x.shape[1:], *new_shape, i3(full),
         i3(lo), i3(tb), 1, _stream())
    return seg, prob


def convert_predicted_logits_to_segmentation_with_correct_shape(predicted_logits: torch.Tensor, plans_manager,
                                                                configuration_manager, label_manager,
                                                                properties_dict: dict,
                                                                return_probabilities: bool = False,
                                                                num_threads_torch: Optional[int] = None):
    """export_prediction.py:15-67 on the device.  Returns the uint8 segmentation in the original axis order (and the
    float32 probabilities [K, ...] when asked) as device tensors.  `num_threads_torch` is accepted for signature parity;
    no host threads are involved."""
    has_regions = bool(getattr(label_manager, 'has_regions', False))
    if has_regions and label_manager.regions_class_order is None:
        raise RuntimeError("if region-based training is requested then you need to define regions_class_order!")
    if not has_regions and label_manager.num_segmentation_heads - 1 >= 255:
        raise NotImplementedError("255 or more foreground labels need a uint16 segmentation, which is not built")
    shape_after = [int(v) for v in properties_dict['shape_after_cropping_and_before_resampling']]
    if len(shape_after) != 3:
        raise NotImplementedError("3-D cases only")
    spacing = list(configuration_manager.spacing)
    current_spacing = spacing if len(spacing) == len(shape_after) else [properties_dict['spacing'][0], *spacing]
    kwargs = dict(configuration_manager.resampling_fn_probabilities_kwargs)
    _check_resampling_kwargs(kwargs.get('is_seg', False), kwargs.get('order', 1), kwargs.get('order_z', 0))
    _, axis = determine_separate_z(current_spacing, properties_dict['spacing'], kwargs.get('force_separate_z'),
                                   kwargs.get('separate_z_anisotropy_threshold', ANISO_THRESHOLD))
    bbox = properties_dict['bbox_used_for_cropping']
    for (lo, hi), n in zip(bbox, shape_after):
        if int(hi) - int(lo) != n:
            raise ValueError(f"bbox_used_for_cropping {bbox} does not span shape_after_cropping_and_before_resampling "
                             f"{shape_after}")
    return resize_logits_to_segmentation(predicted_logits, shape_after, properties_dict['shape_before_cropping'],
                                         [b[0] for b in bbox], plans_manager.transpose_backward, axis,
                                         return_probabilities,
                                         label_manager.regions_class_order if has_regions else None)


def resample_logits_for_next_stage(predicted_logits: torch.Tensor, target_shape: Sequence[int], configuration_manager,
                                   label_manager=None) -> torch.Tensor:
    """export_prediction.py:109-141 (resample_and_save) without the file: the logits [K, d, h, w] of a stage that has
    next_stage_names, resampled to the next stage's preprocessed shape with the configuration's probability resampling
    and arg-maxed to uint8 [target_shape] -- what the next stage loads as its previous-stage segmentation.  No bbox paste
    and no transpose: the result stays in preprocessed axis order.  As in the reference, current and target spacing are
    both the configuration's own spacing, which is what decides the separate-z axis."""
    if label_manager is not None and getattr(label_manager, 'has_regions', False):
        raise NotImplementedError("cascade with region-based labels: the next-stage export is built for plain labels")
    target_shape = [int(v) for v in target_shape]
    if len(target_shape) != 3:
        raise NotImplementedError("3-D cases only")
    spacing = list(configuration_manager.spacing)
    if len(spacing) != 3:
        raise NotImplementedError("the next-stage export needs a 3-D configuration spacing")
    kwargs = dict(configuration_manager.resampling_fn_probabilities_kwargs)
    _check_resampling_kwargs(kwargs.get('is_seg', False), kwargs.get('order', 1), kwargs.get('order_z', 0))
    _, axis = determine_separate_z(spacing, spacing, kwargs.get('force_separate_z'),
                                   kwargs.get('separate_z_anisotropy_threshold', ANISO_THRESHOLD))
    return resize_logits_to_segmentation(predicted_logits, target_shape, target_shape, (0, 0, 0), (0, 1, 2), axis)
