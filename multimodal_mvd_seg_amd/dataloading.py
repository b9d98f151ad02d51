"""On-device training feed for case volumes resident in HBM (the deterministic part).

Host-side mirror of nnUNetDataLoader3D (nnunetv2/training/dataloading/data_loader_3d.py:6-48) and of its base class
(base_data_loader.py:10-139): same constructor arguments, same numpy RNG call order for the case selection
(batchgenerators DataLoader.get_indices: np.random.choice with replacement), the oversampling rule and get_bbox, so a
seeded run picks the boxes the reference loader picks.  What the reference then does on 12 CPU worker processes --
crop, pad (data 0 / seg -1), MirrorTransform, RemoveLabelTransform(-1, 0), DownsampleSegForDSTransform2 and
NumpyToTensor('float') (nnUNetTrainer.py:738-768) -- runs here as three HIP kernels through the C ABI
(csrc/feed.hip) on volumes that stay in HBM (288 GB holds a whole preprocessed dataset); there is no CPU fallback.
The rotation / scaling SpatialTransform (:703-714) runs on the device too when the loader is given `rotation_for_DA`
(csrc/feed_spatial.hip): its resampling is pinned to scipy.ndimage, its batchgenerators glue (draws,
coordinate mesh, rotation matrices) is restated.  The intensity augmentations (:719-736: noise, blur, brightness,
contrast, low-resolution simulation, the two gammas) and MaskTransform run on the device when the loader is given
`intensity_augmentation=True` / `mask_channels` (csrc/feed_intensity.hip): their numeric cores are pinned to
numpy / scipy.ndimage, their batchgenerators glue (which values are drawn, in which order) is restated in
`draw_intensity`.  Anisotropic plans (`do_dummy_2d_data_aug=True`, nnUNetTrainer.py:695-717) take the in-plane form of both
stages: one 2-D map per sample moves every slice of every channel, and the low-resolution simulation leaves axis 0 alone
(DESIGN 19).  `da5=True` runs nnUNetTrainerDA5's recipe instead of the default one (csrc/feed_da5.hip): per-axis
scaling, Rot90 / Transpose / mirror as signed permutations, an exact median filter, blank rectangles, the local
brightness gradient and gamma, sharpening; its glue is restated in `draw_da5`.
"""
import ctypes

import numpy as np
import torch

from ._lib import call, query


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def crop_pad_data(vol, out, bbox_lbs, flip_mask=0, pad=0.0):
    """out[C,pd,ph,pw] (float32, device) <- pad(vol[:, lb:lb+patch]) mirrored on the axes of flip_mask."""
    C, D, H, W = vol.shape
    pd, ph, pw = out.shape[1:]
    if not (vol.is_cuda and out.is_cuda and vol.dtype == torch.float32 and out.dtype == torch.float32
            and vol.is_contiguous() and out.is_contiguous() and out.shape[0] == C):
        raise RuntimeError("crop_pad_data: contiguous float32 device tensors [C,D,H,W] -> [C,pd,ph,pw]")
    call("mvd_feed_crop_pad_f32", _p(vol), _p(out), C, D, H, W, pd, ph, pw, int(bbox_lbs[0]), int(bbox_lbs[1]),
         int(bbox_lbs[2]), int(flip_mask), float(pad), _stream())


def crop_pad_seg(seg, out, bbox_lbs, flip_mask=0, pad=-1, replace=None):
    """int16 seg [C,D,H,W] -> float32 target; replace=(from, to) applies RemoveLabelTransform after the padding."""
    C, D, H, W = seg.shape
    pd, ph, pw = out.shape[1:]
    if not (seg.is_cuda and out.is_cuda and seg.dtype == torch.int16 and out.dtype == torch.float32
            and seg.is_contiguous() and out.is_contiguous() and out.shape[0] == C):
        raise RuntimeError("crop_pad_seg: contiguous int16 -> float32 device tensors [C,D,H,W] -> [C,pd,ph,pw]")
    rf, rt = (replace if replace is not None else (0, 0))
    call("mvd_feed_crop_pad_seg_i16", _p(seg), _p(out), C, D, H, W, pd, ph, pw, int(bbox_lbs[0]), int(bbox_lbs[1]),
         int(bbox_lbs[2]), int(flip_mask), int(pad), int(replace is not None), int(rf), int(rt), _stream())


def downsample_seg(target, scale):
    """DownsampleSegForDSTransform2 (deep_supervision_donwsampling.py:33-53), order 0: [B,C,D,H,W] float32 ->
    [B,C,round(D*s0),round(H*s1),round(W*s2)]."""
    if not isinstance(scale, (tuple, list)):
        scale = [scale] * 3
    if all(s == 1 for s in scale):
        return target
    B, C, D, H, W = target.shape
    new = np.round(np.array([D, H, W], dtype=float) * np.array(scale, dtype=float)).astype(int)
    out = torch.empty((B, C, int(new[0]), int(new[1]), int(new[2])), dtype=torch.float32, device=target.device)
    if not (target.is_cuda and target.dtype == torch.float32 and target.is_contiguous()):
        raise RuntimeError("downsample_seg: contiguous float32 device tensor")
    call("mvd_feed_downsample_seg", _p(target), _p(out), B * C, D, H, W, int(new[0]), int(new[1]), int(new[2]), _stream())
    return out


def rotation_matrix_3d(ax, ay, az):
    """R = Rx(ax) Ry(ay) Rz(az) (batchgenerators create_matrix_rotation_{x,y,z}_3d applied to the identity in turn;
    rotate_coords_3d multiplies a coordinate ROW vector by R)."""
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return np.identity(3).dot(rx).dot(ry).dot(rz)


def get_patch_size(final_patch_size, rot_x, rot_y, rot_z, scale_range):
    """Initial patch that still covers the final one after the largest rotation about each axis and the smallest
    scaling (data_augmentation/compute_initial_patch_size.py, 3-D and 2-D branches)."""
    def _max_abs(r):
        return max(np.abs(r)) if isinstance(r, (tuple, list)) else r
    rot_x, rot_y, rot_z = (min(90 / 360 * 2. * np.pi, _max_abs(r)) for r in (rot_x, rot_y, rot_z))
    coords = np.array(final_patch_size)
    final_shape = np.copy(coords)
    if len(coords) == 3:
        for angles in ((rot_x, 0, 0), (0, rot_y, 0), (0, 0, rot_z)):
            final_shape = np.max(np.vstack((np.abs(np.dot(coords, rotation_matrix_3d(*angles))), final_shape)), 0)
    elif len(coords) == 2:
        rot = np.array([[np.cos(rot_x), -np.sin(rot_x)], [np.sin(rot_x), np.cos(rot_x)]])
        final_shape = np.max(np.vstack((np.abs(np.dot(coords, rot)), final_shape)), 0)
    final_shape = final_shape / min(scale_range)
    return final_shape.astype(int)


def spatial_affine(spatial, patch_size):
    """The 12 doubles of the kernels' coordinate map p = A (o - (f-1)/2) + off for spatial = (ax, ay, az, sc): A = sc R^T
    (augment_spatial: rotate_coords_3d, then scale_coords, then + ctr), off = n/2 - 0.5 (random_crop=False).  sc may be
    one factor per axis (independent_scale_for_each_axis, the DA5 recipe): scale_coords multiplies coordinate i by sc_i,
    so row i of R^T is scaled by sc_i."""
    ax, ay, az, sc = spatial
    if np.ndim(sc) == 0:
        a = sc * rotation_matrix_3d(ax, ay, az).T
    else:
        if len(sc) != 3:
            raise ValueError("spatial_affine: a per-axis scale has three factors")
        a = np.asarray(sc, dtype=np.float64)[:, None] * rotation_matrix_3d(ax, ay, az).T
    off = np.asarray(patch_size, dtype=np.float64) / 2. - 0.5
    return [float(v) for v in a.reshape(-1)] + [float(v) for v in off]


def rotation_matrix_2d(a):
    """batchgenerators create_matrix_rotation_2d; rotate_coords_2d multiplies a coordinate ROW vector (y, x) by it."""
    return np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])


def spatial_affine_2d(spatial, patch_size_2d):
    """The 6 doubles of the in-plane map p = A (o - (f-1)/2) + off of the dummy 2-D mode for spatial = (a_x, 0, 0, sc)
    (augment_spatial, dim == 2: rotate_coords_2d, scale_coords, + ctr): A = sc R^T, off = n/2 - 0.5 over (H, W).  The
    lower-right 2x2 block of spatial_affine((a_x, 0, 0, sc)): axis 0 stays the identity."""
    ax, ay, az, sc = spatial
    if ay != 0 or az != 0:
        raise ValueError("spatial_affine_2d: the in-plane map only rotates about axis 0 (a_y = a_z = 0)")
    if len(patch_size_2d) != 2:
        raise ValueError("spatial_affine_2d: patch_size_2d is (H, W)")
    a = sc * rotation_matrix_2d(ax).T
    off = np.asarray(patch_size_2d, dtype=np.float64) / 2. - 0.5
    return [float(v) for v in a.reshape(-1)] + [float(v) for v in off]


def _affine_arg(affine, n=12):
    vals = [float(v) for v in affine]
    if len(vals) != n:
        raise ValueError(f"affine: {n} values (A row-major, then the offset)")
    return (ctypes.c_double * n)(*vals)


def bspline_prefilter(patch, axis_mask=7):
    """In place: scipy.ndimage.spline_filter1d(order=3, mode='mirror') of every channel of patch [C,D,H,W] along the
    axes of axis_mask (bit 0: D, 1: H, 2: W)."""
    if not (patch.is_cuda and patch.dtype == torch.float32 and patch.is_contiguous() and patch.dim() == 4):
        raise RuntimeError("bspline_prefilter: contiguous float32 device tensor [C,D,H,W]")
    call("mvd_feed_bspline_prefilter_f32", _p(patch), *[int(v) for v in patch.shape], int(axis_mask), _stream())


def spatial_transform_data(coef, out, affine, flip_mask=0, cval=0.0):
    """out[C,fd,fh,fw] <- map_coordinates(order=3, mode='constant', cval) of the PREFILTERED patch coef[C,D,H,W] at
    p = A (o - (f-1)/2) + off (affine: A row-major, then off), mirrored on the axes of flip_mask."""
    if not (coef.is_cuda and out.is_cuda and coef.dtype == torch.float32 and out.dtype == torch.float32
            and coef.is_contiguous() and out.is_contiguous() and coef.dim() == 4 and out.dim() == 4
            and out.shape[0] == coef.shape[0]):
        raise RuntimeError("spatial_transform_data: contiguous float32 device tensors [C,D,H,W] -> [C,fd,fh,fw]")
    call("mvd_feed_warp_data_f32", _p(coef), _p(out), *[int(v) for v in coef.shape], *[int(v) for v in out.shape[1:]],
         _affine_arg(affine), int(flip_mask), float(cval), _stream())


def spatial_transform_seg(seg, out, affine, flip_mask=0, replace=None):
    """out[C,fd,fh,fw] <- interpolate_img(order=1, mode='constant', cval=-1, is_seg=True) of the float32 label patch
    seg[C,D,H,W] at the same coordinates; replace=(from, to) applies RemoveLabelTransform after the vote."""
    if not (seg.is_cuda and out.is_cuda and seg.dtype == torch.float32 and out.dtype == torch.float32
            and seg.is_contiguous() and out.is_contiguous() and seg.dim() == 4 and out.dim() == 4
            and out.shape[0] == seg.shape[0]):
        raise RuntimeError("spatial_transform_seg: contiguous float32 device tensors [C,D,H,W] -> [C,fd,fh,fw]")
    rf, rt = (replace if replace is not None else (0, 0))
    call("mvd_feed_warp_seg", _p(seg), _p(out), *[int(v) for v in seg.shape], *[int(v) for v in out.shape[1:]],
         _affine_arg(affine), int(flip_mask), int(replace is not None), int(rf), int(rt), _stream())


def _check_2d_pair(src, out, name):
    if not (src.is_cuda and out.is_cuda and src.dtype == torch.float32 and out.dtype == torch.float32
            and src.is_contiguous() and out.is_contiguous() and src.dim() == 4 and out.dim() == 4
            and out.shape[0] == src.shape[0] and out.shape[1] == src.shape[1]):
        raise RuntimeError(f"{name}: contiguous float32 device tensors [C,D,H,W] -> [C,D,fh,fw] (axis 0 keeps its size)")


def spatial_transform_data_2d(coef, out, affine, flip_mask=0, cval=0.0):
    """out[C,D,fh,fw] <- per slice (c, z) the 2-D map_coordinates(order=3, mode='constant', cval) of the IN-PLANE
    prefiltered patch coef[C,D,H,W] (bspline_prefilter(..., 6)) at p = A (o - (f-1)/2) + off (affine: 6 values, A 2x2
    row-major, then off), mirrored on the axes of the 3-bit flip_mask (bit 0 flips the slice index)."""
    _check_2d_pair(coef, out, "spatial_transform_data_2d")
    call("mvd_feed_warp2d_data_f32", _p(coef), _p(out), *[int(v) for v in coef.shape], *[int(v) for v in out.shape[2:]],
         _affine_arg(affine, 6), int(flip_mask), float(cval), _stream())


def spatial_transform_seg_2d(seg, out, affine, flip_mask=0, replace=None):
    """out[C,D,fh,fw] <- per slice the 2-D interpolate_img(order=1, mode='constant', cval=-1, is_seg=True) of the float32
    label patch seg[C,D,H,W] at the same coordinates; replace=(from, to) applies RemoveLabelTransform after the vote."""
    _check_2d_pair(seg, out, "spatial_transform_seg_2d")
    rf, rt = (replace if replace is not None else (0, 0))
    call("mvd_feed_warp2d_seg", _p(seg), _p(out), *[int(v) for v in seg.shape], *[int(v) for v in out.shape[2:]],
         _affine_arg(affine, 6), int(flip_mask), int(replace is not None), int(rf), int(rt), _stream())


def _dev_f32(t, name, dim=4):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == dim):
        raise RuntimeError(f"{name}: contiguous float32 device tensor of {dim} dims")


def _chmask(C, channels):
    if C > 16:
        raise ValueError("intensity kernels take at most 16 channels")
    if channels is None:
        return (1 << C) - 1
    m = 0
    for c in channels:
        if not 0 <= int(c) < C:
            raise ValueError(f"channel {c} out of range for {C} channels")
        m |= 1 << int(c)
    return m


def _chan_arg(vals, C, ctype=ctypes.c_float):
    vals = [0.0 if v is None else float(v) for v in vals]
    if len(vals) != C:
        raise ValueError(f"one value per channel ({C}) expected, got {len(vals)}")
    return (ctype * C)(*vals)


STAT_MEAN, STAT_STD, STAT_MIN, STAT_MAX = range(4)
OP_BRIGHTNESS, OP_CONTRAST, OP_GAMMA, OP_GAMMA_INVERTED, OP_CLIP = range(5)
LOWRES_PAD = 12  # scipy zoom's edge pad in front of the order-3 prefilter (_prepad_for_spline_filter, mode 'nearest')


def stats_workspace(C, device):
    """The first-level partials buffer of channel_stats (float64, on `device`)."""
    nbytes = int(query("mvd_feed_stats_workspace_bytes", int(C)))
    return torch.empty(nbytes // 8, dtype=torch.float64, device=device)


def channel_stats(x, stats, ws, channels=None, pre_op=0, gammas=None, pre_stats=None):
    """stats[c] <- (mean, std (ddof 0), min, max) in fp64 of each selected channel of x [C,D,H,W], or of its gamma map
    (pre_op OP_GAMMA / OP_GAMMA_INVERTED, gammas per channel, pre_stats = the channel's own stats).  Deterministic."""
    _dev_f32(x, "channel_stats")
    C = int(x.shape[0])
    if not (stats.is_cuda and stats.dtype == torch.float64 and stats.numel() >= 4 * C and stats.is_contiguous()):
        raise RuntimeError("channel_stats: stats is a contiguous float64 device tensor of >= 4 C values")
    if not (ws.is_cuda and ws.dtype == torch.float64 and ws.numel() * 8 >= query("mvd_feed_stats_workspace_bytes", C)):
        raise RuntimeError("channel_stats: ws too small (stats_workspace)")
    if pre_op and (pre_stats is None or gammas is None or pre_stats.dtype != torch.float64 or pre_stats.numel() < 4 * C):
        raise RuntimeError("channel_stats: the gamma map needs gammas and float64 pre_stats")
    call("mvd_feed_channel_stats_f32", _p(x), _p(stats), _p(ws), C, x[0].numel(), _chmask(C, channels), int(pre_op),
         _chan_arg(gammas, C) if pre_op else None, _p(pre_stats) if pre_op else None, _stream())


def intensity_apply(x, op, params=None, stats_a=None, stats_b=None, channels=None):
    """In place on the selected channels of x [C,D,H,W]: OP_BRIGHTNESS x *= p; OP_CONTRAST clip((x - mean) p + mean, min,
    max) with stats_a; OP_GAMMA / OP_GAMMA_INVERTED augment_gamma(retain_stats=True) with gamma p (stats_a of x,
    stats_b of its gamma map); OP_CLIP clip(x, min, max) of stats_a."""
    _dev_f32(x, "intensity_apply")
    C = int(x.shape[0])
    for st in (stats_a, stats_b):
        if st is not None and not (st.is_cuda and st.dtype == torch.float64 and st.numel() >= 4 * C):
            raise RuntimeError("intensity_apply: stats are float64 device tensors of >= 4 C values")
    call("mvd_feed_intensity_apply_f32", _p(x), C, x[0].numel(), _chmask(C, channels), int(op),
         _chan_arg(params, C) if params is not None else None, _p(stats_a) if stats_a is not None else None,
         _p(stats_b) if stats_b is not None else None, _stream())


def gaussian_blur(x, sigmas, ws):
    """In place: scipy.ndimage.gaussian_filter(x[c], sigmas[c]) (mode 'reflect', truncate 4) for every channel of x
    [C,D,H,W] whose sigma is not None; ws: float32 device scratch of >= 2 * (selected channels) * D*H*W values."""
    _dev_f32(x, "gaussian_blur")
    C = int(x.shape[0])
    nsel = sum(s is not None for s in sigmas)
    if not (ws.is_cuda and ws.dtype == torch.float32 and ws.is_contiguous() and ws.numel() >= 2 * nsel * x[0].numel()):
        raise RuntimeError("gaussian_blur: ws is a float32 device tensor of >= 2 * selected * D*H*W values")
    if any(s is not None and not 0 < float(s) <= 1.1 for s in sigmas):
        raise ValueError("gaussian_blur: 0 < sigma <= 1.1")
    call("mvd_feed_gaussian_blur_f32", _p(x), _p(ws), C, *[int(v) for v in x.shape[1:]],
         _chan_arg(sigmas, C, ctypes.c_double), _stream())


def gaussian_blur_wide(x, sigmas, ws):
    """gaussian_blur for 0 < sigma <= 1.5 (radius int(4 sigma + 0.5) <= 6, the DA5 range): the same arithmetic."""
    _dev_f32(x, "gaussian_blur_wide")
    C = int(x.shape[0])
    nsel = sum(s is not None for s in sigmas)
    if not (ws.is_cuda and ws.dtype == torch.float32 and ws.is_contiguous() and ws.numel() >= 2 * nsel * x[0].numel()):
        raise RuntimeError("gaussian_blur_wide: ws is a float32 device tensor of >= 2 * selected * D*H*W values")
    if any(s is not None and not 0 < float(s) <= 1.5 for s in sigmas):
        raise ValueError("gaussian_blur_wide: 0 < sigma <= 1.5")
    call("mvd_feed_gaussian_blur_wide_f32", _p(x), _p(ws), C, *[int(v) for v in x.shape[1:]],
         _chan_arg(sigmas, C, ctypes.c_double), _stream())


OP_DA5_ADD, OP_DA5_CONTRAST_NOCLIP = range(2)
LOCAL_ADDITIVE, LOCAL_GAMMA = range(2)


def da5_apply(x, op, params, stats=None, channels=None):
    """In place on the selected channels of x [C,D,H,W]: OP_DA5_ADD x += p (BrightnessTransform); OP_DA5_CONTRAST_NOCLIP
    (x - mean) p + mean with stats (ContrastAugmentationTransform, preserve_range=False)."""
    _dev_f32(x, "da5_apply")
    C = int(x.shape[0])
    if stats is not None and not (stats.is_cuda and stats.dtype == torch.float64 and stats.numel() >= 4 * C):
        raise RuntimeError("da5_apply: stats is a float64 device tensor of >= 4 C values")
    call("mvd_feed_da5_apply_f32", _p(x), C, x[0].numel(), _chmask(C, channels), int(op), _chan_arg(params, C),
         _p(stats) if stats is not None else None, _stream())


def median_filter(x, out, sizes):
    """out[c] <- scipy.ndimage.median_filter(x[c], size=sizes[c]) (mode 'reflect') for sizes 2..7, exactly; a size of
    0 / None copies the channel.  x, out [C,D,H,W], distinct buffers.  Finite inputs (NaN is unsupported)."""
    _dev_f32(x, "median_filter")
    _dev_f32(out, "median_filter")
    C = int(x.shape[0])
    if tuple(out.shape) != tuple(x.shape) or out.data_ptr() == x.data_ptr():
        raise RuntimeError("median_filter: out has the shape of x and is another buffer")
    if C > 16 or len(sizes) != C:
        raise ValueError(f"median_filter: one size per channel (at most 16), got {len(sizes)} for {C}")
    call("mvd_feed_median_filter_f32", _p(x), _p(out), C, *[int(v) for v in x.shape[1:]],
         (ctypes.c_int * C)(*[0 if v is None else int(v) for v in sizes]), _stream())


def sharpen(x, ws, strengths, stats):
    """In place: SharpeningTransform on every channel of x [C,D,H,W] whose strength is not None / 0 --
    clip(scipy.signal.convolve(x[c], strength L + delta, 'same'), min, max), L the 3x3x3 Laplacian (6, -1 on the faces);
    stats: channel_stats of x taken before; ws: float32 scratch of >= C*D*H*W values."""
    _dev_f32(x, "sharpen")
    C = int(x.shape[0])
    if not (ws.is_cuda and ws.dtype == torch.float32 and ws.is_contiguous() and ws.numel() >= x.numel()
            and ws.data_ptr() != x.data_ptr()):
        raise RuntimeError("sharpen: ws is a float32 device tensor of >= C*D*H*W values, not x itself")
    if not (stats.is_cuda and stats.dtype == torch.float64 and stats.numel() >= 4 * C):
        raise RuntimeError("sharpen: stats is a float64 device tensor of >= 4 C values")
    call("mvd_feed_sharpen_f32", _p(x), _p(ws), C, *[int(v) for v in x.shape[1:]],
         _chan_arg(strengths, C, ctypes.c_double), _p(stats), _stream())


def local_gauss(x, mode, params, stats=None):
    """In place: the Gaussian-field LocalTransforms on x [C,D,H,W].  params: per channel None or (scale[3], loc[3],
    amount); g = prod_d exp(-(i_d - loc_d)^2 / (2 scale_d^2)) / max g.  LOCAL_ADDITIVE x += amount g
    (BrightnessGradientAdditiveTransform, mean_centered=False); LOCAL_GAMMA x01 ^ (1 + (amount - 1) g) rescaled to the
    channel's own range, stats = channel_stats of x taken before (LocalGammaTransform)."""
    _dev_f32(x, "local_gauss")
    C = int(x.shape[0])
    if len(params) != C:
        raise ValueError(f"local_gauss: one entry per channel ({C}) expected, got {len(params)}")
    if mode == LOCAL_GAMMA and not (stats is not None and stats.is_cuda and stats.dtype == torch.float64
                                    and stats.numel() >= 4 * C):
        raise RuntimeError("local_gauss: the local gamma needs float64 stats of >= 4 C values")
    loc, scale, amount = [0.0] * (3 * C), [1.0] * (3 * C), [0.0] * C
    for c, prm in enumerate(params):
        if prm is not None:
            scale[3 * c:3 * c + 3] = [float(v) for v in prm[0]]
            loc[3 * c:3 * c + 3] = [float(v) for v in prm[1]]
            amount[c] = float(prm[2])
    call("mvd_feed_local_gauss_f32", _p(x), C, *[int(v) for v in x.shape[1:]],
         _chmask(C, [c for c, prm in enumerate(params) if prm is not None]), int(mode),
         (ctypes.c_double * (3 * C))(*loc), (ctypes.c_double * (3 * C))(*scale), (ctypes.c_float * C)(*amount),
         _p(stats) if stats is not None else None, _stream())


RECT_WS_DOUBLES = 64  # the first-level partial sums of blank_rectangle


def blank_rectangle(x, c, lb, size, ws):
    """In place: the box lb .. lb + size of channel c of x [C,D,H,W] becomes its own mean (fp64 sum, fixed order);
    ws: float64 device scratch of >= RECT_WS_DOUBLES values."""
    _dev_f32(x, "blank_rectangle")
    if not (ws.is_cuda and ws.dtype == torch.float64 and ws.numel() >= RECT_WS_DOUBLES):
        raise RuntimeError("blank_rectangle: ws is a float64 device tensor of >= 64 values")
    call("mvd_feed_blank_rectangle_f32", _p(x), *[int(v) for v in x.shape], int(c), (ctypes.c_int * 3)(*[int(v) for v in lb]),
         (ctypes.c_int * 3)(*[int(v) for v in size]), _p(ws), _stream())


def signed_permute(inp, out, perm, flip_mask=0):
    """out <- flip(transpose(inp, perm), flip_mask) over the spatial axes of every channel of inp [C,D,H,W] (bit k of
    flip_mask flips output axis k); permuted axes must have equal extents.  Distinct buffers."""
    _dev_f32(inp, "signed_permute")
    _dev_f32(out, "signed_permute")
    if tuple(out.shape) != tuple(inp.shape) or out.data_ptr() == inp.data_ptr():
        raise RuntimeError("signed_permute: out has the shape of inp and is another buffer")
    call("mvd_feed_signed_permute_f32", _p(inp), _p(out), *[int(v) for v in inp.shape],
         (ctypes.c_int * 3)(*[int(v) for v in perm]), int(flip_mask), _stream())


def compose_signed_permutation(rot90=None, transpose=None, flip_mask=0):
    """(perm, mask) with flip(transpose(x, perm), mask) == the spatial ops np.rot90(x, k, axes) [rot90 = (k, axes)], then
    np.transpose(x, transpose), then the flips of flip_mask, on arrays whose moved axes have equal extents.  Found by
    running those numpy calls on the three coordinate grids of a 2^3 cube: output axis k reads input axis perm[k],
    reversed when the coordinate there starts at 1."""
    grids = np.indices((2, 2, 2))
    res = []
    for g in grids:
        if rot90 is not None:
            g = np.rot90(g, int(rot90[0]), tuple(int(a) for a in rot90[1]))
        if transpose is not None:
            g = np.transpose(g, tuple(int(a) for a in transpose))
        for ax in range(3):
            if flip_mask & (1 << ax):
                g = np.flip(g, ax)
        res.append(g)
    perm, mask = [None] * 3, 0
    for k in range(3):
        step = [0, 0, 0]
        step[k] = 1
        for a in range(3):
            if res[a][tuple(step)] != res[a][0, 0, 0]:
                perm[k] = a
                if res[a][0, 0, 0] == 1:
                    mask |= 1 << k
    return tuple(perm), mask


def gaussian_noise(x, sigma, key, channels=None):
    """In place: x += sigma * N on the selected channels of x [C,D,H,W]; N of stored voxel k = c*D*H*W + v from the
    k-th numpy.random.Philox(key=key).random_raw() output (Box-Muller, see include/mvdseg_hip.h)."""
    _dev_f32(x, "gaussian_noise")
    key = int(key)
    if not 0 <= key < 2 ** 128:
        raise ValueError("gaussian_noise: key in [0, 2^128)")
    call("mvd_feed_gaussian_noise_f32", _p(x), int(x.shape[0]), x[0].numel(), _chmask(int(x.shape[0]), channels),
         key & (2 ** 64 - 1), key >> 64, float(sigma), _stream())


def lowres_gather(x, dpad, target_shape, flip_mask=0, pad=LOWRES_PAD):
    """dpad [td+2pad, th+2pad, tw+2pad] <- zoom(x', target/shape, order=0, mode='nearest', grid_mode=True) edge-padded
    by pad, with x' the single channel x [D,H,W] un-mirrored on flip_mask."""
    _dev_f32(x, "lowres_gather", 3)
    _dev_f32(dpad, "lowres_gather", 3)
    t = [int(v) for v in target_shape]
    if list(dpad.shape) != [v + 2 * pad for v in t]:
        raise RuntimeError("lowres_gather: dpad must be target_shape + 2 pad")
    call("mvd_feed_lowres_gather_f32", _p(x), _p(dpad), *[int(v) for v in x.shape], *t, int(pad), int(flip_mask),
         _stream())


def lowres_gather_2d(x, dpad, target_shape_2d, flip_mask=0, pad=LOWRES_PAD):
    """dpad [D, th+2pad, tw+2pad] <- per slice zoom(x'[z], (th, tw)/(H, W), order=0, mode='nearest', grid_mode=True)
    edge-padded by pad in-plane, with x' the single channel x [D,H,W] un-mirrored on flip_mask: the downsample of
    SimulateLowResolutionTransform(ignore_axes=(0,))."""
    _dev_f32(x, "lowres_gather_2d", 3)
    _dev_f32(dpad, "lowres_gather_2d", 3)
    t = [int(v) for v in target_shape_2d]
    if len(t) != 2 or list(dpad.shape) != [int(x.shape[0]), t[0] + 2 * pad, t[1] + 2 * pad]:
        raise RuntimeError("lowres_gather_2d: dpad must be [D, th + 2 pad, tw + 2 pad]")
    call("mvd_feed_lowres_gather2d_f32", _p(x), _p(dpad), *[int(v) for v in x.shape], *t, int(pad), int(flip_mask),
         _stream())


def mask_remove_label(data, seg, channels, replace=(-1, 0)):
    """MaskTransform (data[c] = 0 where seg[0] < 0, c in channels) then RemoveLabelTransform(replace) on seg, in place;
    data [C,D,H,W], seg [Cs,D,H,W] float32."""
    _dev_f32(data, "mask_remove_label")
    _dev_f32(seg, "mask_remove_label")
    if tuple(data.shape[1:]) != tuple(seg.shape[1:]):
        raise RuntimeError("mask_remove_label: data and seg differ in spatial shape")
    rf, rt = (replace if replace is not None else (0, 0))
    call("mvd_feed_mask_remove_label", _p(data), _p(seg), int(data.shape[0]), int(seg.shape[0]), data[0].numel(),
         _chmask(int(data.shape[0]), channels), int(replace is not None), int(rf), int(rt), _stream())


CASCADE_OPS = ('dilation', 'erosion', 'closing', 'opening')  # ApplyRandomBinaryOperatorTransform's any_of_these, in order
CASCADE_MAX_LABELS = 8


def ball_rows(radius):
    """skimage.morphology.ball(radius) for a float radius (restated: side n = int(2r + 1), grid linspace(-r, r, n) per
    axis, inside when x^2 + y^2 + z^2 <= r^2) as the table mvd_feed_cascade_morph takes: one row (dz, dy, lo, hi) per
    non-empty (z, y) line of the element, READ offsets of the erosion = index - n // 2, where scipy.ndimage centres an
    even-sided element (the dilation reads the negated offsets).  Every line of a ball is one interval."""
    radius = float(radius)
    n = int(2 * radius + 1)
    if not 1 <= n <= 16:
        raise ValueError("ball_rows: the side int(2 r + 1) must be within 1..16 (r < 8)")
    # summed as skimage does, (x^2 + y^2) + z^2: grid points lie exactly on the sphere for many radii (e.g. (2, 3, 6) / 7
    # of r at n = 15), where the order of the additions decides the rounding and with it the voxel
    g = np.linspace(-radius, radius, n)
    g = g * g
    inside = ((g[None, None, :] + g[None, :, None]) + g[:, None, None]) <= radius * radius
    c = n // 2
    rows = []
    for iz in range(n):
        for iy in range(n):
            xs = np.flatnonzero(inside[iz, iy])
            if len(xs) == 0:
                continue
            if int(xs[-1]) - int(xs[0]) + 1 != len(xs):
                raise ValueError("ball_rows: an element line is not one interval")
            rows.append((iz - c, iy - c, int(xs[0]) - c, int(xs[-1]) - c))
    return rows


def cascade_removal_threshold(num_voxels, fraction=0.15):
    """The integer T with (size < T) == (size < num_voxels * fraction) for every integer size, where the right side is
    the reference's fp64 test (cascade_transforms.py:71-72, num_voxels a np.uint64): T = ceil of that fp64 product."""
    return int(np.ceil(float(np.uint64(num_voxels) * float(fraction))))


def cascade_onehot(seg_plane, out, labels):
    """MoveSegAsOneHotToData: out[k] = (seg_plane == labels[k]) as 0/1 floats; seg_plane [D,H,W], out [K,D,H,W]."""
    _dev_f32(seg_plane, "cascade_onehot", 3)
    _dev_f32(out, "cascade_onehot", 4)
    K = len(labels)
    if not 1 <= K <= CASCADE_MAX_LABELS or out.shape[0] != K or tuple(out.shape[1:]) != tuple(seg_plane.shape):
        raise RuntimeError("cascade_onehot: out is [K,D,H,W] for 1..8 labels")
    call("mvd_feed_cascade_onehot", _p(seg_plane), _p(out), seg_plane.numel(), (ctypes.c_int * K)(*[int(l) for l in labels]),
         K, _stream())


def cascade_bitplanes(K, shape, device):
    """Zeroed bit-plane storage for K planes of `shape` (int64 words: [K, words per plane])."""
    words = int(query("mvd_feed_cascade_plane_words", *[int(v) for v in shape]))
    return torch.zeros((int(K), words), dtype=torch.int64, device=device)


def _check_bitplanes(bits, K, shape, name):
    words = int(query("mvd_feed_cascade_plane_words", *[int(v) for v in shape]))
    if not (bits.is_cuda and bits.dtype == torch.int64 and bits.is_contiguous() and bits.numel() >= K * words):
        raise RuntimeError(f"{name}: bit-planes are a contiguous int64 device tensor of >= K * plane words")


def cascade_pack(planes, bits):
    """K float planes [K,D,H,W] (non-zero = set) -> bit-planes along W (cascade_bitplanes)."""
    _dev_f32(planes, "cascade_pack", 4)
    _check_bitplanes(bits, planes.shape[0], planes.shape[1:], "cascade_pack")
    call("mvd_feed_cascade_pack", _p(planes), _p(bits), *[int(v) for v in planes.shape], _stream())


def cascade_unpack(bits, planes):
    """bit-planes -> K float planes [K,D,H,W] of 0/1."""
    _dev_f32(planes, "cascade_unpack", 4)
    _check_bitplanes(bits, planes.shape[0], planes.shape[1:], "cascade_unpack")
    call("mvd_feed_cascade_unpack", _p(bits), _p(planes), *[int(v) for v in planes.shape], _stream())


def cascade_morph(bits, tmp, K, shape, c, op, rows):
    """One channel step of ApplyRandomBinaryOperatorTransform on the K bit-planes of `shape`: operator `op` (index into
    CASCADE_OPS) with the element `rows` (ball_rows) on plane c, then every other plane loses the added voxels.
    tmp: 2 planes of scratch (cascade_bitplanes(2, ...))."""
    _check_bitplanes(bits, K, shape, "cascade_morph")
    _check_bitplanes(tmp, 2, shape, "cascade_morph")
    flat = [int(v) for r in rows for v in r]
    call("mvd_feed_cascade_morph", _p(bits), _p(tmp), int(K), int(c), int(op), *[int(v) for v in shape],
         (ctypes.c_int * len(flat))(*flat), len(rows), _stream())


def cascade_remove_workspace(shape, device):
    n = int(np.prod([int(v) for v in shape]))
    return torch.empty(int(query("mvd_feed_cascade_remove_workspace_bytes", n)), dtype=torch.uint8, device=device)


def cascade_remove(chan, u, threshold, ws, chosen, other=None):
    """RemoveRandomConnectedComponentFromOneHotEncodingTransform on the float plane chan [D,H,W], in place: clears valid
    component number floor(u n_valid) (26-connected, valid: voxel count < threshold, in the order of the smallest linear
    index); `other` [D,H,W] is set to 1 there when given.  chosen: int32[2] device tensor <- (label, n_valid)."""
    _dev_f32(chan, "cascade_remove", 3)
    if other is not None:
        _dev_f32(other, "cascade_remove", 3)
        if tuple(other.shape) != tuple(chan.shape):
            raise RuntimeError("cascade_remove: chan and other differ in shape")
    if not (chosen.is_cuda and chosen.dtype == torch.int32 and chosen.numel() >= 2 and ws.is_cuda):
        raise RuntimeError("cascade_remove: chosen is an int32[2] device tensor, ws a device buffer")
    call("mvd_feed_cascade_remove", _p(chan), _p(other) if other is not None else None, *[int(v) for v in chan.shape],
         int(threshold), float(u), _p(ws), ws.numel() * ws.element_size(), _p(chosen), _stream())


def lowres_target_shape(shape, zoom):
    """np.round(shape * zoom) (augment_linear_downsampling_scipy), at least 1 per axis (the reference cannot resize a
    length-1 axis to 0 either)."""
    return [max(1, int(v)) for v in np.round(np.asarray(shape, dtype=np.float64) * zoom).astype(int)]


def lowres_affine(shape, target):
    """The diagonal map p = s (o - (n-1)/2) + off of scipy's order-3 zoom t -> n on the pad-12 array:
    p = (o + 0.5) t/n - 0.5 + 12."""
    s = [t / n for n, t in zip(shape, target)]
    a = [s[0], 0., 0., 0., s[1], 0., 0., 0., s[2]]
    return a + [si * n / 2. - 0.5 + LOWRES_PAD for si, n in zip(s, shape)]


def lowres_affine_2d(shape_2d, target_2d):
    """lowres_affine over (H, W) only: 6 values for spatial_transform_data_2d."""
    s = [t / n for n, t in zip(shape_2d, target_2d)]
    return [s[0], 0., 0., s[1]] + [si * n / 2. - 0.5 + LOWRES_PAD for si, n in zip(s, shape_2d)]


INTENSITY_KEYS = ('noise', 'blur', 'brightness', 'contrast', 'lowres', 'gamma_inverted', 'gamma')
# p_per_sample of the DA5 transforms as nnUNetTrainerDA5 sets them, and their common p_per_channel
DA5_PROBABILITIES = {'rot90': 0.5, 'transpose': 0.5, 'median': 0.2, 'blur': 0.2, 'noise': 0.1, 'brightness': 0.1,
                     'contrast': 0.2, 'lowres': 0.15, 'gamma': 0.1, 'blank': 0.4, 'gradient': 0.3, 'local_gamma': 0.3,
                     'sharpen': 0.2, 'per_channel': 0.5}


class DeviceDataLoader3D:
    """nnUNetDataLoader3D with the per-batch work on the GPU.  `data` is an nnUNetDataset-like object: `.keys()` and
    `.load_case(key) -> (data [C,D,H,W] float32, seg [1,D,H,W] integer, properties)` with
    properties['class_locations'] = {label: array of (c, z, y, x) rows} (nnunet_dataset.py:87-106).  Cases are
    uploaded once and stay resident."""

    def __init__(self, data, batch_size, patch_size, final_patch_size, label_manager, oversample_foreground_percent=0.0,
                 sampling_probabilities=None, pad_sides=None, probabilistic_oversampling=False, mirror_axes=None,
                 deep_supervision_scales=None, device="cuda:0", rotation_for_DA=None, scale_range=(0.7, 1.4),
                 p_rot_per_sample=0.2, p_scale_per_sample=0.2, p_rot_per_axis=1.0, do_dummy_2d_data_aug=False,
                 intensity_augmentation=False, mask_channels=None, p_noise=0.1, p_blur=0.2, p_blur_per_channel=0.5,
                 p_brightness=0.15, p_contrast=0.15, p_lowres=0.25, p_lowres_per_channel=0.5, p_gamma_inverted=0.1,
                 p_gamma=0.3, cascade_labels=None, cascade_augmentation=False, p_cascade_binary=0.4,
                 cascade_strel_size=(1, 8), p_cascade_remove=0.2, cascade_fill_with_other_class_p=0.0,
                 cascade_max_component_fraction=0.15, da5=False, da5_probabilities=None):
        self._data = data
        # the DA5 recipe (nnUNetTrainerDA5.get_training_transforms) in place of the default intensity stage
        self.da5 = bool(da5)
        self.da5_p = dict(DA5_PROBABILITIES)
        if da5_probabilities is not None:
            unknown = set(da5_probabilities) - set(DA5_PROBABILITIES)
            if unknown:
                raise ValueError(f"DeviceDataLoader3D: unknown DA5 probabilities {sorted(unknown)}")
            self.da5_p.update({k: float(v) for k, v in da5_probabilities.items()})
        if self.da5:
            if len(patch_size) != 3 or len(final_patch_size) != 3 or int(final_patch_size[0]) == 1:
                raise NotImplementedError("DeviceDataLoader3D: DA5 is built for 3-D plans only (a 2-D plan is refused)")
            if do_dummy_2d_data_aug:
                raise NotImplementedError("DeviceDataLoader3D: DA5 with do_dummy_2d_data_aug=True (the in-plane form of "
                                          "the recipe) is not built")
            if cascade_labels is not None or cascade_augmentation:
                raise NotImplementedError("DeviceDataLoader3D: DA5 in cascade mode is not built")
        self._dstate = None  # DA5 scratch (ping-pong sample buffers, rectangle partial sums), reused across batches
        # cascade mode (nnUNetTrainer.py:740-755, :783-784): load_case returns a seg of two channels, channel 1 the previous
        # stage's segmentation; cascade_labels = label_manager.foreground_labels become that many one-hot input channels
        # behind the modalities.  cascade_augmentation adds the binary operators and the component removal (training);
        # without it only the one-hot move runs (get_validation_transforms)
        self.cascade_labels = None if cascade_labels is None else [int(l) for l in cascade_labels]
        if self.cascade_labels is not None and not 1 <= len(self.cascade_labels) <= CASCADE_MAX_LABELS:
            raise NotImplementedError(f"DeviceDataLoader3D: the cascade stage takes 1..{CASCADE_MAX_LABELS} foreground "
                                      f"labels, got {len(self.cascade_labels)}")
        self.cascade_augmentation = bool(cascade_augmentation) and self.cascade_labels is not None
        self.p_cascade_binary, self.p_cascade_remove = float(p_cascade_binary), float(p_cascade_remove)
        self.cascade_strel_size = tuple(float(v) for v in cascade_strel_size)
        if not 1 <= self.cascade_strel_size[0] <= self.cascade_strel_size[1] <= 8:
            raise ValueError("DeviceDataLoader3D: cascade_strel_size within [1, 8] (the kernel's elements are 16^3 at most)")
        self.cascade_fill_with_other_class_p = float(cascade_fill_with_other_class_p)
        self.cascade_max_component_fraction = float(cascade_max_component_fraction)
        # ApplyRandomBinaryOperatorTransform shuffles its stored channel list in place: the order persists between batches
        self._cascade_order = list(range(len(self.cascade_labels or ())))
        self._cstate = None
        self.batch_size = int(batch_size)
        self.indices = list(data.keys())
        self.oversample_foreground_percent = oversample_foreground_percent
        self.final_patch_size = tuple(int(i) for i in final_patch_size)
        self.patch_size = tuple(int(i) for i in patch_size)
        # SpatialTransform (nnUNetTrainer.py:703-714) as configured there: rotation_for_DA = {'x': (lo, hi), 'y': ..,
        # 'z': ..} in radians; None leaves the loader without it (then the patch must already be the final one)
        self.rotation_for_DA = None if rotation_for_DA is None else {k: tuple(float(v) for v in rotation_for_DA[k])
                                                                     for k in ('x', 'y', 'z')}
        self.scale_range = tuple(float(v) for v in scale_range)
        self.p_rot_per_sample, self.p_scale_per_sample = float(p_rot_per_sample), float(p_scale_per_sample)
        self.p_rot_per_axis = float(p_rot_per_axis)
        if self.rotation_for_DA is None and self.patch_size != self.final_patch_size:
            # the larger initial patch only exists to feed the rotation / scaling transform
            raise NotImplementedError("DeviceDataLoader3D: patch_size must equal final_patch_size (no SpatialTransform)")
        # anisotropic plans (nnUNetTrainer.py:695-717): the SpatialTransform runs in-plane on [C*D, H, W] and the
        # low-resolution simulation ignores axis 0
        self.do_dummy_2d_data_aug = bool(do_dummy_2d_data_aug)
        if self.do_dummy_2d_data_aug and self.patch_size[0] != self.final_patch_size[0]:
            raise NotImplementedError("DeviceDataLoader3D: do_dummy_2d_data_aug needs patch_size[0] == "
                                      "final_patch_size[0]: the in-plane 2-D SpatialTransform of Convert3DTo2DTransform "
                                      "leaves axis 0 alone, so it cannot crop or resample it")
        if self.rotation_for_DA is not None and any(p < f for p, f in zip(self.patch_size, self.final_patch_size)):
            raise ValueError("DeviceDataLoader3D: patch_size must not be smaller than final_patch_size")
        # the intensity stage (nnUNetTrainer.py:719-736) with its per-sample / per-channel probabilities, and
        # MaskTransform: mask_channels is the plans' use_mask_for_norm (one bool per input channel)
        self.intensity_augmentation = bool(intensity_augmentation) or self.da5  # DA5 implies the stage
        self.p_noise, self.p_blur, self.p_blur_per_channel = float(p_noise), float(p_blur), float(p_blur_per_channel)
        self.p_brightness, self.p_contrast = float(p_brightness), float(p_contrast)
        self.p_lowres, self.p_lowres_per_channel = float(p_lowres), float(p_lowres_per_channel)
        self.p_gamma_inverted, self.p_gamma = float(p_gamma_inverted), float(p_gamma)
        self.mask_channels = None if mask_channels is None else [i for i, m in enumerate(mask_channels) if m]
        if self.mask_channels == []:
            self.mask_channels = None  # MaskTransform is only added when some channel uses it
        self._istate = None  # intensity scratch (statistics, blur / low-res buffers), reused across batches
        self.list_of_keys = list(data.keys())
        self.need_to_pad = (np.array(patch_size) - np.array(final_patch_size)).astype(int)  # base_data_loader.py:33
        if pad_sides is not None:
            self.need_to_pad += np.array(pad_sides)
        self.pad_sides = pad_sides
        self.sampling_probabilities = sampling_probabilities
        self.annotated_classes_key = tuple(label_manager.all_labels)
        self.has_ignore = label_manager.has_ignore_label
        self.get_do_oversample = self._oversample_last_XX_percent if not probabilistic_oversampling \
            else self._probabilistic_oversampling
        self.mirror_axes = tuple(mirror_axes) if mirror_axes else ()
        self.deep_supervision_scales = deep_supervision_scales
        self.device = torch.device(device)  # planning (plan_batch) is host logic; generate_train_batch needs a GPU
        self._resident = {}
        self._scratch = None  # initial-patch buffers of the modified samples, reused across samples and batches
        d0, s0, _ = self._case(self.indices[0])  # determine_shapes (:55-62)
        # the batch leaves SpatialTransform at the final patch size (== patch_size without it)
        self.num_modalities = int(d0.shape[0])
        self.data_shape = (self.batch_size, d0.shape[0], *self.final_patch_size)
        self.seg_shape = (self.batch_size, s0.shape[0], *self.final_patch_size)
        if self.cascade_labels is not None:
            if s0.shape[0] != 2:
                raise ValueError("DeviceDataLoader3D: in cascade mode load_case returns a seg of two channels (channel 1: "
                                 "the previous stage's segmentation)")
            if self.mask_channels is not None and max(self.mask_channels) >= self.num_modalities:
                raise ValueError("DeviceDataLoader3D: mask_channels name modality channels")
            self.data_shape = (self.batch_size, self.num_modalities + len(self.cascade_labels), *self.final_patch_size)
            self.seg_shape = (self.batch_size, 1, *self.final_patch_size)

    # ------------------------------------------------------------------ residency
    def _case(self, key):
        hit = self._resident.get(key)
        if hit is None:
            data, seg, properties = self._data.load_case(key)
            data = torch.as_tensor(np.ascontiguousarray(data), dtype=torch.float32).to(self.device)
            seg = np.ascontiguousarray(seg)
            if seg.min() < -32768 or seg.max() > 32767:
                raise ValueError("segmentation labels must fit int16 (the reference batch buffer is int16)")
            seg = torch.as_tensor(seg.astype(np.int16)).to(self.device)
            hit = (data, seg, properties)
            self._resident[key] = hit
        return hit

    # ------------------------------------------------------------------ host logic (numpy RNG, reference call order)
    def get_indices(self):
        # batchgenerators DataLoader.get_indices, infinite=True
        return np.random.choice(self.indices, self.batch_size, replace=True, p=self.sampling_probabilities)

    def _oversample_last_XX_percent(self, sample_idx):
        return not sample_idx < round(self.batch_size * (1 - self.oversample_foreground_percent))

    def _probabilistic_oversampling(self, sample_idx):
        return np.random.uniform() < self.oversample_foreground_percent

    def _corner_range(self, data_shape):
        """(lowest, highest) admissible lower patch corner per axis.  A case smaller than the patch is padded on both
        sides (the odd voxel goes to the upper side); `need_to_pad` widens the range by the margin the reference keeps
        for its spatial transform."""
        shape = np.asarray(data_shape, dtype=np.int64)
        patch = np.asarray(self.patch_size, dtype=np.int64)
        margin = np.maximum(np.asarray(self.need_to_pad, dtype=np.int64), patch - shape)
        lowest = (-margin) // 2
        highest = shape + margin // 2 + margin % 2 - patch
        return lowest.tolist(), highest.tolist()

    def _centre_class(self, force_fg, class_locations, overwrite_class, verbose):
        """Which class (or region key) the patch must be centred on; None -> uniform corner.  One np.random.choice
        when a foreground class has to be drawn, none otherwise."""
        everything = self.annotated_classes_key
        if not force_fg:
            if not self.has_ignore:
                return None
            # ignore label present: stay inside the annotated area whenever the case has one
            if len(class_locations[everything]) == 0:
                print('Warning! No annotated pixels in image!')
                return None
            return everything
        if class_locations is None:
            raise AssertionError('if force_fg is set class_locations cannot be None')
        if overwrite_class is not None and overwrite_class not in class_locations.keys():
            raise AssertionError('desired class ("overwrite_class") does not have class_locations (missing key)')
        present = [k for k in class_locations.keys() if len(class_locations[k]) > 0]
        if len(present) > 1:
            # the all-annotated-classes key only serves cases that have nothing more specific
            for j, k in enumerate(present):
                if isinstance(k, tuple) and k == everything:
                    del present[j]
                    break
        if not present:
            if verbose:
                print('case does not contain any foreground classes')
            return None
        if overwrite_class is not None and overwrite_class in present:
            return overwrite_class
        return present[np.random.choice(len(present))]

    def get_bbox(self, data_shape, force_fg, class_locations, overwrite_class=None, verbose=False):
        """Lower / upper corner of the patch to cut from a case of spatial shape `data_shape` -- the sampler of
        nnUNetDataLoaderBase.get_bbox (base_data_loader.py:64-139) with the same arguments, result and numpy-RNG draw
        order (tests/golden/get_bbox.json holds boxes AND the RNG state after each call, generated by the reference
        method): centred on a random voxel of a random foreground class when `force_fg`, uniform otherwise."""
        lowest, highest = self._corner_range(data_shape)
        axes = range(len(data_shape))
        cls = self._centre_class(force_fg, class_locations, overwrite_class, verbose)
        voxels = class_locations[cls] if cls is not None else None
        if voxels is not None and len(voxels) > 0:
            centre = voxels[np.random.choice(len(voxels))]   # row = (channel, z, y, x)
            corner = [max(lowest[i], int(centre[i + 1]) - self.patch_size[i] // 2) for i in axes]
        else:
            corner = [int(np.random.randint(lowest[i], highest[i] + 1)) for i in axes]
        return corner, [corner[i] + self.patch_size[i] for i in axes]

    def draw_mirror(self):
        """MirrorTransform's per-sample draw (batchgenerators, absent from the reference tree -- restated from its
        published source: one uniform per listed axis, flip when < 0.5).  Returns the 3-bit axis mask."""
        mask = 0
        for ax in (0, 1, 2):
            if ax in self.mirror_axes and np.random.uniform() < 0.5:
                mask |= 1 << ax
        return mask

    def draw_spatial(self):
        """SpatialTransform's per-sample draws (batchgenerators augment_spatial with the arguments of
        nnUNetTrainer.py:703-714; absent from the reference tree -- restated from its published source).  No elastic
        draw (do_elastic_deform=False short-circuits); a rotation draw, then per axis x, y, z an axis draw and an angle;
        a scaling draw, then the down/up choice and the factor (independent_scale_for_each_axis=False short-circuits).
        In the dummy 2-D mode (augment_spatial's dim == 2) only the x axis draw and angle exist: the y / z draws sit
        inside `if dim == 3`, so a rotation costs 2 draws, not 6, and a_y = a_z = 0.
        Returns None for an unmodified sample, else (a_x, a_y, a_z, sc)."""
        rot, sc, modified = [0., 0., 0.], 1., False
        if np.random.uniform() < self.p_rot_per_sample:
            for i, ax in enumerate(('x',) if self.do_dummy_2d_data_aug else ('x', 'y', 'z')):
                if np.random.uniform() <= self.p_rot_per_axis:
                    rot[i] = np.random.uniform(*self.rotation_for_DA[ax])
            modified = True
        if np.random.uniform() < self.p_scale_per_sample:
            lo, hi = self.scale_range

            def factor():
                if np.random.random() < 0.5 and lo < 1:
                    return np.random.uniform(lo, 1)
                return np.random.uniform(max(lo, 1), hi)

            if self.da5:
                # independent_scale_for_each_axis=True: one uniform (< p_independent_scale_per_axis = 1), then the
                # down/up draw of every axis in turn
                np.random.uniform()
                sc = tuple(float(factor()) for _ in range(3))
            else:
                sc = factor()
            modified = True
        if not modified:
            return None
        return (float(rot[0]), float(rot[1]), float(rot[2]), sc if isinstance(sc, tuple) else float(sc))

    def draw_intensity(self, nsamples, nchannels):
        """The intensity transforms' draws for a batch (batchgenerators, absent from the reference tree -- restated from
        its published source with nnU-Net's arguments, nnUNetTrainer.py:719-736).  Transform by transform, each over
        all samples (as Compose runs them); every transform first draws `np.random.uniform() < p_per_sample`:
          noise       sigma ~ U(0, 0.1); per channel a uniform (< p_per_channel = 1); then ONE key for the device field
                      (np.random.randint(0, 2^63), in place of the reference's np.random.normal field)
          blur        per channel a uniform (<= 0.5), then sigma ~ U(0.5, 1) for a selected channel
          brightness  one multiplier that is drawn and discarded, then one ~ U(0.75, 1.25) per channel
          contrast    per channel a uniform (< 1), a uniform (< 0.5: U(0.75, 1), else U(1, 1.25))
          low-res     per channel a uniform (< 0.5), then the zoom ~ U(0.5, 1) for a selected channel
          gamma inv.  per channel a uniform (< 0.5: U(0.7, 1), else U(1, 1.5))
          gamma       the same
        The reference takes the noise level and get_range_val's values (blur sigma) from Python's `random` module;
        here every draw is np.random's, so a seeded run is reproducible with np.random.seed alone.  RNG-stream parity
        with the reference is not a goal.  Returns one dict per sample with the keys INTENSITY_KEYS: None
        when the transform skips the sample, else noise (sigma, key), blur / low-res a per-channel list of sigma /
        zoom or None, the others a per-channel list of the factor."""
        out = [dict.fromkeys(INTENSITY_KEYS) for _ in range(nsamples)]
        u = np.random.uniform

        def two_sided(lo, hi):  # contrast / gamma: (lo, 1) or (1, hi) with probability 1/2 each
            return u(lo, 1) if np.random.random() < 0.5 and lo < 1 else u(max(lo, 1), hi)

        for it in out:
            if u() < self.p_noise:
                sigma = u(0, 0.1)
                for _ in range(nchannels):
                    u()  # p_per_channel = 1
                it['noise'] = (float(sigma), int(np.random.randint(0, 2 ** 63, dtype=np.int64)))
        for it in out:
            if u() < self.p_blur:
                it['blur'] = [float(u(0.5, 1.)) if u() <= self.p_blur_per_channel else None for _ in range(nchannels)]
        for it in out:
            if u() < self.p_brightness:
                u(0.75, 1.25)
                it['brightness'] = [float(u(0.75, 1.25)) for _ in range(nchannels)]
        def per_channel_factor(lo, hi):  # contrast: a selection uniform (p_per_channel = 1) before each factor
            u()
            return float(two_sided(lo, hi))

        for it in out:
            if u() < self.p_contrast:
                it['contrast'] = [per_channel_factor(0.75, 1.25) for _ in range(nchannels)]
        for it in out:
            if u() < self.p_lowres:
                it['lowres'] = [float(u(0.5, 1)) if u() < self.p_lowres_per_channel else None for _ in range(nchannels)]
        for key, p in (('gamma_inverted', self.p_gamma_inverted), ('gamma', self.p_gamma)):
            for it in out:
                if u() < p:
                    it[key] = [float(two_sided(0.7, 1.5)) for _ in range(nchannels)]
        return out

    def da5_valid_axes(self):
        """Rot90Transform's / TransposeAxesTransform's axes as nnUNetTrainerDA5 chooses them: the axes of the final patch
        that share its most frequent extent; () when every extent occurs once (then neither transform is added)."""
        p = self.final_patch_size
        counts = [sum(q == v for q in p) for v in p]
        if max(counts) < 2:
            return ()
        return tuple(i for i, n in enumerate(counts) if n == max(counts))

    def draw_da5(self, nsamples, nchannels):
        """The draws of the DA5 recipe behind its SpatialTransform (nnUNetTrainerDA5.get_training_transforms;
        batchgenerators is absent from the reference tree -- its glue is restated from the published source without the
        package at hand, so parity with batchgenerators itself is unpinned).  Transform by transform, each
        over all samples (as Compose runs them), every draw from np.random.  p = self.da5_p[...], pc = p['per_channel']:
          rot90        (only with da5_valid_axes) per sample a uniform (< p), np.random.choice((0, 1, 2, 3)), then
                       np.random.choice(valid_axes, 2, replace=False), sorted
          transpose    (same condition) per sample a uniform (< p), np.random.shuffle of a copy of valid_axes; the
                       shuffled axes fill the valid positions of the transpose
          median|blur  ONE np.random.choice(2) per batch (OneOfTransform); then the chosen transform alone draws:
                       median per sample a uniform (< p), per channel a uniform (< pc) and np.random.randint(2, 8);
                       blur per sample a uniform (< p), per channel a uniform (<= pc) and sigma ~ U(0.3, 1.5)
          noise        as draw_intensity: a uniform (< p), sigma ~ U(0, 0.1), a uniform per channel, one key
          brightness   a uniform (< p), per channel a uniform (<= pc) and np.random.normal(0, 0.5)
          contrast     ONE np.random.choice(2) per batch (0: preserve_range=True, 1: False); per sample a uniform (< p),
                       per channel a uniform (< pc) and the two-sided factor over (0.5, 2)
          low-res      a uniform (< p), per channel a uniform (< pc) and the zoom ~ U(0.25, 1)
          gamma, twice a uniform (< p), per channel the two-sided factor over (0.7, 1.5); both run inverted
          mirror       draw_mirror
          blank        a uniform (< p), per channel a uniform (< pc), n = np.random.randint(1, 5) rectangles, each: per
                       axis size_d = randint(max(1, p_d // 10), p_d // 3 + 1), then per axis lb_d = randint(0,
                       max(p_d - size_d, 1))
          gradient     a uniform (< p), per channel a uniform (< pc), per axis scale_d = exp(U(log(max(1, p_d // 6)),
                       log(p_d))), then per axis loc_d = U(-0.5, 1.5) p_d, then a uniform (< 0.5: U(-5, -1), else U(1, 5))
          local gamma  the same with the gamma: a uniform (< 0.5: U(0.01, 0.8), else U(1.5, 4))
          sharpen      a uniform (< p), per channel a uniform (< pc) and the strength ~ U(0.1, 1)
        With every probability at 0 that is 2 np.random.choice calls, and per sample 11 uniforms (13 with valid axes)
        plus draw_mirror's one per mirror axis.  Returns a dict of per-sample lists (None: the transform skips the
        sample; per-channel lists hold None for a channel that is not selected), 'oneof_blur' / 'oneof_contrast' the two
        batch choices, 'signed' the (perm, mask) of rot90 and transpose composed (None: identity)."""
        P = self.da5_p
        pc = P['per_channel']
        u = np.random.uniform
        ps = self.final_patch_size
        rng = range(nsamples)
        d = {'da5': True}

        def two_sided(lo, hi):
            return u(lo, 1) if np.random.random() < 0.5 and lo < 1 else u(max(lo, 1), hi)

        valid = self.da5_valid_axes()
        d['rot90'], d['transpose'] = [None] * nsamples, [None] * nsamples
        if valid:
            for j in rng:
                if u() < P['rot90']:
                    k = int(np.random.choice((0, 1, 2, 3)))
                    axes = sorted(int(a) for a in np.random.choice(valid, size=2, replace=False))
                    d['rot90'][j] = (k, tuple(axes))
            for j in rng:
                if u() < P['transpose']:
                    shuffled = list(valid)
                    np.random.shuffle(shuffled)
                    t = [0, 1, 2]
                    for pos, a in zip(valid, shuffled):
                        t[pos] = int(a)
                    d['transpose'][j] = tuple(t)
        d['signed'] = []
        for j in rng:
            perm, mask = compose_signed_permutation(d['rot90'][j], d['transpose'][j])
            d['signed'].append(None if perm == (0, 1, 2) and mask == 0 else (perm, mask))

        d['oneof_blur'] = int(np.random.choice(2))
        d['median'], d['blur'] = [None] * nsamples, [None] * nsamples
        for j in rng:
            if d['oneof_blur'] == 0:
                if u() < P['median']:
                    d['median'][j] = [int(np.random.randint(2, 8)) if u() < pc else None for _ in range(nchannels)]
            elif u() < P['blur']:
                d['blur'][j] = [float(u(0.3, 1.5)) if u() <= pc else None for _ in range(nchannels)]
        d['noise'] = [None] * nsamples
        for j in rng:
            if u() < P['noise']:
                sigma = u(0, 0.1)
                for _ in range(nchannels):
                    u()  # p_per_channel = 1
                d['noise'][j] = (float(sigma), int(np.random.randint(0, 2 ** 63, dtype=np.int64)))
        d['brightness'] = [None] * nsamples
        for j in rng:
            if u() < P['brightness']:
                d['brightness'][j] = [float(np.random.normal(0, 0.5)) if u() <= pc else None for _ in range(nchannels)]
        d['oneof_contrast'] = int(np.random.choice(2))
        d['contrast'] = [None] * nsamples
        for j in rng:
            if u() < P['contrast']:
                d['contrast'][j] = [float(two_sided(0.5, 2)) if u() < pc else None for _ in range(nchannels)]
        d['lowres'] = [None] * nsamples
        for j in rng:
            if u() < P['lowres']:
                d['lowres'][j] = [float(u(0.25, 1)) if u() < pc else None for _ in range(nchannels)]
        for key in ('gamma1', 'gamma2'):
            d[key] = [None] * nsamples
            for j in rng:
                if u() < P['gamma']:
                    d[key][j] = [float(two_sided(0.7, 1.5)) for _ in range(nchannels)]
        d['mirror'] = [self.draw_mirror() for _ in rng]
        d['blank'] = [None] * nsamples
        for j in rng:
            if u() < P['blank']:
                chans = []
                for _ in range(nchannels):
                    rects = None
                    if u() < pc:
                        rects = []
                        for _r in range(int(np.random.randint(1, 5))):
                            size = [int(np.random.randint(max(1, p // 10), p // 3 + 1)) for p in ps]
                            lb = [int(np.random.randint(0, max(p - s, 1))) for p, s in zip(ps, size)]
                            rects.append((lb, size))
                    chans.append(rects)
                d['blank'][j] = chans

        def local(amount):
            scale = [float(np.exp(u(np.log(max(1, p // 6)), np.log(p)))) for p in ps]
            loc = [float(u(-0.5, 1.5) * p) for p in ps]
            return scale, loc, float(amount())

        for key, amount in (('gradient', lambda: u(-5, -1) if u() < 0.5 else u(1, 5)),
                            ('local_gamma', lambda: u(0.01, 0.8) if u() < 0.5 else u(1.5, 4))):
            d[key] = [None] * nsamples
            for j in rng:
                if u() < P[key]:
                    d[key][j] = [local(amount) if u() < pc else None for _ in range(nchannels)]
        d['sharpen'] = [None] * nsamples
        for j in rng:
            if u() < P['sharpen']:
                d['sharpen'][j] = [float(u(0.1, 1)) if u() < pc else None for _ in range(nchannels)]
        return d

    def draw_cascade(self, nsamples):
        """The two cascade transforms' draws for a batch (nnUNetTrainer.py:741-755), each over all samples as Compose runs
        them.
          binary operators  ApplyRandomBinaryOperatorTransform's own draws, restated exactly (none depends on the data):
                            per sample a uniform (< 0.4), np.random.shuffle of the stored channel list in place, then per
                            channel a uniform (< p_per_label = 1), np.random.choice among the four operators and
                            uniform(1, 8) for the ball radius.  -> per sample None or [(channel, op, radius), ...]
          removal           the reference's draws depend on the data (np.any, the number of valid components, a choice
                            over them); here a fixed set per sample: a uniform (< 0.2), then per channel a uniform
                            (< p_per_label = 1), u for the pick, a uniform (< fill_with_other_class_p) and -- with more
                            than one channel -- the other class; the device does the data-dependent part.  The
                            distribution is the reference's, the RNG stream is not.
                            -> per sample None or [(channel, u, other channel or None), ...]
        Channels are indices into the K one-hot channels."""
        K = len(self.cascade_labels)
        u = np.random.uniform
        binary, remove = [], []
        for _ in range(nsamples):
            steps = None
            if u() < self.p_cascade_binary:
                np.random.shuffle(self._cascade_order)
                steps = []
                for c in self._cascade_order:
                    if u() < 1:
                        op = int(np.random.choice(len(CASCADE_OPS)))
                        steps.append((int(c), op, float(u(*self.cascade_strel_size))))
            binary.append(steps)
        for _ in range(nsamples):
            steps = None
            if u() < self.p_cascade_remove:
                steps = []
                for c in range(K):
                    if u() < 1:
                        pick = float(u())
                        fill = u() < self.cascade_fill_with_other_class_p
                        other = int(np.random.choice([i for i in range(K) if i != c])) if K > 1 else None
                        steps.append((c, pick, other if fill else None))
            remove.append(steps)
        return {'cascade': True, 'binary': binary, 'remove': remove}

    # ------------------------------------------------------------------ the batch
    def plan_batch(self):
        """The host decisions of one batch, in the reference's RNG order: keys, then per sample (oversample?, bbox),
        then per sample the SpatialTransform draws (only with rotation_for_DA), then the intensity draws (only with
        intensity_augmentation, draw_intensity), then per sample the mirror draw.  With da5 the intensity draws are
        draw_da5's dict, which holds the mirror draws at their place in the recipe (flips repeats them).  In cascade mode with
        cascade_augmentation the plan gains a last element, draw_cascade's dict, drawn after the mirrors."""
        plan = self._plan_base()
        if self.cascade_augmentation:
            plan = plan + (self.draw_cascade(len(plan[0])),)
        return plan

    def _plan_base(self):
        keys = self.get_indices()
        boxes = []
        for j, k in enumerate(keys):
            force_fg = self.get_do_oversample(j)
            data, _, properties = self._case(k)
            lbs, _ = self.get_bbox(tuple(data.shape[1:]), force_fg, properties['class_locations'])
            boxes.append([int(v) for v in lbs])
        if self.da5:
            # the mirror is drawn inside draw_da5, at its place in the recipe; the crop and the warp run un-mirrored
            spatial = [self.draw_spatial() if self.rotation_for_DA is not None else None for _ in keys]
            da5 = self.draw_da5(len(keys), self.num_modalities)
            return list(keys), boxes, spatial, da5, list(da5['mirror'])
        if self.intensity_augmentation:
            spatial = [self.draw_spatial() if self.rotation_for_DA is not None else None for _ in keys]
            intensity = self.draw_intensity(len(keys), self.num_modalities)
            flips = [self.draw_mirror() for _ in keys]
            return list(keys), boxes, spatial, intensity, flips
        if self.rotation_for_DA is None:
            flips = [self.draw_mirror() for _ in keys]
            return list(keys), boxes, flips
        spatial = [self.draw_spatial() for _ in keys]
        flips = [self.draw_mirror() for _ in keys]
        return list(keys), boxes, spatial, flips

    def _scratch_for(self, data, seg):
        shape = (data.shape[0], seg.shape[0])
        if self._scratch is None or self._scratch[0] != shape:
            self._scratch = (shape, torch.empty((data.shape[0], *self.patch_size), dtype=torch.float32, device=self.device),
                             torch.empty((seg.shape[0], *self.patch_size), dtype=torch.float32, device=self.device))
        return self._scratch[1], self._scratch[2]

    def _intensity_state(self, C, V):
        st = self._istate
        if st is None or st['C'] != C:
            n = [v + 2 * LOWRES_PAD for v in self.final_patch_size]
            st = {'C': C, 'stats': torch.empty((2, C, 4), dtype=torch.float64, device=self.device),
                  'stats1': torch.empty((2, 4), dtype=torch.float64, device=self.device),
                  'ws': stats_workspace(C, self.device),
                  'blur': torch.empty(2 * C * V, dtype=torch.float32, device=self.device),
                  'dpad': torch.empty(int(np.prod(n)), dtype=torch.float32, device=self.device)}
            self._istate = st
        return st

    def apply_intensity(self, x, it, flip_mask):
        """The intensity stage on one sample x [C,D,H,W] (already mirrored on flip_mask, as the feed's crop / warp
        kernels store it), in the reference order noise, blur, brightness, contrast, low-res, gamma (inverted), gamma.
        Every transform but the noise (indexed by stored voxel) and the low-res downsample (un-mirrored in its gather,
        re-mirrored by the warp) commutes with the mirror."""
        C = int(x.shape[0])
        shape = tuple(int(v) for v in x.shape[1:])
        st = self._intensity_state(C, x[0].numel())
        sa, sb = st['stats'][0], st['stats'][1]
        if it['noise'] is not None:
            gaussian_noise(x, it['noise'][0], it['noise'][1])
        if it['blur'] is not None and any(v is not None for v in it['blur']):
            gaussian_blur(x, it['blur'], st['blur'])
        if it['brightness'] is not None:
            intensity_apply(x, OP_BRIGHTNESS, it['brightness'])
        if it['contrast'] is not None:
            channel_stats(x, sa, st['ws'])
            intensity_apply(x, OP_CONTRAST, it['contrast'], sa)
        if it['lowres'] is not None:
            for c, z in enumerate(it['lowres']):
                if z is None:
                    continue
                t = lowres_target_shape(shape, z)
                if self.do_dummy_2d_data_aug:  # ignore_axes=(0,): target_shape[0] = shape[0], everything in-plane
                    dpad = st['dpad'][:shape[0] * int(np.prod([v + 2 * LOWRES_PAD for v in t[1:]]))].view(
                        shape[0], *[v + 2 * LOWRES_PAD for v in t[1:]])
                    lowres_gather_2d(x[c], dpad, t[1:], flip_mask)
                    d4 = dpad.unsqueeze(0)
                    channel_stats(d4, st['stats1'][0], st['ws'])
                    bspline_prefilter(d4, 6)
                    spatial_transform_data_2d(d4, x[c:c + 1], lowres_affine_2d(shape[1:], t[1:]), flip_mask, 0.0)
                    intensity_apply(x[c:c + 1], OP_CLIP, None, st['stats1'][0])
                    continue
                dpad = st['dpad'][:int(np.prod([v + 2 * LOWRES_PAD for v in t]))].view(
                    *[v + 2 * LOWRES_PAD for v in t])
                lowres_gather(x[c], dpad, t, flip_mask)
                d4 = dpad.unsqueeze(0)
                channel_stats(d4, st['stats1'][0], st['ws'])
                bspline_prefilter(d4, 7)
                spatial_transform_data(d4, x[c:c + 1], lowres_affine(shape, t), flip_mask, 0.0)
                intensity_apply(x[c:c + 1], OP_CLIP, None, st['stats1'][0])
        for key, op in (('gamma_inverted', OP_GAMMA_INVERTED), ('gamma', OP_GAMMA)):
            if it[key] is not None:
                channel_stats(x, sa, st['ws'])
                channel_stats(x, sb, st['ws'], pre_op=op, gammas=it[key], pre_stats=sa)
                intensity_apply(x, op, it[key], sa, sb)

    def _da5_state(self, C, Cs):
        st = self._dstate
        if st is None or st['shape'] != (C, Cs):
            f = self.final_patch_size
            st = {'shape': (C, Cs), 'a': torch.empty((C, *f), dtype=torch.float32, device=self.device),
                  'b': torch.empty((C, *f), dtype=torch.float32, device=self.device),
                  'seg': torch.empty((Cs, *f), dtype=torch.float32, device=self.device),
                  'rect': torch.empty(RECT_WS_DOUBLES, dtype=torch.float64, device=self.device)}
            self._dstate = st
        return st

    @staticmethod
    def _da5_moves(d, j):
        """The out-of-place passes of sample j's data, in order: signed permutation, median, mirror."""
        med = d['median'][j] is not None and any(v is not None for v in d['median'][j])
        return [d['signed'][j] is not None, med, d['mirror'][j] != 0]

    def apply_da5(self, bufs, d, j):
        """The DA5 recipe behind the SpatialTransform on sample j.  bufs: the buffers [C,D,H,W] the sample walks through,
        one more than _da5_moves counts -- the un-mirrored crop / warp result sits in bufs[0], every out-of-place pass
        (signed permutation of Rot90 + Transpose, median, mirror) moves it on, the last one is the batch slot.  Order:
        rot90 + transpose, median | blur, noise, additive brightness, contrast (clipped | not), low-res, gamma (inverted)
        twice, mirror, blank rectangles, brightness gradient, local gamma, sharpening."""
        bufs = list(bufs)
        x = bufs.pop(0)
        C = int(x.shape[0])
        shape = tuple(int(v) for v in x.shape[1:])
        st = self._intensity_state(C, x[0].numel())
        ds = self._dstate if self._dstate is not None and self._dstate['shape'][0] == C else self._da5_state(C, 1)
        sa, sb = st['stats'][0], st['stats'][1]

        def selected(vals):
            return [c for c, v in enumerate(vals) if v is not None]

        if d['signed'][j] is not None:
            nxt = bufs.pop(0)
            signed_permute(x, nxt, *d['signed'][j])
            x = nxt
        if self._da5_moves(d, j)[1]:
            nxt = bufs.pop(0)
            median_filter(x, nxt, d['median'][j])
            x = nxt
        if d['blur'][j] is not None and selected(d['blur'][j]):
            gaussian_blur_wide(x, d['blur'][j], st['blur'])
        if d['noise'][j] is not None:
            gaussian_noise(x, d['noise'][j][0], d['noise'][j][1])
        if d['brightness'][j] is not None and selected(d['brightness'][j]):
            da5_apply(x, OP_DA5_ADD, d['brightness'][j], channels=selected(d['brightness'][j]))
        if d['contrast'][j] is not None and selected(d['contrast'][j]):
            sel = selected(d['contrast'][j])
            channel_stats(x, sa, st['ws'], channels=sel)
            if d['oneof_contrast'] == 0:
                intensity_apply(x, OP_CONTRAST, d['contrast'][j], sa, channels=sel)
            else:
                da5_apply(x, OP_DA5_CONTRAST_NOCLIP, d['contrast'][j], sa, channels=sel)
        if d['lowres'][j] is not None:
            for c, z in enumerate(d['lowres'][j]):
                if z is None:
                    continue
                t = lowres_target_shape(shape, z)
                dpad = st['dpad'][:int(np.prod([v + 2 * LOWRES_PAD for v in t]))].view(
                    *[v + 2 * LOWRES_PAD for v in t])
                lowres_gather(x[c], dpad, t, 0)
                d4 = dpad.unsqueeze(0)
                channel_stats(d4, st['stats1'][0], st['ws'])
                bspline_prefilter(d4, 7)
                spatial_transform_data(d4, x[c:c + 1], lowres_affine(shape, t), 0, 0.0)
                intensity_apply(x[c:c + 1], OP_CLIP, None, st['stats1'][0])
        for key in ('gamma1', 'gamma2'):
            if d[key][j] is not None:
                channel_stats(x, sa, st['ws'])
                channel_stats(x, sb, st['ws'], pre_op=OP_GAMMA_INVERTED, gammas=d[key][j], pre_stats=sa)
                intensity_apply(x, OP_GAMMA_INVERTED, d[key][j], sa, sb)
        if d['mirror'][j] != 0:
            nxt = bufs.pop(0)
            signed_permute(x, nxt, (0, 1, 2), d['mirror'][j])
            x = nxt
        if bufs:
            raise RuntimeError("apply_da5: more buffers than out-of-place passes")
        if d['blank'][j] is not None:
            for c, rects in enumerate(d['blank'][j]):
                for lb, size in (rects or ()):
                    blank_rectangle(x, c, lb, size, ds['rect'])
        if d['gradient'][j] is not None and selected(d['gradient'][j]):
            local_gauss(x, LOCAL_ADDITIVE, d['gradient'][j])
        if d['local_gamma'][j] is not None and selected(d['local_gamma'][j]):
            channel_stats(x, sa, st['ws'], channels=selected(d['local_gamma'][j]))
            local_gauss(x, LOCAL_GAMMA, d['local_gamma'][j], sa)
        if d['sharpen'][j] is not None and selected(d['sharpen'][j]):
            channel_stats(x, sa, st['ws'], channels=selected(d['sharpen'][j]))
            # every move is done, so the walk's first scratch buffer is free
            sharpen(x, ds['a'], d['sharpen'][j], sa)
        return x

    def _cascade_state(self):
        st = self._cstate
        if st is None:
            K = len(self.cascade_labels)
            st = {'bits': cascade_bitplanes(K, self.final_patch_size, self.device),
                  'tmp': cascade_bitplanes(2, self.final_patch_size, self.device),
                  'ws': cascade_remove_workspace(self.final_patch_size, self.device),
                  'chosen': torch.zeros(2, dtype=torch.int32, device=self.device),
                  'threshold': cascade_removal_threshold(int(np.prod(self.final_patch_size)),
                                                         self.cascade_max_component_fraction)}
            self._cstate = st
        return st

    def apply_cascade(self, onehot, binary, remove):
        """The two cascade augmentations on one sample's K one-hot channels [K,D,H,W], in place: the binary operators on
        the packed bit-planes (packed once, unpacked once), then the component removal per drawn channel."""
        K = int(onehot.shape[0])
        shape = tuple(int(v) for v in onehot.shape[1:])
        st = self._cascade_state()
        if binary:
            cascade_pack(onehot, st['bits'])
            for c, op, radius in binary:
                cascade_morph(st['bits'], st['tmp'], K, shape, c, op, ball_rows(radius))
            cascade_unpack(st['bits'], onehot)
        for c, u, other in (remove or ()):
            cascade_remove(onehot[c], u, st['threshold'], st['ws'], st['chosen'],
                           other=None if other is None else onehot[other])

    def _da5_sample(self, j, data, seg, mod, tgt, box, spatial, d, shift, remove):
        """Sample j of a DA5 batch: crop (or crop + warp) un-mirrored into the head of the buffer walk, the recipe
        (apply_da5) ending in the batch slot `mod`; the seg takes Rot90, Transpose and the mirror as ONE signed
        permutation, since nothing touches it in between."""
        ds = self._da5_state(int(mod.shape[0]), int(tgt.shape[0]))
        n = sum(self._da5_moves(d, j))
        bufs = [ds['a'], ds['b'], ds['a']][:n] + [mod]
        sperm, smask = compose_signed_permutation(d['rot90'][j], d['transpose'][j], d['mirror'][j])
        seg_moves = not (sperm == (0, 1, 2) and smask == 0)
        sdst = ds['seg'] if seg_moves else tgt
        if spatial is None:
            lbs = [b + s for b, s in zip(box, shift)]
            crop_pad_data(data, bufs[0], lbs, 0, 0.0)
            crop_pad_seg(seg, sdst, lbs, 0, -1, replace=remove)
        else:
            pdata, pseg = self._scratch_for(data, seg)
            crop_pad_data(data, pdata, box, 0, 0.0)
            crop_pad_seg(seg, pseg, box, 0, -1)
            bspline_prefilter(pdata, 7)
            affine = spatial_affine(spatial, self.patch_size)
            spatial_transform_data(pdata, bufs[0], affine, 0, 0.0)
            spatial_transform_seg(pseg, sdst, affine, 0, replace=remove)
        if seg_moves:
            signed_permute(sdst, tgt, sperm, smask)
        self.apply_da5(bufs, d, j)

    def generate_train_batch(self, plan=None):
        plan = plan if plan is not None else self.plan_batch()
        intensity = None
        cascade = None
        if isinstance(plan[-1], dict) and plan[-1].get('cascade'):
            plan, cascade = plan[:-1], plan[-1]
            if self.cascade_labels is None:
                raise ValueError("generate_train_batch: a cascade plan needs a loader in cascade mode")
        da5 = None
        if len(plan) == 5 and isinstance(plan[3], dict) and plan[3].get('da5'):
            if not self.da5:
                raise ValueError("generate_train_batch: a DA5 plan needs a loader with da5=True")
            keys, boxes, spatial, da5, flips = plan
        elif len(plan) == 3:
            keys, boxes, flips = plan
            spatial = [None] * len(keys)
        elif len(plan) == 4:
            keys, boxes, spatial, flips = plan
        else:
            keys, boxes, spatial, intensity, flips = plan
        # MaskTransform reads the seg before RemoveLabel: keep the -1 in the stores and replace in the mask pass
        remove = (-1, 0) if self.mask_channels is None else None
        M = self.num_modalities
        data_all = torch.empty(self.data_shape, dtype=torch.float32, device=self.device)
        # cascade mode: both seg channels are cropped, padded and warped together; channel 0 becomes the target
        # (MoveSegAsOneHotToData removes channel 1 from the seg)
        nseg = self.seg_shape[1] if self.cascade_labels is None else 2
        target = torch.empty((self.seg_shape[0], nseg, *self.seg_shape[2:]), dtype=torch.float32, device=self.device)
        # an unmodified sample is the centre crop of the initial patch at (n - f) // 2 (center_crop_aug): cut straight
        # from the resident case (no-op shift when patch_size == final_patch_size)
        shift = [(n - f) // 2 for n, f in zip(self.patch_size, self.final_patch_size)]
        props = []
        for j, k in enumerate(keys):
            data, seg, properties = self._case(k)
            mod = data_all[j] if self.cascade_labels is None else data_all[j, :M]
            if da5 is not None:
                self._da5_sample(j, data, seg, mod, target[j], boxes[j], spatial[j], da5, shift, remove)
                if self.mask_channels is not None:
                    mask_remove_label(mod, target[j], self.mask_channels, replace=(-1, 0))
                props.append(properties)
                continue
            if spatial[j] is None:
                lbs = [b + s for b, s in zip(boxes[j], shift)]
                crop_pad_data(data, mod, lbs, flips[j], 0.0)
                crop_pad_seg(seg, target[j], lbs, flips[j], -1, replace=remove)
            else:
                pdata, pseg = self._scratch_for(data, seg)
                crop_pad_data(data, pdata, boxes[j], 0, 0.0)
                crop_pad_seg(seg, pseg, boxes[j], 0, -1)
                if self.do_dummy_2d_data_aug:
                    bspline_prefilter(pdata, 6)
                    affine = spatial_affine_2d(spatial[j], self.patch_size[1:])
                    spatial_transform_data_2d(pdata, mod, affine, flips[j], 0.0)
                    spatial_transform_seg_2d(pseg, target[j], affine, flips[j], replace=remove)
                else:
                    bspline_prefilter(pdata, 7)
                    affine = spatial_affine(spatial[j], self.patch_size)
                    spatial_transform_data(pdata, mod, affine, flips[j], 0.0)
                    spatial_transform_seg(pseg, target[j], affine, flips[j], replace=remove)
            if intensity is not None:
                self.apply_intensity(mod, intensity[j], flips[j])
            if self.mask_channels is not None:
                mask_remove_label(mod, target[j], self.mask_channels, replace=(-1, 0))
            if self.cascade_labels is not None:
                cascade_onehot(target[j, 1], data_all[j, M:], self.cascade_labels)
                if cascade is not None:
                    self.apply_cascade(data_all[j, M:], cascade['binary'][j], cascade['remove'][j])
            props.append(properties)
        if self.cascade_labels is not None:
            target = target[:, :1].contiguous()
        if self.deep_supervision_scales is not None:
            target = [downsample_seg(target, s) for s in self.deep_supervision_scales]
        return {'data': data_all, 'target': target, 'properties': props, 'keys': keys}

    def __iter__(self):
        return self

    def __next__(self):
        return self.generate_train_batch()


class DeviceDataLoader2D(DeviceDataLoader3D):
    """nnUNetDataLoader2D (data_loader_2d.py:7-86) over the same HBM-resident [C,D,H,W] cases: per sample, in the
    reference's numpy-RNG order, the oversample decision, the class draw when forced, the slice draw (from the class's z
    column, or uniform over the slices), get_bbox on the 2-D shape with that slice's locations (columns 0, 2, 3) and
    overwrite_class, then crop and pad (data 0, seg -1).  The device work is DeviceDataLoader3D's on the [C,1,H,W] slice:
    a box is (slice, y, x) with a patch of depth 1, so the crop kernels cut the slice straight out of the resident volume;
    the SpatialTransform is the in-plane one (augment_spatial with dim == 2 is what the dummy 2-D mode runs per slice,
    DESIGN 19: rotation about x only); mirroring runs over the two axes (bits H and W); the deep-supervision targets are
    the order-0 picks.  Batches are data [B,C,H,W] and target a list of [B,1,h,w] (one tensor without scales).
    patch_size / final_patch_size / mirror_axes / deep_supervision_scales are 2-D, as the 2-D trainer passes them."""

    def __init__(self, data, batch_size, patch_size, final_patch_size, label_manager, oversample_foreground_percent=0.0,
                 sampling_probabilities=None, pad_sides=None, probabilistic_oversampling=False, mirror_axes=None,
                 deep_supervision_scales=None, device="cuda:0", rotation_for_DA=None, scale_range=(0.7, 1.4),
                 p_rot_per_sample=0.2, p_scale_per_sample=0.2, p_rot_per_axis=1.0, intensity_augmentation=False,
                 mask_channels=None, cascade_labels=None, cascade_augmentation=False):
        if len(patch_size) != 2 or len(final_patch_size) != 2:
            raise ValueError("DeviceDataLoader2D: patch_size and final_patch_size have two axes")
        if cascade_labels is not None or cascade_augmentation:
            raise NotImplementedError("DeviceDataLoader2D: the cascade mode (cascade_labels) is not built for the 2d "
                                      "configuration; nnU-Net plans no 2-D cascade")
        if intensity_augmentation:
            # the blur kernel filters all three axes of a volume; on an extent-1 axis that is a multiplication by the sum of
            # the weights, which the 2-D transform does not do -- not routed around yet, so not offered
            raise NotImplementedError("DeviceDataLoader2D: the intensity stage is not built for the 2d configuration")
        if mask_channels is not None and any(mask_channels):
            raise NotImplementedError("DeviceDataLoader2D: MaskTransform belongs to the intensity stage, which is not built "
                                      "for the 2d configuration")
        if mirror_axes and max(mirror_axes) > 1:
            raise ValueError("DeviceDataLoader2D: mirror_axes are axes of the slice, (0, 1) at most")
        super().__init__(data, batch_size, (1, *patch_size), (1, *final_patch_size), label_manager,
                         oversample_foreground_percent=oversample_foreground_percent,
                         sampling_probabilities=sampling_probabilities,
                         pad_sides=None if pad_sides is None else (0, *pad_sides),
                         probabilistic_oversampling=probabilistic_oversampling,
                         mirror_axes=[a + 1 for a in mirror_axes] if mirror_axes else None,
                         deep_supervision_scales=None if deep_supervision_scales is None
                         else [(1, *s) for s in deep_supervision_scales],
                         device=device, rotation_for_DA=rotation_for_DA, scale_range=scale_range,
                         p_rot_per_sample=p_rot_per_sample, p_scale_per_sample=p_scale_per_sample,
                         p_rot_per_axis=p_rot_per_axis, do_dummy_2d_data_aug=True)

    def get_bbox_2d(self, data_shape, force_fg, class_locations, overwrite_class=None, verbose=False):
        """get_bbox over the two axes of a slice (class_locations rows are (c, y, x))."""
        full = (self.patch_size, self.need_to_pad)
        self.patch_size, self.need_to_pad = self.patch_size[1:], self.need_to_pad[1:]
        try:
            return self.get_bbox(data_shape, force_fg, class_locations, overwrite_class, verbose)
        finally:
            self.patch_size, self.need_to_pad = full

    def select_slice_and_bbox(self, j, shape, properties):
        """data_loader_2d.py:17-62 for sample j of a case of shape [C,D,H,W]: (slice, lower corner (y, x))."""
        force_fg = self.get_do_oversample(j)
        locations = properties['class_locations']
        if not force_fg:
            selected = self.annotated_classes_key if self.has_ignore else None
        else:
            eligible = [k for k in locations.keys() if len(locations[k]) > 0]
            if len(eligible) > 1:   # the all-annotated-classes key only serves cases that have nothing more specific
                for i, k in enumerate(eligible):
                    if isinstance(k, tuple) and k == self.annotated_classes_key:
                        del eligible[i]
                        break
            selected = eligible[np.random.choice(len(eligible))] if len(eligible) > 0 else None
        if selected is not None:
            z = int(np.random.choice(locations[selected][:, 1]))
            rows = locations[selected]
            in_slice = {selected: rows[rows[:, 1] == z][:, (0, 2, 3)]}
        else:
            z = int(np.random.choice(shape[1]))
            in_slice = None
        lbs, _ = self.get_bbox_2d(tuple(shape[2:]), force_fg if selected is not None else None, in_slice,
                                  overwrite_class=selected)
        return z, [int(v) for v in lbs]

    def plan_batch(self):
        """keys, then per sample (oversample?, class, slice, bbox) -> boxes (slice, y, x); then per sample the
        SpatialTransform draws (only with rotation_for_DA), then per sample the mirror draw."""
        keys = self.get_indices()
        boxes = []
        for j, k in enumerate(keys):
            data, _, properties = self._case(k)
            z, lbs = self.select_slice_and_bbox(j, tuple(data.shape), properties)
            boxes.append([z] + lbs)
        if self.rotation_for_DA is None:
            return list(keys), boxes, [self.draw_mirror() for _ in keys]
        spatial = [self.draw_spatial() for _ in keys]
        return list(keys), boxes, spatial, [self.draw_mirror() for _ in keys]

    def generate_train_batch(self, plan=None):
        out = super().generate_train_batch(plan)
        out['data'] = out['data'].squeeze(2)
        t = out['target']
        out['target'] = [i.squeeze(2) for i in t] if isinstance(t, list) else t.squeeze(2)
        return out
