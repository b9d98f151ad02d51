"""GPU tests of the device feed's DA5 stage (csrc/feed_da5.hip) against the numpy / scipy restatement in
feed_da5_ref.py: the exact median, every new kernel at odd shapes against fp64, the signed permutation against numpy,
then whole loader batches in the reference order and a train step."""
import itertools

import numpy as np
import pytest
import torch

import feed_da5_ref as REF
import feed_intensity_ref as IREF
from multimodal_mvd_seg_amd import dataloading as DLD

DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu

SHAPES = [(5, 7, 9), (1, 6, 13), (24, 40, 33)]
ALL = {k: 1.0 for k in DLD.DA5_PROBABILITIES}


def G(a):
    return torch.from_numpy(np.array(a, dtype=np.float32, order='C', copy=True)).to(DEV)


def sample(shape, C=3, seed=0):
    """C channels: standard normal * 3 + 1, all-negative, constant."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((C, *shape)) * 3 + 1).astype(np.float32)
    if C > 1:
        x[1] = -np.abs(x[1]) - 2
    if C > 2:
        x[2] = -1.25
    return x


def close(got, ref, k, x):
    t = k * max(1.0, float(np.abs(x).max()))
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"max error {err:.3e}, bar {t:.3e}")
    assert np.isfinite(got).all() and err <= t, (err, t)


def stats_of(g):
    C = int(g.shape[0])
    st = torch.empty((C, 4), dtype=torch.float64, device=DEV)
    DLD.channel_stats(g, st, DLD.stats_workspace(C, DEV))
    return st


# ------------------------------------------------------------------------------------------------ median
def run_median(x, sizes):
    g = G(x)
    out = torch.full_like(g, float('nan'))
    DLD.median_filter(g, out, sizes)
    return out.cpu().numpy()


def check_median(x, sizes):
    got = run_median(x, sizes)
    for c, s in enumerate(sizes):
        if s:
            assert np.array_equal(got[c], REF.median(x[c], s)), (c, s)
        else:   # a copy, bit for bit
            assert np.array_equal(got[c].view(np.uint32), x[c].view(np.uint32))


@pytest.mark.parametrize("shape", [(5, 7, 9), (1, 6, 13), (2, 3, 40), (16, 16, 16)])
@pytest.mark.parametrize("s", range(2, 8))
def test_median_is_scipy(shape, s):
    check_median(np.random.default_rng(s).standard_normal((1, *shape)).astype(np.float32), [s])


@pytest.mark.parametrize("s", [2, 7])
def test_median_across_tile_edges(s):
    """(33, 20, 70) crosses the 8^3 tile on every axis; (9, 9, 9) is one voxel past it."""
    for shape in ((33, 20, 70), (9, 9, 9)):
        check_median(np.random.default_rng(1).standard_normal((1, *shape)).astype(np.float32), [s])


def test_median_ties_constant_and_signed_zero():
    rng = np.random.default_rng(2)
    ties = rng.integers(0, 4, (1, 11, 9, 13)).astype(np.float32)
    const = np.full((1, 6, 9, 10), -2.5, np.float32)
    zeros = rng.choice(np.array([0.0, -0.0, 1.0, -1.0], np.float32), (1, 9, 10, 11))
    for x in (ties, const, zeros):
        for s in (2, 3, 4, 7):
            check_median(x, [s])


def test_median_per_channel_sizes():
    x = np.random.default_rng(3).standard_normal((5, 10, 12, 19)).astype(np.float32)
    x[3, 0, 0, :4] = [0.0, -0.0, np.float32(1e-40), -np.float32(1e-40)]   # the copy keeps every bit
    check_median(x, [0, 2, 7, 0, 4])
    check_median(x, [None, 3, None, None, 6])


def test_median_48_cubed_size_7():
    check_median(np.random.default_rng(4).standard_normal((1, 48, 48, 48)).astype(np.float32), [7])


def test_median_refusals():
    g = G(np.zeros((1, 4, 4, 4)))
    out = torch.empty_like(g)
    for s in (1, 8, -3):
        with pytest.raises(RuntimeError, match="sizes are 2..7"):
            DLD.median_filter(g, out, [s])
    with pytest.raises(RuntimeError):
        DLD.median_filter(g, g, [3])


# ------------------------------------------------------------------------------------------------ pointwise and stencil kernels
@pytest.mark.parametrize("shape", SHAPES)
def test_sharpen(shape):
    x = sample(shape, 4, 5)
    x[3] = sample(shape, 1, 6)[0] * 40
    g = G(x)
    DLD.sharpen(g, torch.empty_like(g), [0.1, 1.0, 0.63, None], stats_of(g))
    got = g.cpu().numpy()
    for c, s in enumerate((0.1, 1.0, 0.63)):
        close(got[c], REF.sharpen(x[c], s), 1e-5, x[c])
    assert np.array_equal(got[3], x[3])                     # skipped channel untouched
    assert np.array_equal(got[2], x[2])                     # a constant channel stays what it is
    g = G(x)
    DLD.sharpen(g, torch.empty_like(g), [None, None, None, 0.9], stats_of(g))
    close(g.cpu().numpy()[3], REF.sharpen(x[3], 0.9), 1e-5, x[3])


def local_params(shape):
    """loc inside the patch, outside on either side, and exactly on a voxel."""
    n = np.asarray(shape, dtype=np.float64)
    return [([max(1.0, v / 5) for v in n], list(n * 0.37 + 0.21), -3.2),
            ([max(1.0, v / 2) for v in n], list(-0.45 * n - 0.3), 4.1),
            ([max(1.5, v * 0.9) for v in n], list(1.45 * n + 0.6), 2.5),
            ([max(1.0, v / 3) for v in n], [float(int(v) // 2) for v in n], 0.3)]


@pytest.mark.parametrize("mode", [DLD.LOCAL_ADDITIVE, DLD.LOCAL_GAMMA])
@pytest.mark.parametrize("shape", SHAPES)
def test_local_gauss(shape, mode):
    prm = local_params(shape)
    if mode == DLD.LOCAL_GAMMA:     # gammas of both branches, (0.01, 0.8) and (1.5, 4)
        prm = [(s, l, a) for (s, l, _), a in zip(prm, (0.01, 3.9, 1.6, 0.75))]
    x = np.concatenate([sample(shape, 3, 7), sample(shape, 1, 8) * 20, sample(shape, 1, 9)])
    params = prm[:1] + [prm[1], prm[2], prm[3], None]
    g = G(x)
    DLD.local_gauss(g, mode, params, stats_of(g) if mode == DLD.LOCAL_GAMMA else None)
    got = g.cpu().numpy()
    fn = REF.gradient if mode == DLD.LOCAL_ADDITIVE else REF.local_gamma
    for c in range(4):
        close(got[c], fn(x[c], *params[c]), 1e-5 if mode == DLD.LOCAL_ADDITIVE else 1e-4, x[c])
    assert np.array_equal(got[4], x[4])
    if mode == DLD.LOCAL_GAMMA:     # mx == mn: finite, and the oracle's value
        assert np.allclose(got[2], -1.25, rtol=0, atol=1e-6)


@pytest.mark.parametrize("shape", SHAPES)
def test_blank_rectangle(shape):
    x = sample(shape, 3, 10)
    n = shape
    far = ([max(0, v - max(1, v // 3)) for v in n], [min(v, max(1, v // 3)) for v in n])      # touches the far border
    one = ([v // 2 for v in n], [1, 1, 1])
    a = ([0, n[1] // 4, n[2] // 4], [n[0], max(1, n[1] // 2), max(1, n[2] // 2)])
    b = ([0, n[1] // 3, n[2] // 3], [max(1, n[0] // 2), max(1, n[1] // 2), max(1, n[2] // 2)])    # overlaps a
    g = G(x)
    ws = torch.empty(DLD.RECT_WS_DOUBLES, dtype=torch.float64, device=DEV)
    plan = {0: [one, far], 1: [a, b], 2: [a]}
    for c, rects in plan.items():
        for lb, size in rects:
            DLD.blank_rectangle(g, c, lb, size, ws)
    got = g.cpu().numpy()
    for c, rects in plan.items():
        close(got[c], REF.blank(x[c], rects), 1e-5, x[c])
    with pytest.raises(RuntimeError, match="inside the patch"):
        DLD.blank_rectangle(g, 0, [0, 0, 1], list(n), ws)


@pytest.mark.parametrize("shape", SHAPES)
def test_additive_brightness_and_unclipped_contrast(shape):
    x = sample(shape, 3, 11)
    g = G(x)
    DLD.da5_apply(g, DLD.OP_DA5_ADD, [0.7, None, -1.3], channels=[0, 2])
    got = g.cpu().numpy()
    close(got, x.astype(np.float64) + np.array([0.7, 0, -1.3])[:, None, None, None], 1e-5, x)
    assert np.array_equal(got[1], x[1])
    for f in ([0.5, 2.0, 1.7], [1.9, 0.55, 0.8]):
        g = G(x)
        DLD.da5_apply(g, DLD.OP_DA5_CONTRAST_NOCLIP, f, stats_of(g))
        close(g.cpu().numpy(), np.stack([REF.contrast_noclip(x[c], f[c]) for c in range(3)]), 1e-5, x)


@pytest.mark.parametrize("sigma", [0.3, 1.1, 1.5])
@pytest.mark.parametrize("shape", SHAPES)
def test_wide_blur(shape, sigma):
    x = sample(shape, 3, 12)
    g = G(x)
    ws = torch.empty(2 * 3 * g[0].numel(), dtype=torch.float32, device=DEV)
    DLD.gaussian_blur_wide(g, [sigma, None, sigma * 0.9], ws)
    got = g.cpu().numpy()
    close(got[0], IREF.blur(x[0], sigma), 1e-5, x)
    assert np.array_equal(got[1], x[1])
    close(got[2], IREF.blur(x[2], sigma * 0.9), 1e-5, x)
    if sigma <= 1.1:    # the same arithmetic as the narrow entry
        g2 = G(x)
        DLD.gaussian_blur(g2, [sigma, None, sigma * 0.9], ws)
        assert torch.equal(g, g2)
    with pytest.raises(ValueError):
        DLD.gaussian_blur_wide(g, [1.6, None, None], ws)
    with pytest.raises(ValueError):
        DLD.gaussian_blur(g, [1.5, None, None], ws)


# ------------------------------------------------------------------------------------------------ signed permutation
@pytest.mark.parametrize("shape", [(6, 6, 6), (6, 6, 10), (33, 33, 33)])
def test_signed_permute_is_numpy(shape):
    x = np.random.default_rng(13).standard_normal((2, *shape)).astype(np.float32)
    g = G(x)
    out = torch.empty_like(g)
    perms = list(itertools.permutations(range(3))) if shape[2] == shape[0] else [(0, 1, 2), (1, 0, 2)]
    for perm in perms:
        for mask in range(8):
            out.fill_(float('nan'))
            DLD.signed_permute(g, out, perm, mask)
            ref = IREF.mirror(np.transpose(x, (0, *[a + 1 for a in perm])), mask)
            assert np.array_equal(out.cpu().numpy(), ref), (perm, mask)


def test_signed_permute_refuses_unequal_axes():
    g = G(np.zeros((1, 6, 6, 10)))
    out = torch.empty_like(g)
    for perm in ((0, 2, 1), (2, 1, 0), (1, 2, 0)):
        with pytest.raises(RuntimeError, match="equal length"):
            DLD.signed_permute(g, out, perm, 0)
    with pytest.raises(RuntimeError, match="permutation"):
        DLD.signed_permute(g, out, (0, 0, 2), 0)


# ------------------------------------------------------------------------------------------------ the loader
class _DS:
    def __init__(self, shapes, C, seed):
        rng = np.random.default_rng(seed)
        self.cases = {}
        for i, shp in enumerate(shapes):
            data = (rng.standard_normal((C, *shp)) * 2 + 0.5).astype(np.float32)
            seg = np.zeros((1, *shp), dtype=np.int16)
            zz, yy, xx = np.meshgrid(*[np.arange(v) for v in shp], indexing='ij')
            for lab in (1, 2, 3):
                ctr = rng.integers(0, shp)
                seg[0][(zz - ctr[0]) ** 2 + (yy - ctr[1]) ** 2 + (xx - ctr[2]) ** 2 < 60] = lab
            seg[0][(zz + yy) < min(shp) // 2] = -1     # outside the brain, as crop_to_nonzero leaves it
            self.cases[f"c{i}"] = (data, seg, {"class_locations": {c: np.argwhere(seg == c) for c in (1, 2, 3)}})

    def keys(self):
        return self.cases.keys()

    def load_case(self, k):
        return self.cases[k]


class _Labels:
    all_labels = [1, 2, 3]
    has_ignore_label = False


F = (24, 24, 24)
ROT = {ax: (-np.pi / 6, np.pi / 6) for ax in 'xyz'}
SCALES = [[1, 1, 1], [0.5, 0.5, 0.5]]


def loaders(rotation, probs, ds, **kw):
    n = (34, 34, 34) if rotation else F
    args = dict(oversample_foreground_percent=0.33, mirror_axes=(0, 1, 2), device=DEV,
                rotation_for_DA=ROT if rotation else None, deep_supervision_scales=SCALES, scale_range=(0.7, 1.43))
    on = DLD.DeviceDataLoader3D(ds, 2, n, F, _Labels(), da5=True, da5_probabilities=probs, mask_channels=[True, False],
                                **args, **kw)
    off = DLD.DeviceDataLoader3D(ds, 2, n, F, _Labels(), **args)
    return on, off


def stage_input_seg(dl, plan, j):
    """The un-mirrored seg patch of sample j before RemoveLabel (the -1 the mask reads), from the feed's tested kernels."""
    keys, boxes, spatial = plan[:3]
    _, seg, _ = dl._case(keys[j])
    out = torch.empty((1, *dl.final_patch_size), dtype=torch.float32, device=DEV)
    if spatial[j] is None:
        shift = [(n - f) // 2 for n, f in zip(dl.patch_size, dl.final_patch_size)]
        DLD.crop_pad_seg(seg, out, [b + s for b, s in zip(boxes[j], shift)], 0, -1)
    else:
        pseg = torch.empty((1, *dl.patch_size), dtype=torch.float32, device=DEV)
        DLD.crop_pad_seg(seg, pseg, boxes[j], 0, -1)
        DLD.spatial_transform_seg(pseg, out, DLD.spatial_affine(spatial[j], dl.patch_size), 0)
    return out.cpu().numpy()


@pytest.mark.parametrize("rotation", [True, False])
@pytest.mark.parametrize("probs", ["all_on", "reference"])
def test_loader_batches_against_the_oracle_chain(probs, rotation):
    ds = _DS([(40, 40, 40), (40, 40, 40)], 2, 7)
    kw = dict(p_rot_per_sample=1.0, p_scale_per_sample=1.0, p_rot_per_axis=1.0) if probs == "all_on" else \
        dict(p_rot_per_sample=0.4, p_scale_per_sample=0.2, p_rot_per_axis=0.5)
    on, off = loaders(rotation, ALL if probs == "all_on" else None, ds, **kw)
    np.random.seed(4)
    median_hit = per_axis_scale = 0
    masks = set()
    nb = 4 if probs == "all_on" else 10
    for b in range(nb):
        plan = on.plan_batch()
        keys, boxes, spatial, d, flips = plan
        if probs == "all_on":     # every mirror mask over the 8 samples (the plan is what both sides read)
            d['mirror'] = [2 * b, 2 * b + 1]
            plan = (keys, boxes, spatial, d, list(d['mirror']))
        masks.update(d['mirror'])
        median_hit += d['oneof_blur'] == 0 and any(m is not None and any(m) for m in d['median'])
        per_axis_scale += any(s is not None and isinstance(s[3], tuple) for s in spatial)
        b1 = on.generate_train_batch(plan)
        b2 = on.generate_train_batch(plan)
        assert torch.equal(b1["data"], b2["data"]) and all(torch.equal(a, c) for a, c in zip(b1["target"], b2["target"]))
        zero = [0] * len(keys)
        base = off.generate_train_batch((keys, boxes, spatial, zero) if rotation else (keys, boxes, zero))
        data, base_d = b1["data"].cpu().numpy(), base["data"].cpu().numpy()
        t0 = b1["target"][0].cpu().numpy()
        for j in range(2):
            pre = REF.signed(stage_input_seg(on, plan, j), d['rot90'][j], d['transpose'][j], d['mirror'][j])
            ref = IREF.mask(REF.chain(base_d[j], d, j), pre, [0])
            close(data[j], ref, 1e-4, np.maximum(np.abs(base_d[j]), np.abs(ref)))
            rem = pre.copy()
            rem[rem == -1] = 0
            assert np.array_equal(t0[j], rem)
        assert torch.equal(b1["target"][1], DLD.downsample_seg(b1["target"][0], SCALES[1]))
    assert median_hit > 0     # the median branch of the OneOf ran
    if probs == "all_on":
        assert masks == set(range(8))
        assert not rotation or per_axis_scale == nb


def test_da5_off_is_bit_identical_to_the_intensity_path():
    ds = _DS([(40, 40, 40)], 2, 9)
    for r, n in ((None, F), (ROT, (34, 34, 34))):
        args = dict(mirror_axes=(0, 1, 2), device=DEV, rotation_for_DA=r, intensity_augmentation=True,
                    mask_channels=[True, False], p_noise=0.5, p_lowres=0.5, p_gamma=0.5, p_scale_per_sample=0.6)
        old = DLD.DeviceDataLoader3D(ds, 2, n, F, _Labels(), **args)
        new = DLD.DeviceDataLoader3D(ds, 2, n, F, _Labels(), da5=False, da5_probabilities=ALL, **args)
        for seed in range(3):
            np.random.seed(seed)
            a = old.generate_train_batch()
            np.random.seed(seed)
            b = new.generate_train_batch()
            assert torch.equal(a["data"], b["data"]) and torch.equal(a["target"], b["target"])


def test_da5_trainer_step():
    from multimodal_mvd_seg_amd import trainer
    patch = (32, 32, 32)
    plans = trainer.make_plans(patch, [[1, 1, 1], [2, 2, 2], [2, 2, 2]], batch_size=2, base_features=16, max_features=32)
    dj = {"channel_names": {"0": "a", "1": "b"}, "labels": {"background": 0, "a": 1, "b": 2, "c": 3}}
    torch.manual_seed(0)
    tr = trainer.nnUNetTrainerDA5MI355(plans, "3d_fullres", 0, dj, device=DEV)
    tr.initialize()
    tr.on_train_epoch_start()
    dl = tr.get_device_dataloader(_DS([(60, 64, 56)], 2, 8), da5_probabilities=ALL)
    assert dl.da5 and dl.intensity_augmentation and dl.patch_size == tuple(
        int(v) for v in DLD.get_patch_size(patch, *[ROT[a] for a in 'xyz'], (0.7, 1.43)))
    np.random.seed(0)
    b = next(dl)
    assert tuple(b["data"].shape) == (2, 2, *patch) and torch.isfinite(b["data"]).all()
    assert np.isfinite(float(tr.train_step(b)["loss"]))
