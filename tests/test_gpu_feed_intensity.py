"""GPU tests of the device feed's intensity stage (csrc/feed_intensity.hip) against the fp64 numpy / scipy
restatement in feed_intensity_ref.py: each kernel on odd shapes (a length-1 axis, a constant channel, negative data),
then whole loader batches in the reference order, a full-size sample and a train step."""
import numpy as np
import pytest
import torch
from scipy import stats as sps

import feed_intensity_ref as REF
from multimodal_mvd_seg_amd import dataloading as DLD

DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu

SHAPES = [(17, 23, 29), (1, 23, 29), (9, 1, 12), (5, 6, 1)]
ALL_ON = dict(p_noise=1.0, p_blur=1.0, p_blur_per_channel=1.0, p_brightness=1.0, p_contrast=1.0, p_lowres=1.0,
              p_lowres_per_channel=1.0, p_gamma_inverted=1.0, p_gamma=1.0)


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


def tol(x, k=1e-5):
    return k * max(1.0, float(np.abs(x).max()))


def close(got, ref, k, x=None):
    t = tol(x if x is not None else ref, k)
    err = float(np.abs(got.astype(np.float64) - ref).max())
    assert np.isfinite(got).all() and err <= t, (err, t)


def empty_it():
    return dict.fromkeys(DLD.INTENSITY_KEYS)


class _DS:
    def __init__(self, shapes, C, seed, neg_label=True):
        rng = np.random.default_rng(seed)
        self.cases = {}
        for i, shp in enumerate(shapes):
            data = (rng.standard_normal((C, *shp)) * 2 + 0.5).astype(np.float32)
            seg = np.zeros((1, *shp), dtype=np.int16)
            zz, yy, xx = np.meshgrid(*[np.arange(v) for v in shp], indexing='ij')
            for lab in (1, 2, 3):
                ctr = rng.integers(0, shp)
                seg[0][(zz - ctr[0]) ** 2 + (yy - ctr[1]) ** 2 + (xx - ctr[2]) ** 2 < 30] = lab
            if neg_label:  # an outside-the-brain region (-1), as nnU-Net's crop_to_nonzero leaves it
                seg[0][(zz + yy) < min(shp) // 2] = -1
            self.cases[f"c{i}"] = (data, seg, {"class_locations": {c: np.argwhere(seg == c) for c in (1, 2, 3)}})

    def keys(self):
        return self.cases.keys()

    def load_case(self, k):
        return self.cases[k]


class _Labels:
    all_labels = [1, 2, 3]
    has_ignore_label = False


def stage_loader(shape, C=3):
    """A loader whose batch patch is `shape`: its apply_intensity runs the stage on a given sample."""
    return DLD.DeviceDataLoader3D(_DS([tuple(max(v, 4) for v in shape)], C, 0, False), 1, shape, shape, _Labels(),
                                  device=DEV, intensity_augmentation=True)


def run_stage(x, it, flip=0):
    dl = stage_loader(x.shape[1:], x.shape[0])
    g = G(x)
    dl.apply_intensity(g, it, flip)
    return g.cpu().numpy()


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("shape", SHAPES)
def test_channel_stats(shape):
    x = sample(shape, 3, 1)
    st = torch.empty((3, 4), dtype=torch.float64, device=DEV)
    DLD.channel_stats(G(x), st, DLD.stats_workspace(3, DEV))
    got = st.cpu().numpy()
    x64 = x.astype(np.float64)
    ref = np.stack([x64.reshape(3, -1).mean(1), x64.reshape(3, -1).std(1), x64.reshape(3, -1).min(1),
                    x64.reshape(3, -1).max(1)], 1)
    assert np.allclose(got, ref, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("sigma", [0.5, 0.73, 1.0])
@pytest.mark.parametrize("shape", SHAPES)
def test_blur(shape, sigma):
    x = sample(shape, 3, 2)
    it = empty_it()
    it['blur'] = [sigma, None, sigma * 0.9]
    got = run_stage(x, it)
    close(got[0], REF.blur(x[0], sigma), 1e-5, x)
    assert np.array_equal(got[1], x[1])  # unselected channel untouched
    close(got[2], REF.blur(x[2], sigma * 0.9), 1e-5, x)


@pytest.mark.parametrize("shape", SHAPES)
def test_brightness_contrast_gammas(shape):
    x = sample(shape, 3, 3)
    x64 = x.astype(np.float64)
    it = empty_it()
    it['brightness'] = [0.8, 1.2, 0.77]
    close(run_stage(x, it), x64 * np.array([0.8, 1.2, 0.77])[:, None, None, None], 1e-5, x)
    for f in ([0.8, 1.2, 0.9], [1.24, 0.76, 1.1]):
        it = empty_it()
        it['contrast'] = f
        close(run_stage(x, it), np.stack([REF.contrast(x64[c], f[c]) for c in range(3)]), 1e-5, x)
    for key, inv in (('gamma', False), ('gamma_inverted', True)):
        for g in ([0.7, 1.45, 0.9], [1.3, 0.75, 1.0]):
            it = empty_it()
            it[key] = g
            got = run_stage(x, it)
            close(got, np.stack([REF.gamma(x64[c], g[c], inv) for c in range(3)]), 1e-4, x)
            assert np.allclose(got[2], -1.25, rtol=0, atol=1e-6)  # constant channel stays constant


@pytest.mark.parametrize("zoom", [0.5, 0.63, 1.0])
@pytest.mark.parametrize("shape", [(17, 23, 29), (1, 23, 29), (9, 14, 1)])
def test_lowres_every_flip(shape, zoom):
    x = sample(shape, 3, 4)
    x[0, 0] += 10  # a step for the clip
    it = empty_it()
    it['lowres'] = [zoom, None, 0.55]
    for flip in range(8):
        xs = REF.mirror(x, flip)  # what the loader stores
        got = REF.mirror(run_stage(xs, it, flip), flip)
        ref0, d0 = REF.lowres(x[0], zoom)
        close(got[0], ref0, 1e-4, x)
        assert got[0].min() >= d0.min() - 1e-6 and got[0].max() <= d0.max() + 1e-6  # the clip
        assert np.array_equal(got[1], x[1])
        close(got[2], REF.lowres(x[2], 0.55)[0], 1e-4, x)
        if zoom == 1.0:
            close(got[0], x[0].astype(np.float64), 1e-5, x)


def test_lowres_gather_is_scipy_order0_with_ties():
    """The order-0 index reproduces scipy's own fp64 rounding at exact ties (n = 2 -> t = 49 and the like)."""
    rng = np.random.default_rng(0)
    for n, t in ((2, 49), (4, 49), (7, 5), (13, 8), (64, 33)):
        x = rng.standard_normal((n, 3, n)).astype(np.float32)
        dpad = torch.empty((t + 24, 3 + 24, t + 24), dtype=torch.float32, device=DEV)
        DLD.lowres_gather(G(x), dpad, (t, 3, t))
        ref = np.pad(REF.ndimage.zoom(x.astype(np.float64), (t / n, 1, t / n), order=0, mode='nearest',
                                      grid_mode=True), 12, mode='edge')
        assert np.array_equal(dpad.cpu().numpy(), ref.astype(np.float32))


def test_mask_and_remove_label():
    rng = np.random.default_rng(5)
    x = sample((7, 9, 11), 3, 5)
    s = rng.integers(-1, 3, (1, 7, 9, 11)).astype(np.float32)
    gx, gs = G(x), G(s)
    DLD.mask_remove_label(gx, gs, [0, 2], replace=(-1, 0))
    assert np.array_equal(gx.cpu().numpy(), REF.mask(x, s, [0, 2]))
    s2 = s.copy()
    s2[s2 == -1] = 0
    assert np.array_equal(gs.cpu().numpy(), s2)


def test_noise_matches_the_host_restatement_and_is_normal():
    shape = (4, 80, 80, 80)
    x = np.zeros(shape, np.float32)
    x[1] = np.linspace(-50, 50, x[1].size, dtype=np.float32).reshape(shape[1:])
    key, sigma = 2 ** 62 + 12345, 0.0731
    for flip in (0, 5):
        it = empty_it()
        it['noise'] = (sigma, key)
        got = REF.mirror(run_stage(REF.mirror(x, flip), it, flip), flip)
        ref = x.astype(np.float64) + sigma * REF.noise_field(key, shape, flip)
        err = np.abs(got - ref)
        assert float(err.max()) <= 1e-5 * sigma + 1e-6 * max(1.0, float(np.abs(x).max())), float(err.max())
    z = (got[0].astype(np.float64) / sigma).ravel()
    z = np.concatenate([z, (got[2:].astype(np.float64) / sigma).ravel()])
    assert z.size >= 1_000_000
    assert abs(z.mean()) < 5e-3 and abs(z.std() - 1) < 5e-3
    assert sps.kstest(z, 'norm').pvalue > 1e-3
    # a different key gives a different field
    it = empty_it()
    it['noise'] = (sigma, key + 1)
    assert not np.array_equal(run_stage(x[:1], it), got[:1])


def test_constant_channel_through_every_transform():
    x = np.full((2, 5, 1, 7), -3.5, np.float32)
    it = {'noise': None, 'blur': [0.8, 0.6], 'brightness': [1.1, 0.9], 'contrast': [0.8, 1.2], 'lowres': [0.6, 1.0],
          'gamma_inverted': [0.8, 1.3], 'gamma': [1.4, 0.75]}
    got = run_stage(x, it, 3)
    close(got, REF.chain(x, it, 3), 1e-4, x)


# ------------------------------------------------------------------------------------------------ the loader
def seg_before_removal(ds, dl, plan, j):
    """The stored target of sample j before RemoveLabel (the -1 the mask reads), from the feed's tested kernels."""
    keys, boxes, spatial, _, flips = plan
    _, seg, _ = dl._case(keys[j])
    out = torch.empty((1, *dl.final_patch_size), dtype=torch.float32, device=DEV)
    if spatial[j] is None:
        shift = [(n - f) // 2 for n, f in zip(dl.patch_size, dl.final_patch_size)]
        DLD.crop_pad_seg(seg, out, [b + s for b, s in zip(boxes[j], shift)], flips[j], -1)
    else:
        pseg = torch.empty((1, *dl.patch_size), dtype=torch.float32, device=DEV)
        DLD.crop_pad_seg(seg, pseg, boxes[j], 0, -1)
        DLD.spatial_transform_seg(pseg, out, DLD.spatial_affine(spatial[j], dl.patch_size), flips[j])
    return out.cpu().numpy()


def make_loaders(ds, n, f, rot, probs, mask_channels, batch=3, **kw):
    args = dict(oversample_foreground_percent=0.33, mirror_axes=(0, 1, 2), device=DEV, rotation_for_DA=rot, **kw)
    on = DLD.DeviceDataLoader3D(ds, batch, n, f, _Labels(), intensity_augmentation=True, mask_channels=mask_channels,
                                **probs, **args)
    off = DLD.DeviceDataLoader3D(ds, batch, n, f, _Labels(), **args)
    return on, off


@pytest.mark.parametrize("rotation", [True, False])
@pytest.mark.parametrize("probs", ["all_on", "reference"])
def test_loader_batches_against_the_oracle_chain(probs, rotation):
    f = (18, 21, 16)
    rot = {ax: (-np.pi / 6, np.pi / 6) for ax in 'xyz'} if rotation else None
    n = (26, 29, 24) if rotation else f
    ds = _DS([(30, 34, 28), (22, 40, 25)], 3, 7)
    scales = [[1, 1, 1], [0.5, 0.5, 0.5]]
    on, off = make_loaders(ds, n, f, rot, ALL_ON if probs == "all_on" else {}, [True, False, True],
                           deep_supervision_scales=scales, p_rot_per_sample=0.5, p_scale_per_sample=0.5)
    np.random.seed(4)
    touched = 0
    for _ in range(4 if probs == "all_on" else 12):
        plan = on.plan_batch()
        keys, boxes, spatial, intensity, flips = plan
        b1 = on.generate_train_batch(plan)
        b2 = on.generate_train_batch(plan)
        assert torch.equal(b1["data"], b2["data"]) and all(torch.equal(a, b) for a, b in zip(b1["target"], b2["target"]))
        base = off.generate_train_batch((keys, boxes, spatial, flips) if rotation else (keys, boxes, flips))
        data, base_d = b1["data"].cpu().numpy(), base["data"].cpu().numpy()
        t0 = b1["target"][0].cpu().numpy()
        for j in range(3):
            pre = seg_before_removal(ds, on, plan, j)
            ref = REF.mask(REF.chain(base_d[j], intensity[j], flips[j]), pre, [0, 2])
            close(data[j], ref, 1e-4, np.maximum(np.abs(base_d[j]), np.abs(ref)))
            rem = pre.copy()
            rem[rem == -1] = 0
            assert np.array_equal(t0[j], rem)
            touched += any(intensity[j][k] is not None for k in DLD.INTENSITY_KEYS)
        assert torch.equal(b1["target"][1], DLD.downsample_seg(b1["target"][0], scales[1]))
    assert touched > 0


def test_off_is_bit_identical_to_the_loader_without_the_arguments():
    f = (18, 21, 16)
    rot = {ax: (-np.pi / 6, np.pi / 6) for ax in 'xyz'}
    ds = _DS([(30, 34, 28)], 3, 9)
    for r, n in ((None, f), (rot, (26, 29, 24))):
        old = DLD.DeviceDataLoader3D(ds, 2, n, f, _Labels(), mirror_axes=(0, 1, 2), device=DEV, rotation_for_DA=r)
        new = DLD.DeviceDataLoader3D(ds, 2, n, f, _Labels(), mirror_axes=(0, 1, 2), device=DEV, rotation_for_DA=r,
                                     intensity_augmentation=False, mask_channels=None, **ALL_ON)
        for seed in range(3):
            np.random.seed(seed)
            a = old.generate_train_batch()
            np.random.seed(seed)
            b = new.generate_train_batch()
            assert torch.equal(a["data"], b["data"]) and torch.equal(a["target"], b["target"])


def test_full_size_all_on_sample():
    """4 x 205^3 -> 128^3, every transform on, one channel against the oracle chain."""
    f = (128, 128, 128)
    rot = {ax: (-np.pi / 6, np.pi / 6) for ax in 'xyz'}
    n = tuple(int(v) for v in DLD.get_patch_size(f, *rot.values(), (0.85, 1.25)))
    assert n == (205, 205, 205)
    ds = _DS([(140, 150, 130)], 4, 11, False)
    on, off = make_loaders(ds, n, f, rot, ALL_ON, None, batch=1, p_rot_per_sample=1.0, p_scale_per_sample=1.0)
    np.random.seed(2)
    plan = on.plan_batch()
    keys, boxes, spatial, intensity, flips = plan
    got = on.generate_train_batch(plan)["data"][0, :1].cpu().numpy()
    base = off.generate_train_batch((keys, boxes, spatial, flips))["data"][0, :1].cpu().numpy()
    it = {k: (v if v is None or k == 'noise' else v[:1]) for k, v in intensity[0].items()}
    ref = REF.chain(base, it, flips[0])
    close(got, ref, 1e-4, np.maximum(np.abs(base), np.abs(ref)))


def test_trainer_step_on_an_intensity_augmented_batch():
    from multimodal_mvd_seg_amd import trainer
    patch = (32, 32, 32)
    plans = trainer.make_plans(patch, [[1, 1, 1], [2, 2, 2], [2, 2, 2]], batch_size=2, base_features=16,
                               max_features=32)
    plans['configurations']['3d_fullres']['use_mask_for_norm'] = [True, False, False]
    dj = {"channel_names": {"0": "a", "1": "b", "2": "c"}, "labels": {"background": 0, "a": 1, "b": 2, "c": 3}}
    torch.manual_seed(0)
    tr = trainer.nnUNetTrainerMI355(plans, "3d_fullres", 0, dj, device=DEV)
    tr.initialize()
    tr.on_train_epoch_start()
    dl = tr.get_device_dataloader(_DS([(60, 64, 56)], 3, 8), intensity_augmentation=True)
    assert dl.intensity_augmentation and dl.mask_channels == [0]
    for k, v in ALL_ON.items():
        setattr(dl, k, v)
    np.random.seed(0)
    b = next(dl)
    assert tuple(b["data"].shape) == (2, 3, *patch) and torch.isfinite(b["data"]).all()
    loss = float(tr.train_step(b)["loss"])
    assert np.isfinite(loss)
    assert not tr.get_device_dataloader(_DS([(60, 64, 56)], 3, 8)).intensity_augmentation
