"""CPU tests of the device feed's intensity stage host logic: the draw sequence of draw_intensity in
batchgenerators' order, the plan forms, the Philox restatement against numpy, and the low-res geometry."""
import numpy as np
import pytest

import feed_intensity_ref as REF
from multimodal_mvd_seg_amd import dataloading as DLD

R30 = (-30. / 360 * 2. * np.pi, 30. / 360 * 2. * np.pi)
ROT = {'x': R30, 'y': R30, 'z': R30}
ALL_ON = dict(p_noise=1.0, p_blur=1.0, p_blur_per_channel=1.0, p_brightness=1.0, p_contrast=1.0, p_lowres=1.0,
              p_lowres_per_channel=1.0, p_gamma_inverted=1.0, p_gamma=1.0)
ALL_OFF = {k: 0.0 for k in ALL_ON}


class _ToyDataset:
    def __init__(self, shapes, C=3, seed=0):
        rng = np.random.default_rng(seed)
        self.cases = {}
        for i, shp in enumerate(shapes):
            data = rng.standard_normal((C, *shp)).astype(np.float32)
            seg = (rng.random((1, *shp)) > 0.97).astype(np.int16) * rng.integers(1, 3, (1, *shp)).astype(np.int16)
            self.cases[f"case{i}"] = (data, seg, {"class_locations": {c: np.argwhere(seg == c) for c in (1, 2)}})

    def keys(self):
        return self.cases.keys()

    def load_case(self, k):
        return self.cases[k]


class _Labels:
    all_labels = [1, 2]
    has_ignore_label = False


def _loader(rotation=True, **kw):
    ds = _ToyDataset([(20, 24, 28), (9, 30, 12)])
    args = dict(oversample_foreground_percent=0.33, mirror_axes=(0, 1, 2), device="cpu")
    if rotation:
        args['rotation_for_DA'] = ROT
    args.update(kw)
    patch = (18, 22, 22) if rotation else (12, 16, 16)
    return DLD.DeviceDataLoader3D(ds, 4, patch, (12, 16, 16), _Labels(), **args)


def _replay_intensity(B, C, p):
    """The restated draw sequence of DESIGN 14, written out call by call; returns (per-sample dicts, draws)."""
    n = 0

    def u(*a):
        nonlocal n
        n += 1
        return np.random.uniform(*a)

    def rnd():
        nonlocal n
        n += 1
        return np.random.random()

    out = [dict.fromkeys(DLD.INTENSITY_KEYS) for _ in range(B)]
    for it in out:                                                       # GaussianNoiseTransform
        if u() < p['p_noise']:
            sigma = u(0, 0.1)
            for _ in range(C):
                u()
            n += 1
            it['noise'] = (sigma, int(np.random.randint(0, 2 ** 63, dtype=np.int64)))
    for it in out:                                                       # GaussianBlurTransform
        if u() < p['p_blur']:
            it['blur'] = []
            for _ in range(C):
                it['blur'].append(u(0.5, 1.) if u() <= p['p_blur_per_channel'] else None)
    for it in out:                                                       # BrightnessMultiplicativeTransform
        if u() < p['p_brightness']:
            u(0.75, 1.25)
            it['brightness'] = [u(0.75, 1.25) for _ in range(C)]
    for it in out:                                                       # ContrastAugmentationTransform
        if u() < p['p_contrast']:
            it['contrast'] = []
            for _ in range(C):
                u()
                it['contrast'].append(u(0.75, 1) if rnd() < 0.5 else u(1, 1.25))
    for it in out:                                                       # SimulateLowResolutionTransform
        if u() < p['p_lowres']:
            it['lowres'] = [u(0.5, 1) if u() < p['p_lowres_per_channel'] else None for _ in range(C)]
    for key in ('gamma_inverted', 'gamma'):                              # the two GammaTransforms
        for it in out:
            if u() < p['p_' + key]:
                it[key] = [u(0.7, 1) if rnd() < 0.5 else u(1, 1.5) for _ in range(C)]
    return out, n


def _expected_draws(out, C):
    n = 0
    for it in out:
        n += 7  # one per-sample draw per transform
        n += (C + 2) if it['noise'] else 0
        n += (C + sum(s is not None for s in it['blur'])) if it['blur'] else 0
        n += (C + 1) if it['brightness'] else 0
        n += 3 * C if it['contrast'] else 0
        n += (C + sum(z is not None for z in it['lowres'])) if it['lowres'] else 0
        n += 2 * C * ((it['gamma_inverted'] is not None) + (it['gamma'] is not None))
    return n


@pytest.mark.parametrize("probs", ["all_on", "reference", "all_off", "half"])
@pytest.mark.parametrize("rotation", [True, False])
def test_plan_replays_the_restated_draw_sequence(probs, rotation):
    p = {"all_on": ALL_ON, "all_off": ALL_OFF, "half": {k: 0.5 for k in ALL_ON}}.get(probs)
    kw = dict(p) if p is not None else {}
    dl = _loader(rotation, intensity_augmentation=True, **kw)
    ref_p = {k: getattr(dl, k) for k in ALL_ON}
    for seed in range(25):
        np.random.seed(seed)
        plan = dl.plan_batch()
        assert len(plan) == 5
        keys, boxes, spatial, intensity, flips = plan
        tail = np.random.uniform()
        np.random.seed(seed)
        k2 = dl.get_indices()
        b2 = [dl.get_bbox(tuple(dl._data.load_case(k)[0].shape[1:]), dl.get_do_oversample(j),
                          dl._data.load_case(k)[2]["class_locations"])[0] for j, k in enumerate(k2)]
        sp = [dl.draw_spatial() if rotation else None for _ in k2]
        exp, n = _replay_intensity(len(k2), 3, ref_p)
        fl = [dl.draw_mirror() for _ in k2]
        assert list(keys) == list(k2) and boxes == b2 and spatial == sp and flips == fl
        assert intensity == exp
        assert n == _expected_draws(exp, 3)
        assert np.random.uniform() == tail  # same number of draws in total
        if not rotation:
            assert spatial == [None] * 4
        if probs == "all_on":
            assert all(all(it[k] is not None for k in DLD.INTENSITY_KEYS) for it in intensity)
            assert all(None not in it['blur'] and None not in it['lowres'] for it in intensity)
        if probs == "all_off":
            assert all(all(it[k] is None for k in DLD.INTENSITY_KEYS) for it in intensity)


def test_drawn_values_lie_in_the_reference_ranges():
    dl = _loader(intensity_augmentation=True, **ALL_ON)
    np.random.seed(3)
    for _ in range(30):
        for it in dl.plan_batch()[3]:
            assert 0 <= it['noise'][0] <= 0.1 and 0 <= it['noise'][1] < 2 ** 63
            assert all(0.5 <= s <= 1 for s in it['blur'])
            assert all(0.75 <= m <= 1.25 for m in it['brightness'] + it['contrast'])
            assert all(0.5 <= z <= 1 for z in it['lowres'])
            assert all(0.7 <= g <= 1.5 for g in it['gamma_inverted'] + it['gamma'])


def test_plans_reproducible_and_hit_rates_plausible():
    dl = _loader(intensity_augmentation=True)
    np.random.seed(11)
    p1 = [dl.plan_batch() for _ in range(300)]
    np.random.seed(11)
    p2 = [dl.plan_batch() for _ in range(300)]
    assert p1 == p2
    its = [it for p in p1 for it in p[3]]  # 1200 samples
    rate = {k: np.mean([it[k] is not None for it in its]) for k in DLD.INTENSITY_KEYS}
    for k, p in zip(DLD.INTENSITY_KEYS, (0.1, 0.2, 0.15, 0.15, 0.25, 0.1, 0.3)):
        assert abs(rate[k] - p) < 4 * np.sqrt(p * (1 - p) / len(its)) + 1e-9, (k, rate[k])
    sel = [s is not None for it in its if it['blur'] for s in it['blur']]
    assert 0.4 < np.mean(sel) < 0.6
    keys = [it['noise'][1] for it in its if it['noise']]
    assert len(set(keys)) == len(keys)


def test_off_keeps_the_old_plans_and_draws():
    for rotation, size in ((False, 3), (True, 4)):
        dl_old = _loader(rotation)
        dl_off = _loader(rotation, intensity_augmentation=False, mask_channels=None, **ALL_ON)
        for seed in range(10):
            np.random.seed(seed)
            a = dl_old.plan_batch()
            ta = np.random.uniform()
            np.random.seed(seed)
            b = dl_off.plan_batch()
            assert len(a) == size and a == b and np.random.uniform() == ta


def test_philox_restatement_equals_numpy():
    for key in (0, 1, 123456789012345, 2 ** 63 - 1, 2 ** 64 + 7, 2 ** 127 + 2 ** 70 + 5):
        n = 1037
        assert np.array_equal(REF.philox_raw(key, n), np.random.Philox(key=key).random_raw(n))


def test_box_muller_normals_are_standard():
    z = REF.normals(987654321, 1 << 20)
    assert np.isfinite(z).all() and abs(z.mean()) < 5e-3 and abs(z.std() - 1) < 5e-3


def test_lowres_geometry():
    assert DLD.lowres_target_shape((128, 128, 128), 0.5) == [64, 64, 64]
    assert DLD.lowres_target_shape((17, 1, 29), 0.63) == [11, 1, 18]
    assert DLD.lowres_target_shape((1, 2, 3), 0.5) == [1, 1, 2]  # round-half-even, at least 1
    a = DLD.lowres_affine((17, 23, 29), (11, 14, 18))
    o = np.array([0, 5, 16])
    n, t = np.array([17, 23, 29]), np.array([11, 14, 18])
    p = np.array(a[:9]).reshape(3, 3) @ (o - (n - 1) / 2.) + np.array(a[9:])
    assert np.allclose(p, (o + 0.5) * t / n - 0.5 + 12, atol=1e-12)


def test_mask_channels_and_limits():
    dl = _loader(intensity_augmentation=True, mask_channels=[True, False, True])
    assert dl.mask_channels == [0, 2]
    assert _loader(mask_channels=[False, False, False]).mask_channels is None
    with pytest.raises(ValueError):
        DLD._chmask(17, None)
    with pytest.raises(ValueError):
        DLD._chmask(3, [3])
    assert DLD._chmask(3, None) == 7 and DLD._chmask(4, [1, 3]) == 10
    np.random.seed(0)
    with pytest.raises(RuntimeError):
        dl.generate_train_batch(dl.plan_batch())  # no CPU path
