"""CPU tests of the DA5 recipe of the device feed: the oracle's median against a brute-force window sort, the
per-axis scale of spatial_affine, draw_da5's draws, the composition of Rot90 and Transpose into one signed permutation,
the trainers and the refusals.  Nothing here touches a GPU."""
import itertools

import numpy as np
import pytest
import torch

import feed_da5_ref as REF
from multimodal_mvd_seg_amd import dataloading as DLD
from multimodal_mvd_seg_amd import trainer

DJ = {"channel_names": {"0": "a", "1": "b"}, "labels": {"background": 0, "a": 1, "b": 2, "c": 3}}
STRIDES = [[1, 1, 1], [2, 2, 2], [2, 2, 2]]
ROT = {ax: (-np.pi / 6, np.pi / 6) for ax in 'xyz'}
ALL = {k: 1.0 for k in DLD.DA5_PROBABILITIES}
NONE = {k: 0.0 for k in DLD.DA5_PROBABILITIES}


class _DS:
    def __init__(self, shapes, C=2, seed=0):
        rng = np.random.default_rng(seed)
        self.cases = {}
        for i, shp in enumerate(shapes):
            data = rng.standard_normal((C, *shp)).astype(np.float32)
            seg = rng.integers(0, 4, (1, *shp)).astype(np.int16)
            self.cases[f"c{i}"] = (data, seg, {"class_locations": {c: np.argwhere(seg == c) for c in (1, 2, 3)}})

    def keys(self):
        return self.cases.keys()

    def load_case(self, k):
        return self.cases[k]


class _Labels:
    all_labels = [1, 2, 3]
    has_ignore_label = False


def loader(final=(24, 24, 24), patch=None, batch=2, **kw):
    patch = final if patch is None else patch
    kw.setdefault('rotation_for_DA', ROT if patch != final else None)
    return DLD.DeviceDataLoader3D(_DS([(40, 40, 40), (36, 44, 40)]), batch, patch, final, _Labels(), device="cpu",
                                  mirror_axes=(0, 1, 2), **kw)


@pytest.mark.parametrize("shape", [(5, 7, 9), (1, 6, 13)])
@pytest.mark.parametrize("s", range(2, 8))
def test_oracle_median_is_the_window_sort(shape, s):
    x = np.random.default_rng(s).standard_normal(shape).astype(np.float32)
    assert np.array_equal(REF.median(x, s), REF.median_brute(x, s))


def test_spatial_affine_per_axis_scale():
    rng = np.random.default_rng(0)
    patch = (30, 26, 34)
    ax, ay, az = rng.uniform(-0.5, 0.5, 3)
    sc = (0.8, 1.3, 1.1)
    a = np.asarray(DLD.spatial_affine((ax, ay, az, sc), patch))
    A, off = a[:9].reshape(3, 3), a[9:]
    # augment_spatial's chain on coordinate row vectors: rotate, scale each coordinate, + centre
    c = rng.standard_normal((50, 3))
    want = c.dot(DLD.rotation_matrix_3d(ax, ay, az)) * np.asarray(sc)[None] + (np.asarray(patch) / 2. - 0.5)[None]
    assert np.allclose(c.dot(A.T) + off[None], want, rtol=0, atol=1e-12)
    # a scalar gives today's 12 doubles bit for bit
    today = [float(v) for v in (1.17 * DLD.rotation_matrix_3d(ax, ay, az).T).reshape(-1)] + \
        [float(v) for v in np.asarray(patch, dtype=np.float64) / 2. - 0.5]
    assert DLD.spatial_affine((ax, ay, az, 1.17), patch) == today
    assert np.allclose(DLD.spatial_affine((ax, ay, az, (1.17,) * 3), patch), today, rtol=0, atol=1e-15)
    with pytest.raises(ValueError):
        DLD.spatial_affine((ax, ay, az, (1., 2.)), patch)


class _Count:
    """Counts the calls of the np.random functions draw_da5 uses."""
    NAMES = ('uniform', 'random', 'choice', 'randint', 'normal', 'shuffle')

    def __init__(self, monkeypatch):
        self.n = dict.fromkeys(self.NAMES, 0)
        for name in self.NAMES:
            monkeypatch.setattr(np.random, name, self._wrap(name, getattr(np.random, name)))

    def _wrap(self, name, fn):
        def f(*a, **k):
            self.n[name] += 1
            return fn(*a, **k)
        return f


def test_draw_da5_nothing_selected(monkeypatch):
    dl = loader(da5=True, da5_probabilities=NONE)
    assert dl.da5_valid_axes() == (0, 1, 2)
    np.random.seed(1)
    cnt = _Count(monkeypatch)
    d = dl.draw_da5(3, 2)
    # two OneOf choices per batch; per sample 13 p_per_sample uniforms (11 + rot90 + transpose) and 3 mirror uniforms
    assert cnt.n == {'uniform': 3 * (13 + 3), 'random': 0, 'choice': 2, 'randint': 0, 'normal': 0, 'shuffle': 0}
    for key in ('rot90', 'transpose', 'signed', 'median', 'blur', 'noise', 'brightness', 'contrast', 'lowres', 'gamma1',
                'gamma2', 'blank', 'gradient', 'local_gamma', 'sharpen'):
        assert d[key] == [None] * 3, key
    assert len(d['mirror']) == 3 and d['oneof_blur'] in (0, 1) and d['oneof_contrast'] in (0, 1)
    # no extent occurs twice: Rot90 and Transpose are not part of the recipe and draw nothing
    dl2 = loader(final=(20, 24, 28), da5=True, da5_probabilities=NONE)
    assert dl2.da5_valid_axes() == ()
    cnt.n = dict.fromkeys(cnt.NAMES, 0)
    dl2.draw_da5(3, 2)
    assert cnt.n['uniform'] == 3 * (11 + 3) and cnt.n['choice'] == 2


def test_draw_da5_one_of_is_drawn_once_per_batch(monkeypatch):
    dl = loader(da5=True, da5_probabilities=ALL)
    seen = set()
    for seed in range(8):
        np.random.seed(seed)
        cnt = _Count(monkeypatch)
        d = dl.draw_da5(4, 2)
        monkeypatch.undo()
        # choice: 2 OneOf draws, and per sample rot90's k and axes
        assert cnt.n['choice'] == 2 + 2 * 4
        chosen, other = ('median', 'blur') if d['oneof_blur'] == 0 else ('blur', 'median')
        assert all(v is not None for v in d[chosen]) and d[other] == [None] * 4
        seen.add(d['oneof_blur'])
    assert seen == {0, 1}


def test_draw_da5_everything_selected_is_within_range():
    dl = loader(da5=True, da5_probabilities=ALL)
    p = dl.final_patch_size
    for seed in range(6):
        np.random.seed(seed)
        d = dl.draw_da5(2, 3)
        for j in range(2):
            k, axes = d['rot90'][j]
            assert k in (0, 1, 2, 3) and len(axes) == 2 and axes[0] < axes[1]
            assert sorted(d['transpose'][j]) == [0, 1, 2]
            if d['oneof_blur'] == 0:
                assert all(2 <= s <= 7 for s in d['median'][j])
            else:
                assert all(0.3 <= s <= 1.5 for s in d['blur'][j])
            assert 0 <= d['noise'][j][0] <= 0.1
            assert len(d['brightness'][j]) == 3 and all(v is not None for v in d['brightness'][j])
            assert all(0.5 <= f <= 2 for f in d['contrast'][j])
            assert all(0.25 <= z <= 1 for z in d['lowres'][j])
            for key in ('gamma1', 'gamma2'):   # both gammas are the inverted one: apply_da5 runs them as such
                assert all(0.7 <= g <= 1.5 for g in d[key][j])
            assert 0 <= d['mirror'][j] < 8
            for rects in d['blank'][j]:
                assert 1 <= len(rects) <= 4
                for lb, size in rects:
                    for l, s, n in zip(lb, size, p):
                        assert max(1, n // 10) <= s <= n // 3 and 0 <= l and l + s <= n
            for key, lo_hi in (('gradient', ((-5, -1), (1, 5))), ('local_gamma', ((0.01, 0.8), (1.5, 4)))):
                for scale, loc, amount in d[key][j]:
                    assert all(n // 6 <= s <= n for s, n in zip(scale, p))
                    assert all(-0.5 * n <= l <= 1.5 * n for l, n in zip(loc, p))
                    assert any(lo <= amount <= hi for lo, hi in lo_hi)
            assert all(0.1 <= s <= 1 for s in d['sharpen'][j])
    assert 'gamma' not in d and 'gamma_inverted' not in d


def test_rot90_and_transpose_compose_into_one_signed_permutation():
    x = np.arange(64).reshape(4, 4, 4)
    n = 0
    for k in range(4):
        for axes in ((0, 1), (0, 2), (1, 2)):
            for t in itertools.permutations(range(3)):
                perm, mask = DLD.compose_signed_permutation((k, axes), t)
                got = np.transpose(x, perm)
                for ax in range(3):
                    if mask & (1 << ax):
                        got = np.flip(got, ax)
                assert np.array_equal(got, np.transpose(np.rot90(x, k, axes), t)), (k, axes, t)
                n += 1
    assert n == 4 * 3 * 6
    assert DLD.compose_signed_permutation() == ((0, 1, 2), 0)
    assert DLD.compose_signed_permutation(None, None, 5) == ((0, 1, 2), 5)


def make(name, patch=(32, 32, 32), dataset_json=DJ, **kw):
    plans = trainer.make_plans(patch, STRIDES, batch_size=2, base_features=8, max_features=32, **kw)
    tr = getattr(trainer, name)(plans, kw.get("configuration", "3d_fullres"), 0, dataset_json,
                                device=torch.device("cuda"))
    tr._set_batch_size_and_oversample()   # what initialize() does before the loaders are built
    return tr


def test_da5_trainer_initial_patch_size():
    for patch in ((32, 32, 32), (40, 56, 48)):
        tr = make("nnUNetTrainerDA5MI355", patch)
        rot, dummy, initial, mirror = tr.configure_rotation_dummyDA_mirroring_and_inital_patch_size()
        r = (-30. / 360 * 2. * np.pi, 30. / 360 * 2. * np.pi)
        assert list(initial) == list(DLD.get_patch_size(patch, r, r, r, (0.7, 1.43)))
        assert not dummy and mirror == (0, 1, 2) and tr.inference_allowed_mirroring_axes == (0, 1, 2)
        base = make("nnUNetTrainerMI355", patch).configure_rotation_dummyDA_mirroring_and_inital_patch_size()[2]
        assert all(a >= b for a, b in zip(initial, base)) and list(initial) != list(base)
    assert make("nnUNetTrainerDA5_10epochsMI355").num_epochs == 10
    assert issubclass(trainer.nnUNetTrainerDA5_10epochsMI355, trainer.nnUNetTrainerDA5MI355)
    import multimodal_mvd_seg_amd as pkg
    for name in ("nnUNetTrainerDA5MI355", "nnUNetTrainerDA5_10epochsMI355", "nnUNetTrainerNoMirroringMI355",
                 "nnUNetTrainerNoDAMI355"):
        assert getattr(pkg, name) is getattr(trainer, name)


def test_refusals_name_da5():
    with pytest.raises(NotImplementedError, match="DA5"):       # a 2-D plan
        DLD.DeviceDataLoader3D(_DS([(40, 40, 40)]), 2, (24, 24), (24, 24), _Labels(), device="cpu", da5=True)
    with pytest.raises(NotImplementedError, match="DA5"):       # the in-plane form
        DLD.DeviceDataLoader3D(_DS([(40, 40, 40)]), 2, (24, 30, 30), (24, 24, 24), _Labels(), device="cpu", da5=True,
                               do_dummy_2d_data_aug=True, rotation_for_DA=ROT)
    with pytest.raises(NotImplementedError, match="DA5"):       # cascade mode
        DLD.DeviceDataLoader3D(_DS([(40, 40, 40)]), 2, (24, 24, 24), (24, 24, 24), _Labels(), device="cpu", da5=True,
                               cascade_labels=[1, 2, 3])
    with pytest.raises(ValueError, match="DA5"):
        loader(da5=True, da5_probabilities={'nope': 1.0})
    ds = _DS([(40, 40, 40)])
    with pytest.raises(NotImplementedError, match="DA5"):       # anisotropic plan -> dummy 2-D mode
        make("nnUNetTrainerDA5MI355", (16, 64, 64)).get_device_dataloader(ds, device="cpu")
    plans2d = trainer.make_plans((32, 32), [[1, 1], [2, 2], [2, 2]], batch_size=2, base_features=8, max_features=32,
                                 configuration="2d")
    tr2d = trainer.nnUNetTrainerDA5MI355(plans2d, "2d", 0, DJ, device=torch.device("cuda"))
    tr2d._set_batch_size_and_oversample()
    with pytest.raises(NotImplementedError, match="DA5"):
        tr2d.get_device_dataloader(ds, device="cpu")
    dl = make("nnUNetTrainerDA5MI355").get_device_dataloader(ds, device="cpu")
    assert dl.da5 and dl.intensity_augmentation and dl.scale_range == (0.7, 1.43)
    assert (dl.p_rot_per_sample, dl.p_rot_per_axis, dl.p_scale_per_sample) == (0.4, 0.5, 0.2)
    assert dl.da5_p == DLD.DA5_PROBABILITIES


def test_no_mirroring_and_no_da_trainers():
    ds = _DS([(40, 40, 40)])
    nm = make("nnUNetTrainerNoMirroringMI355")
    rot, dummy, initial, mirror = nm.configure_rotation_dummyDA_mirroring_and_inital_patch_size()
    base = make("nnUNetTrainerMI355").configure_rotation_dummyDA_mirroring_and_inital_patch_size()
    assert mirror is None and nm.inference_allowed_mirroring_axes is None
    assert rot == base[0] and list(initial) == list(base[2])
    assert nm.get_device_dataloader(ds, device="cpu").mirror_axes == ()
    nd = make("nnUNetTrainerNoDAMI355")
    dl = nd.get_device_dataloader(ds, device="cpu")
    assert nd.inference_allowed_mirroring_axes is None
    assert dl.patch_size == dl.final_patch_size == (32, 32, 32)
    assert dl.rotation_for_DA is None and not dl.intensity_augmentation and dl.mirror_axes == () and not dl.da5


def test_plain_plan_is_unchanged_with_da5_off():
    """plan_batch of the default recipe against its draw sequence written out here: keys, boxes, per sample the
    SpatialTransform draws (one scalar scale), draw_intensity, the mirrors."""
    dl = loader(final=(24, 24, 24), patch=(34, 34, 34), batch=3, intensity_augmentation=True, da5=False,
                p_rot_per_sample=0.6, p_scale_per_sample=0.6, oversample_foreground_percent=0.33)
    for seed in range(5):
        np.random.seed(seed)
        plan = dl.plan_batch()
        np.random.seed(seed)
        keys = np.random.choice(dl.indices, 3, replace=True, p=None)
        boxes = []
        for j, k in enumerate(keys):
            force = not j < round(3 * (1 - 0.33))
            data, _, props = dl._case(k)
            boxes.append([int(v) for v in dl.get_bbox(tuple(data.shape[1:]), force, props['class_locations'])[0]])
        spatial = []
        for _ in keys:
            rot, sc, mod = [0., 0., 0.], 1., False
            if np.random.uniform() < 0.6:
                for i, ax in enumerate('xyz'):
                    if np.random.uniform() <= 1.0:
                        rot[i] = np.random.uniform(*ROT[ax])
                mod = True
            if np.random.uniform() < 0.6:
                if np.random.random() < 0.5:
                    sc = np.random.uniform(0.7, 1)
                else:
                    sc = np.random.uniform(1, 1.4)
                mod = True
            spatial.append((float(rot[0]), float(rot[1]), float(rot[2]), float(sc)) if mod else None)
        intensity = dl.draw_intensity(3, 2)
        flips = [dl.draw_mirror() for _ in keys]
        assert plan == (list(keys), boxes, spatial, intensity, flips)
        assert any(s is not None and s[3] != 1.0 for s in spatial) or seed > 0
