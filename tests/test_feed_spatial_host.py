"""CPU tests of the device feed's SpatialTransform host logic: the initial patch size, the rotation matrix,
the per-sample draws in batchgenerators' augment_spatial order, the loader's construction rules and the trainer's
configure_rotation_dummyDA_mirroring_and_inital_patch_size."""
import numpy as np
import pytest

from multimodal_mvd_seg_amd import dataloading as DLD
from multimodal_mvd_seg_amd import trainer

R30 = (-30. / 360 * 2. * np.pi, 30. / 360 * 2. * np.pi)
ROT = {'x': R30, 'y': R30, 'z': R30}


class _ToyDataset:
    def __init__(self, shapes, seed=0):
        rng = np.random.default_rng(seed)
        self.cases = {}
        for i, shp in enumerate(shapes):
            data = rng.standard_normal((2, *shp)).astype(np.float32)
            seg = (rng.random((1, *shp)) > 0.97).astype(np.int16) * rng.integers(1, 3, (1, *shp)).astype(np.int16)
            self.cases[f"case{i}"] = (data, seg, {"class_locations": {c: np.argwhere(seg == c) for c in (1, 2)}})

    def keys(self):
        return self.cases.keys()

    def load_case(self, k):
        return self.cases[k]


class _Labels:
    all_labels = [1, 2]
    has_ignore_label = False


def _loader(**kw):
    ds = _ToyDataset([(20, 24, 28), (9, 30, 12)])
    args = dict(oversample_foreground_percent=0.33, mirror_axes=(0, 1, 2), device="cpu", rotation_for_DA=ROT)
    args.update(kw)
    return DLD.DeviceDataLoader3D(ds, 4, (18, 22, 22), (12, 16, 16), _Labels(), **args)


def test_get_patch_size_matches_the_reference_values():
    assert DLD.get_patch_size((128,) * 3, R30, R30, R30, (0.85, 1.25)).tolist() == [205, 205, 205]
    assert DLD.get_patch_size((64,) * 3, R30, R30, R30, (0.85, 1.25)).tolist() == [102, 102, 102]
    # angles are clipped to 90 degrees; no rotation and no shrink leaves the patch as it is
    assert DLD.get_patch_size((32, 40, 48), 0., 0., 0., (1, 1.2)).tolist() == [32, 40, 48]
    assert (DLD.get_patch_size((64,) * 3, 4.0, 0., 0., (1, 1)) == DLD.get_patch_size((64,) * 3, np.pi / 2, 0., 0.,
                                                                                      (1, 1))).all()


def test_rotation_matrix_is_rx_ry_rz():
    ax, ay, az = 0.3, -1.1, 2.5
    c, s = np.cos, np.sin
    rx = np.array([[1, 0, 0], [0, c(ax), -s(ax)], [0, s(ax), c(ax)]])
    ry = np.array([[c(ay), 0, s(ay)], [0, 1, 0], [-s(ay), 0, c(ay)]])
    rz = np.array([[c(az), -s(az), 0], [s(az), c(az), 0], [0, 0, 1]])
    assert np.allclose(DLD.rotation_matrix_3d(ax, ay, az), rx @ ry @ rz, rtol=0, atol=1e-15)
    assert np.allclose(DLD.rotation_matrix_3d(0, 0, 0), np.eye(3))


def test_affine_is_scaled_transposed_rotation_about_the_patch_centre():
    sp = (0.2, -0.4, 0.7, 1.3)
    a = np.array(DLD.spatial_affine(sp, (205, 204, 99)))
    A, off = a[:9].reshape(3, 3), a[9:]
    assert np.allclose(A, 1.3 * DLD.rotation_matrix_3d(0.2, -0.4, 0.7).T) and np.allclose(off, [102, 101.5, 49])
    # the batchgenerators coordinate pipeline on a few points: zero-centred mesh, c . R (row vector), * sc, + ctr
    f = np.array([128, 127, 64])
    o = np.array([[0, 0, 0], [127, 126, 63], [5, 77, 12]], dtype=float)
    c = (o - (f - 1) / 2.) @ DLD.rotation_matrix_3d(0.2, -0.4, 0.7) * 1.3 + (np.array([205, 204, 99]) / 2. - 0.5)
    assert np.allclose((A @ (o - (f - 1) / 2.).T).T + off, c, atol=1e-12)


def _replay_spatial(p_rot, p_scale, rot, scale, p_axis=1.0):
    """augment_spatial's draws for one sample (restated), returning (spatial or None, number of draws)."""
    n, angles, sc, mod = 0, [0., 0., 0.], 1., False
    u = np.random.uniform(); n += 1
    if u < p_rot:
        for i, ax in enumerate('xyz'):
            u = np.random.uniform(); n += 1
            if u <= p_axis:
                angles[i] = np.random.uniform(*rot[ax]); n += 1
        mod = True
    u = np.random.uniform(); n += 1
    if u < p_scale:
        r = np.random.random(); n += 1
        if r < 0.5 and scale[0] < 1:
            sc = np.random.uniform(scale[0], 1)
        else:
            sc = np.random.uniform(max(scale[0], 1), scale[1])
        n += 1
        mod = True
    return ((*angles, sc) if mod else None), n


@pytest.mark.parametrize("p_rot,p_scale", [(0.2, 0.2), (1.0, 0.0), (0.0, 1.0), (1.0, 1.0), (0.0, 0.0), (0.5, 0.5)])
def test_spatial_draws_replay_the_augment_spatial_sequence(p_rot, p_scale):
    dl = _loader(p_rot_per_sample=p_rot, p_scale_per_sample=p_scale)
    counts = set()
    for seed in range(40):
        np.random.seed(seed)
        got = dl.plan_batch()
        assert len(got) == 4
        keys, boxes, spatial, flips = got
        tail = np.random.uniform()
        # replay: keys and boxes through the loader's own (already pinned) methods, then the restated sequence
        np.random.seed(seed)
        k2 = dl.get_indices()
        for j, k in enumerate(k2):
            dl.get_bbox(tuple(dl._data.load_case(k)[0].shape[1:]), dl.get_do_oversample(j),
                        dl._data.load_case(k)[2]["class_locations"])
        exp = []
        for _ in k2:
            sp, n = _replay_spatial(p_rot, p_scale, ROT, (0.7, 1.4))
            exp.append(sp)
            counts.add((sp is not None and sp[:3] != (0., 0., 0.), sp is not None and sp[3] != 1., n))
        fl = [dl.draw_mirror() for _ in k2]
        assert list(keys) == list(k2) and spatial == exp and flips == fl
        assert np.random.uniform() == tail  # same number of draws
    # draw count per sample: 2 when neither branch fires, +6 for a rotation, +2 for a scaling
    for rot, scl, n in counts:
        assert n == 2 + 6 * rot + 2 * scl
    if p_rot == 1.0 and p_scale == 1.0:
        assert counts == {(True, True, 10)}
    if p_rot == 0.0 and p_scale == 0.0:
        assert counts == {(False, False, 2)}


def test_spatial_draws_consume_exactly_the_restated_number_of_values():
    dl = _loader(p_rot_per_sample=0.5, p_scale_per_sample=0.5)
    for seed in range(30):
        np.random.seed(seed)
        sp = dl.draw_spatial()
        tail = np.random.uniform()
        np.random.seed(seed)
        ref, _ = _replay_spatial(0.5, 0.5, ROT, (0.7, 1.4))
        assert sp == ref and np.random.uniform() == tail
        if sp is not None:
            assert all(R30[0] <= a <= R30[1] for a in sp[:3]) and 0.7 <= sp[3] <= 1.4


def test_plans_reproducible_and_mostly_unmodified_with_reference_probabilities():
    dl = _loader()
    np.random.seed(5)
    p1 = [dl.plan_batch() for _ in range(50)]
    np.random.seed(5)
    p2 = [dl.plan_batch() for _ in range(50)]
    assert p1 == p2
    frac = np.mean([s is None for p in p1 for s in p[2]])
    assert 0.5 < frac < 0.8  # 0.8 * 0.8 = 0.64 expected


def test_construction_rules():
    dl = _loader()
    assert dl.patch_size == (18, 22, 22) and dl.final_patch_size == (12, 16, 16)
    assert dl.data_shape == (4, 2, 12, 16, 16) and dl.seg_shape == (4, 1, 12, 16, 16)
    ds = _ToyDataset([(20, 24, 28)])
    with pytest.raises(NotImplementedError):  # without the transform, the sizes must still agree
        DLD.DeviceDataLoader3D(ds, 2, (18, 22, 22), (12, 16, 16), _Labels(), device="cpu")
    with pytest.raises(NotImplementedError, match="2-D"):
        _loader(do_dummy_2d_data_aug=True)
    # without rotation_for_DA the plan keeps its 3-tuple form
    dl0 = DLD.DeviceDataLoader3D(ds, 2, (12, 16, 16), (12, 16, 16), _Labels(), mirror_axes=(0, 1, 2), device="cpu")
    np.random.seed(1)
    assert len(dl0.plan_batch()) == 3
    with pytest.raises(RuntimeError):
        dl.generate_train_batch(dl.plan_batch())  # no CPU path


def _stub_trainer(patch):
    t = trainer.nnUNetTrainerMI355.__new__(trainer.nnUNetTrainerMI355)
    t.configuration_manager = trainer.PlansManager(trainer.make_plans(
        patch, [[1, 1, 1], [2, 2, 2]])).get_configuration("3d_fullres")
    return t


def test_trainer_configures_rotation_and_initial_patch():
    rot, dummy, initial, mirror = _stub_trainer((128, 128, 128)).configure_rotation_dummyDA_mirroring_and_inital_patch_size()
    assert rot == {'x': R30, 'y': R30, 'z': R30} and dummy is False
    assert list(initial) == [205, 205, 205] and mirror == (0, 1, 2)
    rot, dummy, initial, mirror = _stub_trainer((32, 160, 160)).configure_rotation_dummyDA_mirroring_and_inital_patch_size()
    assert dummy is True and rot['x'] == (-np.pi, np.pi) and rot['y'] == (0, 0) and rot['z'] == (0, 0)
    assert initial[0] == 32 and mirror == (0, 1, 2)
