"""CPU tests of the cascade stage's host logic: the numpy / scipy restatement (tests/cascade_ref.py) against
the reference's own class bodies (tests/golden/cascade_transforms.npz), the ball and its offset table, the integer removal
threshold, the draws, the input-channel count, the refusals, and that a loader without the cascade mode plans what it
planned before."""
import json
import os

import numpy as np
import pytest
from scipy import ndimage as ndi

import cascade_ref as REF
from conftest import GOLDEN, load_npz
from multimodal_mvd_seg_amd import dataloading as DLD
from multimodal_mvd_seg_amd import trainer as TR

R30 = (-30. / 360 * 2. * np.pi, 30. / 360 * 2. * np.pi)
ROT = {'x': R30, 'y': R30, 'z': R30}


# ------------------------------------------------------------------------------------------------ golden fixture
def test_binary_operator_restatement_reproduces_the_reference_classes():
    """Draws included: the restatement is seeded like the reference and must give its outputs and channel orders."""
    g = load_npz("cascade_transforms.npz")
    fired = 0
    for seed in g["bin_seeds"]:
        np.random.seed(int(seed))
        idx = [int(i) for i in g["channel_idx"]]
        data = g[f"bin{seed}_in"].copy()
        orders = REF.binary_operator_transform(data, idx)
        assert np.array_equal(data, g[f"bin{seed}_out1"]), seed
        orders += REF.binary_operator_transform(data, idx)   # the same list again: the order persists
        assert np.array_equal(data, g[f"bin{seed}_out2"]), seed
        assert np.array_equal(np.asarray(orders, dtype=np.int64).reshape(-1, len(idx)), g[f"bin{seed}_orders"]), seed
        fired += len(orders)
        assert np.array_equal(data[:, 0], g[f"bin{seed}_in"][:, 0])   # the modality channel is not touched
    assert fired >= 8


def test_removal_restatement_reproduces_the_reference_classes():
    """The pick is forced to the ordinal the reference's np.random.choice took; everything else is the restatement."""
    g = load_npz("cascade_transforms.npz")
    for seed in g["rem_seeds"]:
        data = g[f"rem{seed}_in"].copy()
        events = g[f"rem{seed}_events"]
        assert len(events) > 0
        for b, c, ordinal, n_valid in events:
            got = REF.remove_component(data[b, c], ordinal=int(ordinal))
            assert got == (ordinal, n_valid)
            # floor(u n_valid) reaches that ordinal from the middle of its interval
            assert min(n_valid - 1, int((ordinal + 0.5) / n_valid * n_valid)) == ordinal
        assert np.array_equal(data, g[f"rem{seed}_out"]), seed


# ------------------------------------------------------------------------------------------------ ball, offsets
@pytest.mark.parametrize("radius,side,count", [(1.0, 3, 7), (1.49, 3, 7), (1.5, 4, 8), (2.3, 5, 33), (3.7, 8, 160),
                                               (7.99, 16, 1736)])
def test_ball_side_count_symmetry_and_rows(radius, side, count):
    b = REF.ball(radius)
    assert b.shape == (side,) * 3 and int(b.sum()) == count
    assert np.array_equal(b, b[::-1, ::-1, ::-1])
    rows = DLD.ball_rows(radius)
    assert rows == REF.element_rows(radius)
    assert sum(hi - lo + 1 for _, _, lo, hi in rows) == count and len(rows) <= 256
    assert all(-8 <= v <= 8 for r in rows for v in r)
    # the table, read as the kernel reads it, is scipy's dilation and erosion
    rng = np.random.default_rng(side)
    m = rng.random((9, 11, 21)) < 0.3
    assert np.array_equal(REF.morph_from_rows(m, rows, False), REF.binary_dilation(m, b))
    assert np.array_equal(REF.morph_from_rows(~m, rows, True), REF.binary_erosion(~m, b))


def test_ball_rows_equal_the_restated_ball_at_random_radii():
    """Grid points lie exactly on the sphere for many radii (n = 15: (2, 3, 6) / 7 of r), so the table must add the squares
    in the order the restated ball() does; the trainer's radii are uniform(1, 8)."""
    rng = np.random.RandomState(0)
    sides = set()
    for radius in list(rng.uniform(1, 8, 300)) + [7.154414195618729, 3.5, 7.0]:
        assert DLD.ball_rows(radius) == REF.element_rows(radius), radius
        sides.add(int(2 * radius + 1))
    assert sides == set(range(3, 17))


def test_even_sided_element_is_centred_at_half_its_side_with_mirrored_offsets():
    b = REF.ball(1.5)
    assert sorted(map(tuple, np.argwhere(b))) == sorted((a, c, d) for a in (1, 2) for c in (1, 2) for d in (1, 2))
    m = np.zeros((7, 7, 7), dtype=bool)
    m[3, 3, 3] = True
    assert sorted(set(np.argwhere(REF.binary_dilation(m, b))[:, 0] - 3)) == [-1, 0]
    assert sorted(set(np.argwhere(~REF.binary_erosion(~m, b))[:, 0] - 3)) == [0, 1]
    full = np.ones((5, 5, 5), dtype=bool)
    assert REF.binary_erosion(full, REF.ball(3.7)).all()     # border_value=True
    with pytest.raises(ValueError):
        DLD.ball_rows(8.0)


def test_label_order_is_the_order_of_the_smallest_linear_index():
    rng = np.random.default_rng(4)
    m = rng.random((8, 9, 10)) < 0.12
    lab, sizes = REF.label_with_component_sizes(m)
    first = [np.flatnonzero(lab.ravel() == i)[0] for i in sizes]
    assert first == sorted(first) and len(first) > 5
    assert sum(sizes.values()) == m.sum()
    assert np.array_equal(lab, ndi.label(m, structure=np.ones((3, 3, 3)))[0])


@pytest.mark.parametrize("n", [8000, 8001, 20 * 21 * 22, 128 ** 3, 7])
def test_integer_removal_threshold_agrees_with_the_fp64_expression(n):
    t = DLD.cascade_removal_threshold(n)
    assert t == REF.removal_threshold(n)
    x = np.uint64(n) * 0.15
    for size in (t - 2, t - 1, t, t + 1):
        if size >= 0:
            assert (size < t) == bool(size < x), (n, size)
    if n == 8000:
        assert 8000 * 0.15 == 1200.0 and t == 1200      # a 1200-voxel component is not valid, an 1199-voxel one is
    if n == 8001:
        assert x != int(x) and t == 1201


# ------------------------------------------------------------------------------------------------ trainer surface
CH = {"channel_names": {"0": "a", "1": "b"}}


def _pm(**kw):
    plans = TR.make_plans((16, 16, 16), [(1, 1, 1), (2, 2, 2), (2, 2, 2)], base_features=4, max_features=16,
                          configuration='3d_lowres', spacing=(2., 2., 2.), cascade_configuration='3d_cascade_fullres',
                          cascade_spacing=(1., 1., 1.), **kw)
    return plans, TR.PlansManager(plans)


def test_two_stage_plan_and_input_channels():
    plans, pm = _pm()
    low, full = pm.get_configuration('3d_lowres'), pm.get_configuration('3d_cascade_fullres')
    assert low.next_stage_names == ['3d_cascade_fullres'] and getattr(low, 'previous_stage_name', None) is None
    assert full.previous_stage_name == '3d_lowres' and full.next_stage_names is None
    assert full.patch_size == low.patch_size and full.spacing == [1., 1., 1.] and low.spacing == [2., 2., 2.]
    plain = dict(CH, labels={"background": 0, "a": 1, "b": 2, "c": 3})
    gaps = dict(CH, labels={"background": 0, "a": 2, "b": 5})
    one = {"modality": {"0": "ct"}, "labels": {"background": 0, "a": 1, "b": 2}}
    assert TR.determine_num_input_channels(pm, low, plain) == 2
    assert TR.determine_num_input_channels(pm, full, plain) == 5
    assert TR.determine_num_input_channels(pm, full, gaps) == 4
    assert pm.get_label_manager(gaps).foreground_labels == [2, 5]
    assert TR.determine_num_input_channels(pm, low, one) == 1 and TR.determine_num_input_channels(pm, full, one) == 3


class _Stub:
    """The attributes _check_cascade reads, without a device."""

    def __init__(self, cls, cfg, dataset_json, pm):
        self.configuration_manager = cfg
        self.label_manager = pm.get_label_manager(dataset_json)
        self._cls = cls

    is_cascaded = TR.nnUNetTrainerMI355.is_cascaded

    def check(self):
        return self._cls._check_cascade(self)


def test_refusals_say_what_they_refuse():
    plans, pm = _pm()
    full, low = pm.get_configuration('3d_cascade_fullres'), pm.get_configuration('3d_lowres')
    base = TR.nnUNetTrainerMI355
    plain = dict(CH, labels={"background": 0, "a": 1, "b": 2})
    _Stub(base, full, plain, pm).check()
    _Stub(base, low, plain, pm).check()
    regions = dict(CH, labels={"background": 0, "whole": [1, 2], "core": 2}, regions_class_order=[1, 2])
    with pytest.raises(NotImplementedError, match="cascade.*region"):
        _Stub(base, full, regions, pm).check()
    _Stub(base, low, regions, pm).check()      # regions without a cascade stay allowed
    ignore = dict(CH, labels={"background": 0, "a": 1, "ignore": 2})
    with pytest.raises(NotImplementedError, match="cascade.*ignore label"):
        _Stub(base, full, ignore, pm).check()
    many = dict(CH, labels=dict({"background": 0}, **{f"l{i}": i for i in range(1, 10)}))
    with pytest.raises(NotImplementedError, match="cascade.*at most 8"):
        _Stub(base, full, many, pm).check()
    for cls in (TR.ContrastiveTrainerMI355, TR.FinalNetTrainerMI355):
        with pytest.raises(NotImplementedError, match="cascade.*dual-branch"):
            _Stub(cls, full, plain, pm).check()
        _Stub(cls, low, plain, pm).check()
    p2 = TR.make_plans((16, 16), [(1, 1), (2, 2)], configuration='2d', previous_stage_name='3d_lowres')
    with pytest.raises(NotImplementedError, match="cascade.*2-D"):
        _Stub(base, TR.PlansManager(p2).get_configuration('2d'), plain, pm).check()


# ------------------------------------------------------------------------------------------------ loader planning
class ToyDataset:
    def __init__(self, shapes, C=2, seed=0, prev=False):
        rng = np.random.default_rng(seed)
        self.cases = {}
        for i, shp in enumerate(shapes):
            data = rng.standard_normal((C, *shp)).astype(np.float32)
            seg = (rng.random((1, *shp)) > 0.97).astype(np.int16) * rng.integers(1, 3, (1, *shp)).astype(np.int16)
            loc = {c: np.argwhere(seg == c) for c in (1, 2)}
            if prev:
                seg = np.concatenate([seg, np.random.default_rng(100 + seed + i).integers(0, 3, (1, *shp)).astype(np.int16)])
            self.cases[f"case{i}"] = (data, seg, {"class_locations": loc})

    def keys(self):
        return self.cases.keys()

    def load_case(self, k):
        return self.cases[k]


class Labels:
    all_labels = [1, 2]
    has_ignore_label = False


FORMS = {"plain": dict(), "spatial": dict(rotation_for_DA=ROT), "intensity": dict(rotation_for_DA=ROT,
                                                                                   intensity_augmentation=True)}


def make_loader(module, form, prev=False, **kw):
    args = dict(oversample_foreground_percent=0.33, mirror_axes=(0, 1, 2), device="cpu")
    args.update(FORMS[form])
    args.update(kw)
    patch = (12, 16, 16) if form == "plain" else (18, 22, 22)
    return module.DeviceDataLoader3D(ToyDataset([(20, 24, 28), (9, 30, 12)], prev=prev), 4, patch, (12, 16, 16), Labels(),
                                     **args)


def record_plans(module):
    """What tests/golden/cascade_parent_plans.json holds (written from the commit before the cascade mode existed)."""
    out = {}
    for form in FORMS:
        dl = make_loader(module, form)
        for seed in range(4):
            np.random.seed(seed)
            plans = [dl.plan_batch() for _ in range(2)]
            out[f"{form}/{seed}"] = json.loads(json.dumps({"plans": plans, "tail": np.random.uniform()}))
    return out


def test_a_loader_without_the_cascade_mode_plans_and_draws_what_it_did_before():
    with open(os.path.join(GOLDEN, "cascade_parent_plans.json")) as f:
        want = json.load(f)
    got = record_plans(DLD)
    assert got.keys() == want["cases"].keys() and len(got) == 12
    for k in got:
        assert got[k] == want["cases"][k], k


@pytest.mark.parametrize("form", list(FORMS))
def test_cascade_plan_is_the_old_plan_plus_the_cascade_draws(form):
    base = make_loader(DLD, form)
    val = make_loader(DLD, form, prev=True, cascade_labels=[1, 2])
    aug = make_loader(DLD, form, prev=True, cascade_labels=[1, 2], cascade_augmentation=True)
    assert val.data_shape == (4, 4, 12, 16, 16) and val.seg_shape == (4, 1, 12, 16, 16) and base.data_shape[1] == 2
    for seed in range(6):
        np.random.seed(seed)
        a = base.plan_batch()
        tail = np.random.uniform()
        np.random.seed(seed)
        assert val.plan_batch() == a and np.random.uniform() == tail    # the validation mode draws nothing more
        np.random.seed(seed)
        order = list(aug._cascade_order)
        c = aug.plan_batch()
        assert c[:-1] == a and c[-1]['cascade'] is True
        # replay: the cascade draws come after the mirror draws
        np.random.seed(seed)
        base.plan_batch()
        binary = REF.draw_binary_operator(4, order)
        assert binary == c[-1]['binary'] and order == aug._cascade_order
        for steps in c[-1]['remove']:
            if np.random.uniform() < 0.2:
                assert [s[0] for s in steps] == [0, 1]
                for ch, u, other in steps:
                    assert np.random.uniform() < 1
                    assert u == np.random.uniform() and 0 <= u < 1
                    assert not np.random.uniform() < 0.0 and other is None
                    np.random.choice([i for i in range(2) if i != ch])
            else:
                assert steps is None


def test_draw_cascade_is_reproducible_and_its_rates_are_the_transforms():
    dl = make_loader(DLD, "plain", prev=True, cascade_labels=[1, 2], cascade_augmentation=True,
                     cascade_fill_with_other_class_p=0.5)
    np.random.seed(5)
    a = [dl.draw_cascade(4) for _ in range(250)]
    dl._cascade_order[:] = [0, 1]
    np.random.seed(5)
    b = [dl.draw_cascade(4) for _ in range(250)]
    assert a == b
    binary = [s for d in a for s in d['binary']]
    remove = [s for d in a for s in d['remove']]
    assert abs(np.mean([s is not None for s in binary]) - 0.4) < 0.06
    assert abs(np.mean([s is not None for s in remove]) - 0.2) < 0.05
    steps = [t for s in binary if s for t in s]
    assert {t[1] for t in steps} == {0, 1, 2, 3} and all(1 <= t[2] < 8 for t in steps)
    assert all(sorted(t[0] for t in s) == [0, 1] for s in binary if s)
    fills = [t[2] for s in remove if s for t in s]
    assert abs(np.mean([f is not None for f in fills]) - 0.5) < 0.12
    assert all(f is None or f == 1 - c for s in remove if s for c, _, f in s)


def test_loader_refusals():
    with pytest.raises(NotImplementedError, match="1..8 foreground labels, got 9"):
        make_loader(DLD, "plain", prev=True, cascade_labels=list(range(1, 10)))
    with pytest.raises(ValueError, match="two channels"):
        make_loader(DLD, "plain", prev=False, cascade_labels=[1, 2])
    with pytest.raises(NotImplementedError, match="cascade"):
        DLD.DeviceDataLoader2D(ToyDataset([(20, 24, 28)], prev=True), 2, (16, 16), (16, 16), Labels(), device="cpu",
                               cascade_labels=[1, 2])
    dl = make_loader(DLD, "plain", prev=True, cascade_labels=[1, 2], cascade_augmentation=True)
    np.random.seed(0)
    with pytest.raises(RuntimeError):
        dl.generate_train_batch(dl.plan_batch())   # no CPU path
