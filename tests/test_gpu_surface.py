"""GPU tests of the surface distances (csrc/surface.hip, surface.py, evaluation.compute_surface_metrics,
perform_actual_validation(surface_metrics=True)) against the fp64 scipy restatement in surface_ref.py.

Bounds.  Unit spacing: squared distances are integers and must be EQUAL on every voxel; their roots equal scipy's bit for
bit.  With a spacing, sum_i ((d_i s_i)^2) followed by a root carries at most about 3.5 units of fp64 roundoff in any
evaluation order, two evaluations differ by at most 7 * 2^-53 = 7.8e-16 relative: 1e-14 leaves a decade.  Order
statistics move by no more than the largest element error and the lerp adds two roundings: 1e-13.  A mean of n
non-negative terms is within (n - 1) * 2^-53 of the true one in any summation order: 2 n 2^-53 between two of them.
"""
import numpy as np
import pytest
import torch

import surface_ref as REF
from multimodal_mvd_seg_amd import evaluation as EV
from multimodal_mvd_seg_amd import surface as SF

DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu

SPACINGS = [(2.5, 0.7, 0.7), (1.0, 1.0, 3.0), (0.4, 0.4, 0.4)]
REL = 1e-14
REL_STAT = 1e-13


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from multimodal_mvd_seg_amd import _lib
    _lib.load()


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def rel_err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    if got.size == 0:
        return 0.0
    zero = want == 0
    assert np.array_equal(got[zero], want[zero])
    return float(np.max(np.abs(got[~zero] - want[~zero]) / want[~zero])) if (~zero).any() else 0.0


def face_mask(shape=(21, 27, 33)):
    m = REF.blob_mask(shape, seed=5, sigma=2.0, fill=0.25)
    D, H, W = shape
    m[0, 3:9, 4:11] = True
    m[D - 1, 10:15, 20:30] = True
    m[5:9, 0, 6:12] = True
    m[10:16, H - 1, 1:7] = True
    m[3:8, 12:18, 0] = True
    m[12:19, 5:9, W - 1] = True
    m[0, 0, 0] = m[D - 1, H - 1, W - 1] = True
    return m


@pytest.mark.parametrize("connectivity", [1, 2, 3])
def test_border_equals_the_reference_on_every_voxel(connectivity):
    m = face_mask()
    for f in (m[0], m[-1], m[:, 0], m[:, -1], m[:, :, 0], m[:, :, -1]):
        assert f.any()
    got = SF.surface_border(G(m), connectivity)
    assert got.dtype == torch.uint8
    assert np.array_equal(got.cpu().numpy().astype(bool), REF.border(m, connectivity))
    full = np.ones((5, 6, 70), dtype=bool)
    assert np.array_equal(SF.surface_border(G(full), connectivity).cpu().numpy().astype(bool), REF.border(full, connectivity))


def edt_cases():
    """(name, sites): the transform's input is ~sites"""
    rng = np.random.default_rng(11)
    out = [("blob", REF.border(REF.blob_mask((17, 23, 29), 2, 2.0, 0.3)))]
    out.append(("extent 1", rng.random((1, 31, 37)) < 0.03))
    s = np.zeros((19, 21, 23), dtype=bool)
    s[4, 17, 2] = True
    out.append(("single site", s))
    s = np.zeros((15, 18, 75), dtype=bool)                # rows without a site, and whole z slices without one
    s[3:5, 2:6, 10:70:7] = True
    s[11, 16, 74] = True
    out.append(("empty lines", s))
    s = np.zeros((33, 35, 70), dtype=bool)                # longest distances
    s[0:2, 0:2, 0:2] = True
    out.append(("corner", s))
    out.append(("wide rows", rng.random((5, 9, 200)) < 0.01))
    out.append(("dense", rng.random((13, 11, 65)) < 0.4))
    return out


EDT_CASES = edt_cases()


@pytest.mark.parametrize("name,sites", EDT_CASES, ids=[c[0] for c in EDT_CASES])
def test_unit_spacing_transform_is_exact_on_every_voxel(name, sites):
    import scipy.ndimage as ndi
    assert sites.any()
    want = ndi.distance_transform_edt(~sites)
    sq = SF.distance_transform_edt(G(~sites), return_squared=True)
    assert sq.dtype == torch.int32 and tuple(sq.shape) == sites.shape
    assert np.array_equal(sq.cpu().numpy().astype(np.int64), np.round(want ** 2).astype(np.int64))
    got = SF.distance_transform_edt(G(~sites))
    assert got.dtype == torch.float64
    assert np.array_equal(got.cpu().numpy(), want)       # the device root is correctly rounded


@pytest.mark.parametrize("spacing", SPACINGS)
def test_spaced_transform_on_every_voxel(spacing):
    import scipy.ndimage as ndi
    worst = 0.0
    for name, sites in EDT_CASES:
        want = ndi.distance_transform_edt(~sites, sampling=spacing)
        got = SF.distance_transform_edt(G(~sites), sampling=spacing).cpu().numpy()
        e = rel_err(got, want)
        sq = SF.distance_transform_edt(G(~sites), sampling=spacing, return_squared=True)
        assert sq.dtype == torch.float64
        worst = max(worst, e)
        print(f"spacing {spacing} {name}: max rel err {e:.3e}")
        assert e <= REL, (name, e)
    print(f"spacing {spacing}: worst {worst:.3e}")


PAIR = REF.blob_pair((37, 45, 71), seed=7, sigma=2.5, fill=0.15)


@pytest.mark.parametrize("spacing", [None] + SPACINGS)
@pytest.mark.parametrize("connectivity", [1, 3])
def test_surface_distances_and_metrics(spacing, connectivity):
    a, b = PAIR
    ga, gb = G(a), G(b)
    n = {}
    for (x, y, gx, gy, tag) in ((a, b, ga, gb, "ab"), (b, a, gb, ga, "ba")):
        want = np.sort(REF.surface_distances(x, y, spacing, connectivity))
        got = SF.surface_distances(gx, gy, spacing, connectivity)
        assert got.dtype == torch.float64 and got.dim() == 1 and got.is_cuda
        got = np.sort(got.cpu().numpy())
        n[tag] = len(want)
        if spacing is None:
            assert np.array_equal(got, want)
        else:
            e = rel_err(got, want)
            print(f"sds {tag} spacing {spacing}: {e:.3e}")
            assert e <= REL
    assert n["ab"] != n["ba"]
    want_hd, want_95 = REF.hd(a, b, spacing, connectivity), REF.hd95(a, b, spacing, connectivity)
    got_hd, got_95 = SF.hd(ga, gb, spacing, connectivity), SF.hd95(ga, gb, spacing, connectivity)
    assert isinstance(got_hd, float) and isinstance(got_95, float)
    print(f"hd {got_hd!r} / {want_hd!r}  hd95 {got_95!r} / {want_95!r}")
    if spacing is None:
        assert got_hd == want_hd and got_95 == want_95
    else:
        assert abs(got_hd - want_hd) <= REL_STAT * want_hd and abs(got_95 - want_95) <= REL_STAT * want_95
    for fn, ref, cnt in ((SF.asd, REF.asd, n["ab"]), (SF.assd, REF.assd, max(n.values()))):
        got, want = fn(ga, gb, spacing, connectivity), ref(a, b, spacing, connectivity)
        bound = 2 * cnt * 2.0 ** -53
        print(f"{fn.__name__} {got!r} / {want!r} bound {bound:.2e}")
        assert abs(got - want) <= bound * want
    assert SF.asd(gb, ga, spacing, connectivity) != SF.asd(ga, gb, spacing, connectivity)
    # the reference's wrappers
    assert SF.hausdorff_distance(ga, gb, voxel_spacing=spacing, connectivity=connectivity) == got_hd
    assert SF.hausdorff_distance_95(ga, gb, voxel_spacing=spacing, connectivity=connectivity) == got_95
    assert SF.avg_surface_distance_symmetric(ga, gb, voxel_spacing=spacing, connectivity=connectivity) == \
        SF.assd(ga, gb, spacing, connectivity)


def test_nan_rule_and_empty_masks_on_the_device():
    a, _ = PAIR
    ga = G(a)
    empty, full = torch.zeros_like(ga), torch.ones_like(ga)
    for fn in (SF.hausdorff_distance, SF.hausdorff_distance_95, SF.avg_surface_distance,
               SF.avg_surface_distance_symmetric):
        for t, r in ((empty, ga), (ga, empty), (full, ga), (ga, full)):
            assert np.isnan(fn(t, r))
            assert fn(t, r, nan_for_nonexisting=False) == 0
    with pytest.raises(RuntimeError, match="first supplied array"):
        SF.hd(empty, ga)
    with pytest.raises(RuntimeError, match="second supplied array"):
        SF.hd95(ga, empty)
    assert SF.hd(full, ga) == REF.hd(np.ones_like(a), a)


@pytest.mark.parametrize("spacing", [None, (2.5, 0.7, 0.7)])
def test_boxed_transform_equals_the_full_volume_one(spacing, monkeypatch):
    a = np.zeros((40, 52, 90), dtype=bool)
    b = np.zeros_like(a)
    pa, pb = REF.blob_pair((15, 20, 31), seed=9, sigma=2.0, fill=0.3)
    a[20:35, 3:23, 50:81], b[20:35, 3:23, 50:81] = pa, pb
    ga, gb = G(a), G(b)
    boxed = [SF.surface_distances(ga, gb, spacing), SF.surface_distances(gb, ga, spacing)]
    boxed_m = SF._binary_metrics(ga, gb, spacing, 1)
    monkeypatch.setattr(SF, "_FORCE_FULL_BOX", True)
    full = [SF.surface_distances(ga, gb, spacing), SF.surface_distances(gb, ga, spacing)]
    full_m = SF._binary_metrics(ga, gb, spacing, 1)
    for x, y in zip(boxed, full):
        assert torch.equal(x, y) and x.numel() > 100
    assert boxed_m == full_m
    if spacing is None:
        assert np.array_equal(boxed[0].cpu().numpy(), np.sort(REF.surface_distances(a, b)))


def five_label_case():
    shape = (31, 43, 67)
    ref = np.zeros(shape, dtype=np.int16)
    pred = np.zeros(shape, dtype=np.uint8)
    for l in (1, 2, 3, 4, 5):
        a, b = REF.blob_pair(shape, seed=30 + l, sigma=2.5, fill=0.08, shift=(1, 1, -2))
        ref[b & (ref == 0)] = l
        if l != 4:                                        # label 4 is absent from the prediction
            pred[a & (pred == 0)] = l
    return ref, pred, [1, 2, 3, 4, 5, (2, 3)]


@pytest.mark.parametrize("spacing", [None, (2.5, 0.7, 0.7)])
def test_compute_surface_metrics_on_a_five_label_volume(spacing):
    ref, pred, regions = five_label_case()
    got = EV.compute_surface_metrics(G(ref), G(pred), regions, spacing=spacing, connectivity=1)
    want = REF.surface_metrics(ref, pred, regions, spacing, 1)
    assert list(got.keys()) == list(want.keys()) == [1, 2, 3, 4, 5, (2, 3)]
    for key in want:
        assert set(got[key]) == {'HD', 'HD95', 'ASSD'}
        if key == 4:
            assert all(np.isnan(v) for v in got[key].values()) and all(np.isnan(v) for v in want[key].values())
            continue
        nb = int(REF.border(np.isin(ref, key)).sum() + REF.border(np.isin(pred, key)).sum())
        print(key, got[key], want[key])
        if spacing is None:
            assert got[key]['HD'] == want[key]['HD'] and got[key]['HD95'] == want[key]['HD95']
        else:
            assert abs(got[key]['HD'] - want[key]['HD']) <= REL_STAT * want[key]['HD']
            assert abs(got[key]['HD95'] - want[key]['HD95']) <= REL_STAT * want[key]['HD95']
        bound = 2 * nb * 2.0 ** -53
        assert abs(got[key]['ASSD'] - want[key]['ASSD']) <= bound * want[key]['ASSD']
    assert got[(2, 3)] != got[2]
    # numpy volumes are uploaded; an ignore label is refused
    assert EV.compute_surface_metrics(ref, pred, [1], spacing=spacing) == {1: got[1]}
    with pytest.raises(NotImplementedError):
        EV.compute_surface_metrics(G(ref), G(pred), [1], ignore_label=3)


def test_twelve_repetitions_are_bit_identical():
    ref, pred, regions = five_label_case()
    gr, gp = G(ref), G(pred)
    for spacing in (None, (2.5, 0.7, 0.7)):
        first = EV.compute_surface_metrics(gr, gp, regions, spacing=spacing)
        for _ in range(11):
            again = EV.compute_surface_metrics(gr, gp, regions, spacing=spacing)
            for key in first:
                for m in first[key]:
                    x, y = first[key][m], again[key][m]
                    assert (np.isnan(x) and np.isnan(y)) or np.float64(x).tobytes() == np.float64(y).tobytes(), (key, m)


def test_perform_actual_validation_with_surface_metrics():
    import test_gpu_export as TE
    tr = TE._trainer(False)
    cases = [TE._case(0), TE._case(1)]
    plain, segs0 = tr.perform_actual_validation(cases, return_segmentations=True)
    with_surf, segs1 = tr.perform_actual_validation(cases, return_segmentations=True, surface_metrics=True,
                                                    surface_connectivity=1)
    labels = [1, 2, 3]
    base_keys = {'Dice', 'IoU', 'FP', 'TP', 'FN', 'TN', 'n_pred', 'n_ref'}
    for case, s0, s1, c0, c1 in zip(cases, segs0, segs1, plain['metric_per_case'], with_surf['metric_per_case']):
        assert torch.equal(s0, s1)
        want = REF.surface_metrics(case['seg'][0], s1.cpu().numpy(), labels, case['properties']['spacing'], 1)
        for r in labels:
            assert set(c0['metrics'][r]) == base_keys                       # the default adds nothing
            assert set(c1['metrics'][r]) == base_keys | {'HD', 'HD95', 'ASSD'}
            for k in base_keys:
                x, y = c0['metrics'][r][k], c1['metrics'][r][k]
                assert x == y or (np.isnan(x) and np.isnan(y))
            for k in ('HD', 'HD95'):
                x, y = c1['metrics'][r][k], want[r][k]
                print(r, k, x, y)
                assert (np.isnan(x) and np.isnan(y)) or abs(x - y) <= REL_STAT * y
            x, y = c1['metrics'][r]['ASSD'], want[r]['ASSD']
            nb = int(REF.border(case['seg'][0] == r).sum() + REF.border(s1.cpu().numpy() == r).sum())
            assert (np.isnan(x) and np.isnan(y)) or abs(x - y) <= 2 * nb * 2.0 ** -53 * y
        assert np.isfinite([want[r]['HD'] for r in labels]).any(), "all-NaN surface metrics would test nothing"
    assert set(plain['mean'][1]) == base_keys and set(with_surf['mean'][1]) == base_keys | {'HD', 'HD95', 'ASSD'}
    assert set(plain['foreground_mean']) == base_keys
    for k in base_keys:
        assert plain['foreground_mean'][k] == with_surf['foreground_mean'][k] or np.isnan(plain['foreground_mean'][k])
    assert with_surf['mean'][1]['HD95'] == pytest.approx(
        np.nanmean([c['metrics'][1]['HD95'] for c in with_surf['metric_per_case']]), nan_ok=True)


def test_full_size_case():
    """288 x 384 x 384, one label, a blob of realistic size (about 2 % of the volume), anisotropic spacing."""
    import scipy.ndimage as ndi
    shape = (288, 384, 384)
    rng = np.random.default_rng(4)
    low = ndi.gaussian_filter(rng.standard_normal((72, 96, 96)), 5.0, mode='nearest')
    low[:20] = low[50:] = low.min()
    low[:, :25] = low[:, 70:] = low.min()
    field = ndi.zoom(low, 4, order=1, mode='nearest', grid_mode=True)
    assert field.shape == shape
    a = field > np.quantile(field, 0.98)
    b = np.roll(a, (2, -3, 1), axis=(0, 1, 2)) | (np.roll(field, (9, 5, -7), axis=(0, 1, 2)) > np.quantile(field, 0.997))
    spacing = (2.5, 0.7, 0.7)
    got = EV.compute_surface_metrics(G(b.astype(np.uint8)), G(a.astype(np.uint8)), [1], spacing=spacing)[1]
    s_ab = REF.surface_distances(a, b, spacing, 1)          # the two scipy transforms, each used once
    s_ba = REF.surface_distances(b, a, spacing, 1)
    want = {'HD': float(max(s_ab.max(), s_ba.max())), 'HD95': float(np.percentile(np.hstack((s_ab, s_ba)), 95)),
            'ASSD': float(np.mean((s_ab.mean(), s_ba.mean())))}
    nb = max(len(s_ab), len(s_ba))
    print(got, want, len(s_ab), len(s_ba))
    assert abs(got['HD'] - want['HD']) <= REL_STAT * want['HD']
    assert abs(got['HD95'] - want['HD95']) <= REL_STAT * want['HD95']
    assert abs(got['ASSD'] - want['ASSD']) <= 2 * nb * 2.0 ** -53 * want['ASSD']
