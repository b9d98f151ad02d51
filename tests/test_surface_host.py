"""CPU tests of the surface-distance module (multimodal_mvd_seg_amd/surface.py): the host arithmetic
(footprints, numpy's percentile restated), the refusals, the reference's NaN rule in the scipy restatement and the
restatement itself against the brute-force definition.  Nothing here touches a GPU."""
import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

import surface_ref as REF
from multimodal_mvd_seg_amd import evaluation as EV
from multimodal_mvd_seg_amd import surface as SF


@pytest.mark.parametrize("connectivity", [1, 2, 3])
def test_footprint_offsets_are_scipys_binary_structure(connectivity):
    fp = ndi.generate_binary_structure(3, connectivity)
    want = sorted(tuple(int(v) - 1 for v in p) for p in np.argwhere(fp))
    got = sorted(SF.footprint_offsets(connectivity))
    assert got == want and len(got) == {1: 7, 2: 19, 3: 27}[connectivity]


def test_footprint_refuses_other_connectivities():
    for c in (0, 4):
        with pytest.raises(ValueError):
            SF.footprint_offsets(c)


@pytest.mark.parametrize("n", [1, 2, 19, 20, 21, 100000])
def test_host_percentile_is_numpys_bit_for_bit(n):
    rng = np.random.default_rng(n)
    x = np.sqrt(rng.integers(0, max(2, n // 3), size=n).astype(np.float64))   # repeated values, irrational steps
    for q in (95, 50, 0, 100):
        assert SF.percentile(x, q) == float(np.percentile(x, q)), (n, q)
    lo, hi, g = SF.percentile_indices(n, 95.0)
    s = np.sort(x)
    assert 0 <= lo <= hi <= n - 1 and hi - lo <= 1
    assert SF.lerp(s[lo], s[hi], g) == float(np.percentile(x, 95))


def test_nan_rule_for_empty_and_full_masks_in_the_restatement():
    a, b = REF.blob_pair((9, 11, 13), seed=1, sigma=1.5)
    empty, full = np.zeros_like(a), np.ones_like(a)
    for fn in (REF.hausdorff_distance, REF.hausdorff_distance_95, REF.avg_surface_distance,
               REF.avg_surface_distance_symmetric):
        for t, r in ((empty, b), (a, empty), (full, b), (a, full)):
            assert np.isnan(fn(t, r))
            assert fn(t, r, nan_for_nonexisting=False) == 0
        assert np.isfinite(fn(a, b))
    m = REF.surface_metrics(np.where(b, 1, 0), np.where(a, 1, 0), [1, 2, (1, 2)])
    assert np.isnan(m[2]['HD']) and np.isfinite(m[1]['HD95']) and m[(1, 2)] == m[1]


def test_refusals():
    ok = torch.zeros((4, 5, 6), dtype=torch.uint8)
    with pytest.raises(NotImplementedError, match="1024"):
        SF.distance_transform_edt(torch.zeros((1025, 1, 1), dtype=torch.uint8))
    with pytest.raises(NotImplementedError, match="1024"):
        SF.hd(torch.zeros((1, 1, 1025), dtype=torch.uint8), torch.zeros((1, 1, 1025), dtype=torch.uint8))
    for bad in ((1.0, 0.0, 1.0), (1.0, -2.0, 1.0), (1.0, 1.0), (1.0, float("nan"), 1.0)):
        with pytest.raises(ValueError, match="positive"):
            SF.distance_transform_edt(ok, sampling=bad)
        with pytest.raises(ValueError, match="positive"):
            SF.hd95(ok, ok, voxelspacing=bad)
    with pytest.raises(ValueError, match="connectivity"):
        SF.surface_border(ok, connectivity=4)
    with pytest.raises(NotImplementedError, match="ignore label"):
        EV.compute_surface_metrics(ok, ok, [1], ignore_label=2)
    with pytest.raises(ValueError, match="3-D"):
        SF.surface_border(torch.zeros((5, 6), dtype=torch.uint8))
    for call in (lambda: SF.distance_transform_edt(ok), lambda: SF.surface_border(ok), lambda: SF.surface_distances(ok, ok),
                 lambda: SF.hd(ok, ok), lambda: SF.hd95(ok, ok), lambda: SF.asd(ok, ok), lambda: SF.assd(ok, ok),
                 lambda: SF.hausdorff_distance_95(ok, ok), lambda: EV.compute_surface_metrics(ok, ok, [1])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


@pytest.mark.parametrize("spacing", [None, (2.5, 0.7, 0.7)])
def test_restatement_equals_the_brute_force_definition(spacing):
    a, b = REF.blob_pair((14, 19, 17), seed=3, sigma=2.0)
    for x, y in ((a, b), (b, a)):
        sds = REF.surface_distances(x, y, spacing, 1)
        assert len(sds) > 100
        assert np.array_equal(sds, REF.brute_force_sds(x, y, spacing, 1))
    assert not np.array_equal(np.sort(REF.surface_distances(a, b, spacing)), np.sort(REF.surface_distances(b, a, spacing)))
