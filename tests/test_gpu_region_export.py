"""GPU tests of the region branch of the segmentation export (mvd_export_resize_regions_u8, mvd_export_resize_sigmoid_f32;
label_handling.py:163-171, :199-205) against the scipy oracle of export_ref.py followed by fp32 torch.sigmoid and
the reference's overwrite loop.

Margin rule (the existing export test's): three fp32 lerps of |logit| <= 64 err by at most about 2.3e-5 in the logit, so a
head's sign cannot differ from the fp64 oracle's where |z_r| >= 1e-4; labels must be EQUAL on every voxel whose fp64
interpolated logits all satisfy that, and the voxels under the margin may be at most 1e-3 of the volume (asserted from the
oracle alone, on the CPU, in test_test_logits_stay_under_the_cap).  sigmoid's derivative is at most 1/4: 1e-5 on
probabilities."""
import itertools

import numpy as np
import pytest
import torch

import export_ref as REF
import region_loss_ref as RR
from multimodal_mvd_seg_amd import export as EX

DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu

PROB_TOL = 1e-5
MARGIN = 1e-4
MAX_EXCLUDED = 1e-3
ORDER = [1, 2, 3]

# shape in, shape out, separate-z axis, pre-crop volume, bbox corner, transpose_backward
CASES = [
    ((37, 45, 52), (61, 83, 70), None, (61, 83, 70), (0, 0, 0), (0, 1, 2)),
    ((37, 45, 52), (20, 31, 40), None, (23, 40, 41), (2, 5, 1), (0, 1, 2)),
    ((37, 45, 52), (61, 83, 70), 0, (61, 83, 70), (0, 0, 0), (0, 1, 2)),
    ((37, 45, 52), (61, 83, 70), 2, (66, 85, 77), (3, 1, 7), (2, 0, 1)),
]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from multimodal_mvd_seg_amd import _lib
    _lib.load()


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def oracle(x, new, full, lo, tb, axis, order):
    """-> (uint8 segmentation, float32 sigmoid planes, fp64 margin = min_r |z_r|) in the original axis order"""
    res = REF.resample_logits(x, new, axis)
    prob = torch.sigmoid(torch.from_numpy(res.astype(np.float32))).numpy()
    seg = RR.regions_to_segmentation(prob, order).astype(np.uint8)
    return (REF.paste_transpose(seg, full, lo, tb), REF.paste_transpose(prob, full, lo, tb),
            REF.paste_transpose(np.abs(res).min(0), full, lo, tb, fill=np.inf))


def check_labels(seg, seg_ref, mar, what=""):
    low = mar < MARGIN
    share = float(low.mean())
    mism = int(((seg != seg_ref) & ~low).sum())
    print(f"{what}: voxels {seg.size}, under the margin {share:.2e}, mismatches above it {mism}, "
          f"mismatches in all {int((seg != seg_ref).sum())}")
    assert share <= MAX_EXCLUDED, share
    assert mism == 0, mism


@pytest.mark.parametrize("shape,new,axis,full,lo,tb", CASES)
def test_labels_and_sigmoid_planes_match_the_scipy_oracle(shape, new, axis, full, lo, tb):
    x = REF.smooth_logits(3, shape, seed=0)
    seg_ref, prob_ref, mar = oracle(x, new, full, lo, tb, axis, ORDER)
    seg, prob = EX.resize_logits_to_segmentation(G(x), new, full, lo, tb, axis, return_probabilities=True,
                                                 regions_class_order=ORDER)
    assert seg.dtype == torch.uint8 and tuple(seg.shape) == seg_ref.shape and tuple(prob.shape) == prob_ref.shape
    seg, prob = seg.cpu().numpy(), prob.cpu().numpy()
    err = float(np.abs(prob.astype(np.float64) - prob_ref).max())
    print(f"{shape}->{new} sep-z {axis}: max |p - p_oracle| = {err:.3e}")
    assert np.isfinite(prob).all() and err <= PROB_TOL, err
    check_labels(seg, seg_ref, mar, f"{shape}->{new} sep-z {axis}")
    inside = REF.paste_transpose(np.ones(new, bool), full, lo, tb)
    assert not prob[:, ~inside].any() and not seg[~inside].any()      # no probs[0] = 1 for regions


# ------------------------------------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("order", [[1, 2, 3], [3, 2, 1], [2, 7, 5]])
def test_equal_shape_is_the_overwrite_loop(order):
    rng = np.random.default_rng(1)
    x = rng.standard_normal((3, 19, 23, 29)).astype(np.float32)
    x.reshape(-1)[::13] = 0.0                                           # exactly 0 is "off"
    seg = EX.resize_logits_to_segmentation(G(x), x.shape[1:], x.shape[1:], (0, 0, 0), regions_class_order=order)
    want = RR.regions_to_segmentation(torch.sigmoid(torch.from_numpy(x)).numpy(), order).astype(np.uint8)
    assert np.array_equal(seg.cpu().numpy(), want)


def test_integer_logits_at_twofold_upsampling_are_exact():
    """Weights 1/4 and 3/4 on small integers: every fp32 operation is exact, the sign of every head equals the fp64
    oracle's on every voxel, zeros included."""
    rng = np.random.default_rng(2)
    x = rng.integers(-8, 9, size=(4, 10, 12, 14)).astype(np.float32)
    new = tuple(2 * s for s in x.shape[1:])
    res = REF.resample_logits(x, new)
    assert (res == 0).any()
    order = [4, 3, 2, 1]
    seg = EX.resize_logits_to_segmentation(G(x), new, new, (0, 0, 0), regions_class_order=order).cpu().numpy()
    want = np.zeros(new, np.uint8)
    for i, c in enumerate(order):
        want[res[i] > 0] = c
    assert np.array_equal(seg, want)


def test_a_later_smaller_region_overwrites_an_earlier_one_and_the_reverse():
    x = np.full((2, 6, 6, 6), -5.0, np.float32)
    x[0, 1:5, 1:5, 1:5] = 5.0      # whole
    x[1, 2:4, 2:4, 2:4] = 5.0      # core, inside whole
    a = EX.resize_logits_to_segmentation(G(x), (6, 6, 6), (6, 6, 6), (0, 0, 0), regions_class_order=[1, 2]).cpu().numpy()
    assert (a[2:4, 2:4, 2:4] == 2).all() and (a == 1).sum() == 64 - 8 and (a == 0).sum() == 216 - 64
    y = x[::-1].copy()             # the small region first: the large one, written later, hides it
    b = EX.resize_logits_to_segmentation(G(y), (6, 6, 6), (6, 6, 6), (0, 0, 0), regions_class_order=[2, 1]).cpu().numpy()
    assert (b == 1).sum() == 64 and not (b == 2).any()


@pytest.mark.parametrize("lo", [(0, 0, 0), (4, 0, 0), (0, 6, 0), (0, 0, 5), (4, 6, 5), (2, 3, 1)])
def test_the_bbox_may_touch_every_face(lo):
    """integer logits at twofold upsampling: exact, so the labels are compared on every voxel"""
    rng = np.random.default_rng(6)
    x = rng.integers(-8, 9, size=(3, 6, 7, 7)).astype(np.float32)
    x[0] = np.abs(x[0]) + 1                                            # head 0 is on everywhere inside
    new, full = (12, 14, 14), (16, 20, 19)
    seg_ref, prob_ref, _ = oracle(x, new, full, lo, (0, 1, 2), None, ORDER)
    seg, prob = EX.resize_logits_to_segmentation(G(x), new, full, lo, return_probabilities=True, regions_class_order=ORDER)
    seg, prob = seg.cpu().numpy(), prob.cpu().numpy()
    inside = np.zeros(full, bool)
    inside[tuple(slice(l, l + n) for l, n in zip(lo, new))] = True
    assert (seg[inside] > 0).all() and not seg[~inside].any() and not prob[:, ~inside].any()
    assert np.array_equal(seg, seg_ref)
    assert float(np.abs(prob - prob_ref).max()) <= PROB_TOL


def test_every_transpose_backward_equals_the_identity_result_transposed():
    x = REF.smooth_logits(3, (10, 13, 17), seed=7)
    new, full, lo = (15, 21, 19), (18, 22, 23), (1, 0, 4)
    kw = dict(return_probabilities=True, regions_class_order=ORDER)
    seg0, prob0 = EX.resize_logits_to_segmentation(G(x), new, full, lo, (0, 1, 2), **kw)
    seg0, prob0 = seg0.cpu().numpy(), prob0.cpu().numpy()
    for tb in itertools.permutations(range(3)):
        seg, prob = EX.resize_logits_to_segmentation(G(x), new, full, lo, tb, **kw)
        assert seg.is_contiguous() and np.array_equal(seg.cpu().numpy(), seg0.transpose(tb)), tb
        assert np.array_equal(prob.cpu().numpy(), prob0.transpose([0] + [a + 1 for a in tb])), tb
        # and every order against the scipy oracle itself, not only against the device's identity result
        seg_ref, prob_ref, mar = oracle(x, new, full, lo, tb, None, ORDER)
        check_labels(seg.cpu().numpy(), seg_ref, mar, f"transpose_backward {tb}")
        assert float(np.abs(prob.cpu().numpy() - prob_ref).max()) <= PROB_TOL, tb


def test_convert_with_a_label_manager_takes_the_regions_branch():
    from multimodal_mvd_seg_amd.trainer import ConfigurationManager, LabelManager, PlansManager
    lm = LabelManager({"background": 0, "whole": [1, 2, 3], "core": [2, 3], "enh": 3}, [1, 2, 3])
    x = REF.smooth_logits(3, (12, 14, 16), seed=9)
    props = {'shape_after_cropping_and_before_resampling': (18, 20, 22), 'shape_before_cropping': (20, 24, 25),
             'bbox_used_for_cropping': [[1, 19], [2, 22], [3, 25]], 'spacing': (1.0, 1.0, 1.0)}
    seg = EX.convert_predicted_logits_to_segmentation_with_correct_shape(
        G(x), PlansManager({}), ConfigurationManager({'spacing': [1.5, 1.4, 1.4]}), lm, props)
    want = EX.resize_logits_to_segmentation(G(x), (18, 20, 22), (20, 24, 25), (1, 2, 3), regions_class_order=[1, 2, 3])
    assert torch.equal(seg, want) and int(seg.max()) == 3
    with pytest.raises(NotImplementedError):
        EX.resize_logits_to_segmentation(torch.zeros((9, 2, 2, 2), device=DEV), (2, 2, 2), (2, 2, 2), (0, 0, 0),
                                         regions_class_order=list(range(9)))
