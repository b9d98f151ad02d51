"""GPU tests of the segmentation export and evaluation tail (csrc/export.hip, export.py, evaluation.py,
nnUNetTrainerMI355.perform_actual_validation) against the fp64 scipy restatement in export_ref.py.

Tolerances.  Logits are Gaussian-smoothed noise of std 8 clipped to +-64.  Three fp32 lerps of |logit| <= 64 err by at
most about 2.3e-5 in the logit; softmax's derivative is at most 1/4 and its own fp32 rounding is below 1e-6, hence
1e-5 on probabilities.  Two channels off by 2.3e-5 each cannot swap order when the oracle's top-2 margin (fp64, after
resampling) is at least 1e-4, so labels must be EQUAL on every such voxel; the voxels left out may be at most 1e-3 of
the volume, which is asserted too (the oracle alone leaves about 2.5e-5 of this input under the margin).
"""
import itertools

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

import export_ref as REF
from multimodal_mvd_seg_amd import evaluation as EV
from multimodal_mvd_seg_amd import export as EX

DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu

PROB_TOL = 1e-5
LOGIT_TOL = 2.3e-5
MARGIN = 1e-4
MAX_EXCLUDED = 1e-3


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from multimodal_mvd_seg_amd import _lib
    _lib.load()


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def check_labels(seg, seg_ref, mar, what=""):
    low = mar < MARGIN
    share = float(low.mean())
    mism = int(((seg != seg_ref) & ~low).sum())
    print(f"{what}: voxels {seg.size}, under the margin {share:.2e}, mismatches above it {mism}, "
          f"mismatches in all {int((seg != seg_ref).sum())}")
    assert share <= MAX_EXCLUDED, share
    assert mism == 0, mism


# shape in, shape out, separate-z axis, pre-crop volume, bbox corner, transpose_backward
CASES = [
    ((37, 45, 52), (61, 83, 70), None, (61, 83, 70), (0, 0, 0), (0, 1, 2)),      # upsample, odd sizes
    ((37, 45, 52), (20, 31, 40), None, (23, 40, 41), (2, 5, 1), (0, 1, 2)),      # downsample, inside a larger volume
    ((37, 45, 52), (37, 60, 52), None, (37, 60, 52), (0, 0, 0), (0, 1, 2)),      # two axes unchanged
    ((37, 45, 52), (61, 83, 70), 0, (61, 83, 70), (0, 0, 0), (0, 1, 2)),         # each separate-z axis
    ((37, 45, 52), (61, 83, 70), 1, (61, 83, 70), (0, 0, 0), (0, 1, 2)),
    ((37, 45, 52), (61, 83, 70), 2, (66, 85, 77), (3, 1, 7), (2, 0, 1)),
    ((37, 45, 52), (30, 83, 52), 0, (30, 83, 52), (0, 0, 0), (1, 2, 0)),         # separate z, downsampled out of plane
]


@pytest.mark.parametrize("shape,new,axis,full,lo,tb", CASES)
def test_resized_probabilities_and_labels_match_the_scipy_oracle(shape, new, axis, full, lo, tb):
    x = REF.smooth_logits(5, shape, seed=0)
    seg_ref, prob_ref, mar = REF.export(x, new, full, lo, tb, axis)
    seg, prob = EX.resize_logits_to_segmentation(G(x), new, full, lo, tb, axis, return_probabilities=True)
    assert seg.dtype == torch.uint8 and tuple(seg.shape) == seg_ref.shape and tuple(prob.shape) == prob_ref.shape
    seg, prob = seg.cpu().numpy(), prob.cpu().numpy()
    err = float(np.abs(prob.astype(np.float64) - prob_ref).max())
    print(f"{shape}->{new} sep-z {axis}: max |p - p_oracle| = {err:.3e}")
    assert np.isfinite(prob).all() and err <= PROB_TOL, err
    check_labels(seg, seg_ref, mar, f"{shape}->{new} sep-z {axis}")


@pytest.mark.parametrize("axis_spacing", [((1.0, 1.0, 1.0), None), ((3.1, 1.0, 1.0), 0), ((1.0, 1.0, 3.5), 2)])
def test_resample_data_or_seg_to_shape_matches_the_oracle(axis_spacing):
    spacing, axis = axis_spacing
    x = REF.smooth_logits(3, (21, 30, 17), seed=4)
    new = (33, 25, 17)
    got = EX.resample_data_or_seg_to_shape(G(x), new, spacing, (1.0, 1.0, 1.0)).cpu().numpy()
    ref = REF.resample_logits(x, new, axis)
    err = float(np.abs(got - ref).max())
    print(f"resample {spacing}: max |logit - oracle| = {err:.3e}")
    assert got.shape == ref.shape and err <= LOGIT_TOL, err
    same = EX.resample_data_or_seg_to_shape(G(x), x.shape[1:], spacing, spacing)
    assert torch.equal(same.cpu(), torch.from_numpy(x))


# ------------------------------------------------------------------------------------------------ exact cases
def test_equal_shape_is_a_plain_argmax():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((7, 19, 23, 29)).astype(np.float32)
    seg = EX.resize_logits_to_segmentation(G(x), x.shape[1:], x.shape[1:], (0, 0, 0))
    assert np.array_equal(seg.cpu().numpy(), x.argmax(0).astype(np.uint8))


def test_integer_upsampling_of_blockwise_constant_integer_logits_is_exact():
    """Upsampling by 2 has the weights 1/4 and 3/4 and the logits are small integers, constant on 2x2x2 blocks with a
    distinct winner per block: every fp32 operation is exact, so the labels equal the fp64 oracle's argmax everywhere,
    ties between interpolated blocks included."""
    rng = np.random.default_rng(2)
    K, blocks = 6, (5, 6, 7)
    coarse = rng.integers(-8, 9, size=(K, *blocks)).astype(np.float32)
    winner = rng.integers(0, K, size=blocks)
    np.put_along_axis(coarse, winner[None], 16.0, axis=0)
    x = coarse.repeat(2, 1).repeat(2, 2).repeat(2, 3)
    new = tuple(2 * s for s in x.shape[1:])
    ref = REF.resample_logits(x, new)
    seg = EX.resize_logits_to_segmentation(G(x), new, new, (0, 0, 0)).cpu().numpy()
    assert np.array_equal(seg, ref.argmax(0).astype(np.uint8))
    inner = tuple(slice(1, None, 4) for _ in range(3))       # output voxels whose taps stay inside one block
    assert np.array_equal(seg[inner], winner)
    logits = EX.resample_data_or_seg_to_shape(G(x), new, (1, 1, 1), (1, 1, 1)).cpu().numpy()
    assert np.array_equal(logits.astype(np.float64), ref)


def test_exact_ties_choose_the_lowest_index():
    x = REF.smooth_logits(1, (9, 10, 11), seed=5)[0]
    stack = np.stack([x - 1, x, x, x - 2, x]).astype(np.float32)     # channels 1, 2 and 4 tie everywhere
    for new in ((9, 10, 11), (14, 17, 13)):
        seg = EX.resize_logits_to_segmentation(G(stack), new, new, (0, 0, 0)).cpu().numpy()
        assert (seg == 1).all()
    zeros = torch.zeros((4, 6, 6, 6), device=DEV)
    assert not EX.resize_logits_to_segmentation(zeros, (9, 9, 9), (9, 9, 9), (0, 0, 0)).any()


@pytest.mark.parametrize("lo", [(0, 0, 0), (4, 0, 0), (0, 6, 0), (0, 0, 5), (4, 6, 5), (2, 3, 1)])
def test_outside_the_bbox_is_zero_and_the_bbox_may_touch_every_face(lo):
    rng = np.random.default_rng(6)
    x = rng.standard_normal((3, 8, 9, 10)).astype(np.float32)
    x[0] -= 10                                                        # label 0 never wins inside
    new, full = (11, 13, 14), (15, 19, 19)
    res = REF.resample_logits(x, new)
    seg, prob = EX.resize_logits_to_segmentation(G(x), new, full, lo, return_probabilities=True)
    seg, prob = seg.cpu().numpy(), prob.cpu().numpy()
    inside = np.zeros(full, bool)
    inside[tuple(slice(l, l + n) for l, n in zip(lo, new))] = True
    assert (seg[inside] > 0).all() and not seg[~inside].any()
    check_labels(seg[inside].reshape(new), res.argmax(0).astype(np.uint8), REF.margin(res), f"bbox at {lo}")
    assert (prob[0][~inside] == 1).all() and not prob[1:][:, ~inside].any()


def test_every_transpose_backward_equals_the_identity_result_transposed():
    x = REF.smooth_logits(4, (10, 13, 17), seed=7)
    new, full, lo = (15, 21, 19), (18, 22, 23), (1, 0, 4)
    seg0, prob0 = EX.resize_logits_to_segmentation(G(x), new, full, lo, (0, 1, 2), return_probabilities=True)
    seg0, prob0 = seg0.cpu().numpy(), prob0.cpu().numpy()
    for tb in itertools.permutations(range(3)):
        seg, prob = EX.resize_logits_to_segmentation(G(x), new, full, lo, tb, return_probabilities=True)
        assert seg.is_contiguous() and np.array_equal(seg.cpu().numpy(), seg0.transpose(tb)), tb
        assert np.array_equal(prob.cpu().numpy(), prob0.transpose([0] + [a + 1 for a in tb])), tb


def test_launch_shape_does_not_change_the_result_and_bad_arguments_are_refused():
    x = G(REF.smooth_logits(3, (12, 9, 14), seed=8))
    a = EX.resize_logits_to_segmentation(x, (19, 14, 23), (19, 14, 23), (0, 0, 0))
    b = EX.resize_logits_to_segmentation(x, (19, 14, 23), (19, 14, 23), (0, 0, 0))
    assert torch.equal(a, b)
    with pytest.raises(ValueError):
        EX.resize_logits_to_segmentation(x, (19, 14, 23), (19, 14, 23), (1, 0, 0))
    with pytest.raises(ValueError):
        EX.resize_logits_to_segmentation(x, (19, 14, 23), (19, 14, 23), (0, 0, 0), (0, 1, 1))
    with pytest.raises(NotImplementedError):
        EX.resize_logits_to_segmentation(torch.zeros((256, 2, 2, 2), device=DEV), (2, 2, 2), (2, 2, 2), (0, 0, 0))


# ------------------------------------------------------------------------------------------------ confusion counts
def _label_volumes(shape, seed, gt_dtype):
    rng = np.random.default_rng(seed)
    gt = ndi.zoom(rng.integers(0, 6, size=[max(1, s // 6) for s in shape]), [s / max(1, s // 6) for s in shape], order=0,
                  mode='nearest', grid_mode=True)[:shape[0], :shape[1], :shape[2]]
    gt = np.ascontiguousarray(gt).astype(gt_dtype)
    assert gt.shape == tuple(shape)
    pred = gt.astype(np.uint8)
    flip = rng.random(shape) < 0.2
    pred[flip] = rng.integers(0, 6, size=int(flip.sum())).astype(np.uint8)
    gt[rng.random(shape) < 0.05] = 7                                  # the ignore label
    return gt, pred


@pytest.mark.parametrize("gt_dtype", [np.uint8, np.int16])
@pytest.mark.parametrize("ignore", [None, 7])
@pytest.mark.parametrize("shape", [(13, 17, 19), (32, 32, 32), (3, 5, 1)])
def test_confusion_counts_are_bit_exact_against_numpy(gt_dtype, ignore, shape):
    gt, pred = _label_volumes(shape, 11, gt_dtype)
    if gt_dtype == np.int16:
        gt[0, 0, 0] = -1                                              # a negative label belongs to no set
    # single labels, unions, a label absent from both volumes (9), more sets than one pass holds
    sets = [1, 2, (1, 2), 9, (3, 4, 5), 0, (0, 7), 5, (9, 10)]
    ref = REF.counts(gt, pred, sets, ignore)
    got = EV.confusion_counts(G(gt), G(pred), sets, ignore).cpu().numpy()
    assert got.dtype == np.int64 and np.array_equal(got, ref), (got, ref)
    nvalid = gt.size if ignore is None else int((gt != ignore).sum())
    assert (got.sum(1) == nvalid).all()
    assert np.array_equal(EV.confusion_counts(G(gt), G(pred), [3], ignore).cpu().numpy(), REF.counts(gt, pred, [3], ignore))
    m = EV.compute_metrics(G(gt), G(pred), sets, ignore)['metrics']
    assert np.isnan(m[9]['Dice']) and m[1]['TP'] == int(ref[0, 0]) and m[(1, 2)]['n_ref'] == int(ref[2, 0] + ref[2, 2])


def test_confusion_counts_repeat_bit_identically_and_masks_count_like_the_reference():
    gt, pred = _label_volumes((40, 50, 61), 12, np.int16)
    g, p = G(gt), G(pred)
    first = EV.confusion_counts(g, p, [1, 2, 3, 4, 5], 7)
    for _ in range(11):
        assert torch.equal(EV.confusion_counts(g, p, [1, 2, 3, 4, 5], 7), first)
    assert np.array_equal(first.cpu().numpy(), REF.counts(gt, pred, [1, 2, 3, 4, 5], 7))
    tp, fp, fn, tn = EV.compute_tp_fp_fn_tn(G(gt == 2), G(pred == 2), G(gt == 7))
    assert [tp, fp, fn, tn] == REF.counts(gt, pred, [2], 7)[0].tolist()
    assert list(EV.compute_tp_fp_fn_tn(G(gt == 2), G(pred == 2))) == REF.counts(gt, pred, [2])[0].tolist()


def test_confusion_counts_of_a_full_volume():
    gt, pred = _label_volumes((192, 256, 256), 13, np.uint8)
    got = EV.confusion_counts(G(gt), G(pred), [1, 2, 3, 4, 5], 7).cpu().numpy()
    assert (got.sum(1) == int((gt != 7).sum())).all()
    assert np.array_equal(got, REF.counts(gt, pred, [1, 2, 3, 4, 5], 7))


# ------------------------------------------------------------------------------------------------ end to end
STRIDES = [[1, 1, 1], [2, 2, 2], [2, 2, 2]]
DS = {"channel_names": {str(i): f"m{i}" for i in range(2)}, "labels": {"background": 0, "a": 1, "b": 2, "c": 3}}
TB = [1, 2, 0]


def _trainer(graph):
    from multimodal_mvd_seg_amd import trainer
    plans = trainer.make_plans((32, 32, 32), STRIDES, batch_size=2, base_features=8, max_features=32)
    plans['transpose_forward'], plans['transpose_backward'] = [2, 0, 1], TB
    plans['configurations']['3d_fullres']['spacing'] = [3.2, 1.0, 1.0]      # anisotropic: axis 0 is resampled on its own
    tr = trainer.nnUNetTrainerMI355(plans, "3d_fullres", 0, DS, device=DEV)
    tr.use_hip_graph = graph
    torch.manual_seed(0)
    tr.initialize()
    with torch.no_grad():                 # an untrained head gives near-equal logits; spread them as a trained one does
        for head in tr.network.decoder.seg_layers:
            for p in head.parameters():
                p.mul_(40.0)
    tr.optimizer.fp.invalidate_packs()
    return tr


def _case(seed=0):
    rng = np.random.default_rng(seed)
    data = ndi.gaussian_filter(rng.standard_normal((2, 36, 44, 40)), (0, 2, 2, 2)).astype(np.float32) * 4
    props = {'shape_before_cropping': (50, 70, 61), 'bbox_used_for_cropping': [[3, 48], [0, 63], [5, 61]],
             'shape_after_cropping_and_before_resampling': (45, 63, 56), 'spacing': [2.5, 0.7, 0.7]}
    full_t = tuple(props['shape_before_cropping'][a] for a in TB)
    gt = ndi.zoom(rng.integers(0, 4, size=(6, 7, 8)), [s / c for s, c in zip(full_t, (6, 7, 8))], order=0, mode='nearest',
                  grid_mode=True).astype(np.int16)
    assert gt.shape == full_t
    return {'data': torch.from_numpy(data), 'properties': props, 'seg': gt[None]}


@pytest.mark.parametrize("graph", [False, True])
def test_perform_actual_validation_end_to_end_and_training_is_undisturbed(graph):
    from multimodal_mvd_seg_amd.inference import SlidingWindowPredictor
    a, b = _trainer(graph), _trainer(graph)
    b.network.load_state_dict(a.network.state_dict())
    b.optimizer.fp.invalidate_packs()
    batches = [a.make_dummy_batch(seed=50 + i) for i in range(7)]
    la = [np.asarray(a.train_step(x)["loss"]).copy() for x in batches[:5]]
    lb = [np.asarray(b.train_step(x)["loss"]).copy() for x in batches[:5]]
    assert all(np.array_equal(x, y) for x, y in zip(la, lb))

    cases = [_case(0), _case(1)]
    assert a.enable_deep_supervision and a.network.decoder.deep_supervision and a.network.training
    metrics, segs = a.perform_actual_validation(cases, return_segmentations=True)
    assert a.network.decoder.deep_supervision is True and a.enable_deep_supervision and a.network.training
    assert set(metrics) == {'metric_per_case', 'mean', 'foreground_mean'} and len(metrics['metric_per_case']) == 2

    # the oracle: the same predictor's logits -> scipy export -> numpy counts
    a.network.decoder.deep_supervision = False
    predictor = SlidingWindowPredictor(a.network, (32, 32, 32), 4, tile_step_size=0.5, use_gaussian=True,
                                       use_mirroring=True, allowed_mirroring_axes=(0, 1, 2), device=DEV)
    labels = [1, 2, 3]
    for case, seg, got in zip(cases, segs, metrics['metric_per_case']):
        logits = predictor.predict_sliding_window_return_logits(case['data']).cpu().numpy()
        p = case['properties']
        seg_ref, _, mar = REF.export(logits, p['shape_after_cropping_and_before_resampling'], p['shape_before_cropping'],
                                     [v[0] for v in p['bbox_used_for_cropping']], TB, separate_z_axis=0)
        seg = seg.cpu().numpy()
        assert seg.shape == seg_ref.shape == case['seg'].shape[1:]
        check_labels(seg, seg_ref, mar, "end to end")
        low = mar < MARGIN                       # excluded from both sides: both take the device's label there
        seg_ref[low] = seg[low]
        ref = REF.counts(case['seg'][0], seg_ref, labels)
        for r, row in zip(labels, ref):
            m = got['metrics'][r]
            assert [m['TP'], m['FP'], m['FN'], m['TN']] == row.tolist(), (r, m, row)
            assert m['n_pred'] == row[0] + row[1] and m['n_ref'] == row[0] + row[2]
            assert m['Dice'] == 2 * row[0] / (2 * row[0] + row[1] + row[2])
        assert len(np.unique(seg)) > 1, "a constant prediction would test nothing"
    a.network.decoder.deep_supervision = True
    assert metrics['foreground_mean']['Dice'] == pytest.approx(
        np.mean([np.nanmean([c['metrics'][r]['Dice'] for c in metrics['metric_per_case']]) for r in labels]))

    # the next train steps do not notice the validation in between
    la = [np.asarray(a.train_step(x)["loss"]).copy() for x in batches[5:]]
    lb = [np.asarray(b.train_step(x)["loss"]).copy() for x in batches[5:]]
    torch.cuda.synchronize()
    assert all(np.array_equal(x, y) for x, y in zip(la, lb)), (la, lb)
    for (n, p), (_, q) in zip(a.network.named_parameters(), b.network.named_parameters()):
        assert torch.equal(p.detach(), q.detach()), n
    if graph:
        assert a._step_graph is not None and a._step_graph["graph"] is not None


def test_convert_predicted_logits_reads_the_plans_and_properties():
    from multimodal_mvd_seg_amd import trainer
    plans = trainer.make_plans((32, 32, 32), STRIDES)
    plans['transpose_backward'] = TB
    plans['configurations']['3d_fullres']['spacing'] = [3.2, 1.0, 1.0]
    pm = trainer.PlansManager(plans)
    cm, lm = pm.get_configuration('3d_fullres'), pm.get_label_manager(DS)
    case = _case(2)
    p = case['properties']
    x = REF.smooth_logits(4, (36, 44, 40), seed=9)
    seg, prob = EX.convert_predicted_logits_to_segmentation_with_correct_shape(G(x), pm, cm, lm, p,
                                                                               return_probabilities=True)
    seg_ref, prob_ref, mar = REF.export(x, p['shape_after_cropping_and_before_resampling'], p['shape_before_cropping'],
                                        [v[0] for v in p['bbox_used_for_cropping']], TB, separate_z_axis=0)
    check_labels(seg.cpu().numpy(), seg_ref, mar, "convert")
    assert float(np.abs(prob.cpu().numpy() - prob_ref).max()) <= PROB_TOL
    # a non-contiguous view, as the predictor returns for an image smaller than the patch
    big = torch.zeros((4, 40, 48, 44), device=DEV)
    big[:, 2:38, 1:45, 3:43] = G(x)
    seg2 = EX.convert_predicted_logits_to_segmentation_with_correct_shape(big[:, 2:38, 1:45, 3:43], pm, cm, lm, p)
    assert torch.equal(seg2, seg)


# ------------------------------------------------------------------------------------------------ full size
def test_full_size_volume_on_a_strided_subsample():
    """5 x 192x256x256 -> 288x384x384.  The oracle is evaluated at every fourth voxel per axis (1/64 of the volume) with
    map_coordinates(order=1, mode='nearest') at the coordinates zoom(grid_mode=True) uses (test_export_host checks that
    the two agree), so that the host side stays under a minute."""
    K, shape, new = 5, (192, 256, 256), (288, 384, 384)
    rng = np.random.default_rng(0)
    x = np.stack([ndi.gaussian_filter(rng.standard_normal(shape, dtype=np.float32), 2.0, mode='nearest') for _ in range(K)])
    x = np.clip(x / x.std() * 8.0, -64, 64).astype(np.float32)
    seg = EX.resize_logits_to_segmentation(G(x), new, new, (0, 0, 0)).cpu().numpy()
    sub = [np.arange(1, n, 4) for n in new]
    coords = np.array(np.meshgrid(*[(float(i) / n) * (s + 0.5) - 0.5 for s, i, n in zip(sub, shape, new)], indexing='ij'))
    res = np.stack([ndi.map_coordinates(c.astype(np.float64), coords, order=1, mode='nearest') for c in x])
    seg_ref = REF.softmax_f32(res).argmax(0).astype(np.uint8)
    check_labels(seg[np.ix_(*sub)], seg_ref, REF.margin(res), "full size")
    assert seg.shape == new and seg.max() == K - 1
