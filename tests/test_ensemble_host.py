"""CPU tests of the ensembling path (multimodal_mvd_seg_amd/ensembling.py): the numpy oracle against the fixture
written by the reference's own average_probabilities / convert_logits_to_segmentation (tools/make_golden.py ensemble),
every refusal that can be raised without a device, and the case bookkeeping of ensemble_crossvalidations."""
import numpy as np
import pytest
import torch

import ensemble_ref as EREF
from conftest import load_npz
from multimodal_mvd_seg_amd import ensembling as ENS
from multimodal_mvd_seg_amd import trainer
from multimodal_mvd_seg_amd.inference import SlidingWindowPredictor

PLAIN = trainer.LabelManager({"background": 0, "a": 1, "b": 2})
REGIONS = trainer.LabelManager({"background": 0, "whole": [1, 2, 3], "core": [2, 3], "enh": 3}, [1, 2, 3])


def test_oracle_equals_the_reference_fixture():
    z = load_npz("ensemble.npz")
    probs = list(z["probabilities"])
    assert len(probs) == 3 and probs[0].shape == (3, 6, 7, 9) and probs[0].dtype == np.float32
    seg, mean = EREF.merge(probs)
    assert mean.dtype == np.float32 and np.array_equal(mean.view(np.uint32), z["mean"].view(np.uint32))
    assert np.array_equal(seg, z["segmentation"])
    # member 0 stored as float16: raised to fp32 first (ensemble.py:24-25)
    seg, mean = EREF.merge([z["first_f16"]] + probs[1:])
    assert mean.dtype == np.float32 and np.array_equal(mean.view(np.uint32), z["mean_f16first"].view(np.uint32))
    assert np.array_equal(seg, z["segmentation_f16first"])
    assert not np.array_equal(z["mean"], z["mean_f16first"])
    # the inputs are left alone
    assert np.array_equal(np.stack(probs), z["probabilities"])


def test_fp64_oracle_is_consistent_with_the_single_model_export_oracle():
    import export_ref as REF
    x = REF.smooth_logits(3, (6, 7, 5), seed=1, std=2.0)
    seg, mean, mar, inside = EREF.ensemble([x], (9, 8, 7), (11, 9, 10), (1, 0, 2), (2, 0, 1))
    seg1, prob1, _ = REF.export(x, (9, 8, 7), (11, 9, 10), (1, 0, 2), (2, 0, 1))
    assert np.array_equal(seg, seg1) and np.abs(mean - prob1).max() < 1e-6
    assert np.isinf(mar[~inside]).all() and (mean[0][~inside] == 1).all() and not seg[~inside].any()
    assert np.allclose(mean.sum(0), 1)


def _cpu(K, n=1, shape=(2, 3, 4)):
    return [torch.zeros((K, *shape)) for _ in range(n)]


def test_refusals_that_need_no_device():
    with pytest.raises(NotImplementedError, match="region"):
        ENS.merge_probabilities(_cpu(3, 2), REGIONS)
    with pytest.raises(NotImplementedError, match="region"):
        ENS.ensemble_predictions([], None, REGIONS, {})
    with pytest.raises(NotImplementedError, match="region"):
        ENS.ensemble_crossvalidations([{}], REGIONS)
    with pytest.raises(NotImplementedError, match="9 heads"):
        ENS.average_probabilities(_cpu(9, 2))
    with pytest.raises(NotImplementedError, match="9 heads"):
        ENS.ensemble_logits_to_segmentation(_cpu(9, 2), (2, 3, 4), (2, 3, 4), (0, 0, 0))
    with pytest.raises(NotImplementedError, match="9 members"):
        ENS.average_probabilities(_cpu(3, 9))
    with pytest.raises(NotImplementedError, match="9 members"):
        ENS.ensemble_logits_to_segmentation(_cpu(3, 9), (2, 3, 4), (2, 3, 4), (0, 0, 0))
    with pytest.raises(NotImplementedError, match="uint16"):
        ENS.average_probabilities(_cpu(256, 2, (1, 1, 1)))
    with pytest.raises(ValueError, match="K differ"):
        ENS.average_probabilities(_cpu(3) + _cpu(4))
    with pytest.raises(ValueError, match="K differ"):
        ENS.ensemble_logits_to_segmentation(_cpu(3) + _cpu(4), (2, 3, 4), (2, 3, 4), (0, 0, 0))
    with pytest.raises(ValueError, match="shape"):
        ENS.average_probabilities(_cpu(3) + _cpu(3, 1, (2, 3, 5)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ENS.average_probabilities(_cpu(3, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ENS.merge_probabilities([np.zeros((3, 2, 2, 2), np.float32)], PLAIN)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ENS.ensemble_logits_to_segmentation(_cpu(3, 2), (2, 3, 4), (2, 3, 4), (0, 0, 0))
    with pytest.raises(AssertionError):
        ENS.average_probabilities([])
    with pytest.raises(ValueError):
        ENS.ensemble_logits_to_segmentation([], (2, 3, 4), (2, 3, 4), (0, 0, 0))


def test_ensemble_predictions_checks_members_against_the_label_manager_before_it_needs_a_device():
    plans = trainer.make_plans((32, 32, 32), [[1, 1, 1], [2, 2, 2]], spacing=(1.0, 1.0, 1.0))
    pm = trainer.PlansManager(plans)
    cm = pm.get_configuration('3d_fullres')
    props = {'shape_before_cropping': (4, 5, 6), 'bbox_used_for_cropping': [[0, 4], [0, 5], [0, 6]],
             'shape_after_cropping_and_before_resampling': (4, 5, 6), 'spacing': [1.0, 1.0, 1.0]}
    with pytest.raises(ValueError, match="K differ"):
        ENS.ensemble_predictions([(torch.zeros(3, 2, 3, 4), cm), (torch.zeros(4, 2, 3, 4), cm)], pm, PLAIN, props)
    with pytest.raises(NotImplementedError, match="9 members"):
        ENS.ensemble_predictions([(torch.zeros(3, 2, 3, 4), cm)] * 9, pm, PLAIN, props)
    many = trainer.LabelManager({"background": 0, **{f"l{i}": i for i in range(1, 9)}})
    with pytest.raises(NotImplementedError, match="9 heads"):
        ENS.ensemble_predictions([(torch.zeros(9, 2, 3, 4), cm)], pm, many, props)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ENS.ensemble_predictions([(torch.zeros(3, 2, 3, 4), cm)], pm, PLAIN, props)
    bad = dict(props, bbox_used_for_cropping=[[0, 4], [0, 5], [0, 5]])
    with pytest.raises(ValueError, match="does not span"):
        ENS.ensemble_predictions([(torch.zeros(3, 2, 3, 4), cm)], pm, PLAIN, bad)
    cubic = trainer.PlansManager(trainer.make_plans((32, 32, 32), [[1, 1, 1]], spacing=(1.0, 1.0, 1.0)))
    cubic.plans['configurations']['3d_fullres']['resampling_fn_probabilities_kwargs'] = {'order': 3}
    with pytest.raises(NotImplementedError, match="order=3"):
        ENS.ensemble_predictions([(torch.zeros(3, 2, 3, 4), cubic.get_configuration('3d_fullres'))], pm, PLAIN, props)


def test_crossvalidation_bookkeeping_missing_and_duplicate_cases():
    p = torch.zeros(3, 2, 2, 2)
    with pytest.raises(RuntimeError, match="model 1 does not seem to contain all predictions.*case_b"):
        ENS.ensemble_crossvalidations([{"case_a": p, "case_b": p}, {"case_a": p}], PLAIN)
    with pytest.raises(RuntimeError, match="model 0 does not seem to contain all predictions.*case_c"):
        ENS.ensemble_crossvalidations([[{"case_a": p}, {"case_b": p}], [{"case_a": p, "case_c": p}, {"case_b": p}]], PLAIN)
    with pytest.raises(AssertionError, match="Duplicate detected. Case case_a .* model 1"):
        ENS.ensemble_crossvalidations([[{"case_a": p}, {"case_b": p}], [{"case_a": p}, {"case_a": p, "case_b": p}]], PLAIN)
    with pytest.raises(RuntimeError, match="fold without predictions"):
        ENS.ensemble_crossvalidations([[{"case_a": p}, {}]], PLAIN)
    with pytest.raises(ValueError):
        ENS.ensemble_crossvalidations([], PLAIN)
    with pytest.raises(NotImplementedError, match="9 models"):
        ENS.ensemble_crossvalidations([{"case_a": p}] * 9, PLAIN)
    # complete and duplicate-free bookkeeping reaches the merge, which needs the device
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ENS.ensemble_crossvalidations([[{"case_a": p}, {"case_b": p}], {"case_b": p, "case_a": p}], PLAIN)


def test_predictor_takes_a_list_of_parameters():
    net = torch.nn.Identity()
    a = SlidingWindowPredictor(net, (8, 8, 8), 2, list_of_parameters=[{}, {}])
    assert len(a.list_of_parameters) == 2 and hasattr(a, "predict_logits_from_preprocessed_data")
    assert SlidingWindowPredictor(net, (8, 8, 8), 2).list_of_parameters is None
    with pytest.raises(ValueError, match="empty"):
        SlidingWindowPredictor(net, (8, 8, 8), 2, list_of_parameters=[])


def test_package_exports_the_module():
    import multimodal_mvd_seg_amd as pkg
    assert pkg.ensembling is ENS and "ensembling" in pkg.__all__
