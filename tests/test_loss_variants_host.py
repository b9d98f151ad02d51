"""CPU tests of the loss trainer variants of DESIGN 29: the six classes exist, their _build_loss composes what
variants/loss/*.py composes (weights over every level, do_bg / smooth / ignore_index / k / label_smoothing), every refusal
says why, and the header declares the top-k entry points the binding calls.  Nothing here touches a GPU."""
import os
import re

import numpy as np
import pytest
import torch

import topk_ref as TR
from conftest import ROOT
from multimodal_mvd_seg_amd import _lib, losses, ops, trainer

CH = {"channel_names": {"0": "a", "1": "b"}}
PLAIN = dict(CH, labels={"background": 0, "a": 1, "b": 2, "c": 3})
IGNORE = dict(CH, labels={"background": 0, "a": 1, "b": 2, "c": 3, "ignore": 4})
REGIONS = dict(CH, labels={"background": 0, "whole": [1, 2, 3], "core": [2, 3], "enh": 3}, regions_class_order=[1, 2, 3])
REGIONS_IGNORE = dict(CH, labels={"background": 0, "whole": [1, 2, 3], "core": [2, 3], "enh": 3, "ignore": 4},
                      regions_class_order=[1, 2, 3])
STRIDES = [[1, 1, 1], [2, 2, 2], [2, 2, 2], [2, 2, 2]]


def make(name, dataset_json=PLAIN, patch=(32, 32, 32), strides=STRIDES, batch_dice=False, **kw):
    plans = trainer.make_plans(patch, strides, batch_size=2, base_features=8, max_features=32, batch_dice=batch_dice, **kw)
    cfg = kw.get("configuration", "3d_fullres")
    return getattr(trainer, name)(plans, cfg, 0, dataset_json, device=torch.device("cuda"))


def test_the_six_classes_exist_and_override_build_loss_alone():
    for name in TR.VARIANTS:
        cls = getattr(trainer, name)
        assert issubclass(cls, trainer.nnUNetTrainerMI355)
        own = {k for k in vars(cls) if not k.startswith("__")}
        assert own == {"_build_loss"}, (name, own)


@pytest.mark.parametrize("name", TR.VARIANTS)
def test_weights_cover_every_level(name):
    loss = make(name)._build_loss()
    assert isinstance(loss, losses.DeepSupervisionWrapper)
    w = np.asarray(loss.weight_factors)
    assert np.allclose(w, TR.variant_weights(3), rtol=0, atol=1e-15) and w[-1] > 0 and abs(w.sum() - 1) < 1e-15
    base = trainer.nnUNetTrainerMI355(trainer.make_plans((32, 32, 32), STRIDES), "3d_fullres", 0, PLAIN,
                                      device=torch.device("cuda"))._build_loss()
    assert base.weight_factors[-1] == 0     # the base trainer keeps its zeroed tail


def test_dice_trainer():
    l = make("nnUNetTrainerDiceLossMI355", batch_dice=True)._build_loss().loss
    assert type(l) is losses.MemoryEfficientSoftDiceLoss
    assert (l.batch_dice, l.do_bg, l.smooth, l.weight_ce, l.weight_dice) == (True, False, 1e-5, 0.0, 1.0)
    r = make("nnUNetTrainerDiceLossMI355", REGIONS)._build_loss().loss
    assert type(r) is losses.DC_and_BCE_loss        # sigmoid heads: do_bg = has_regions, no BCE term
    assert (r.batch_dice, r.do_bg, r.smooth, r.weight_ce, r.weight_dice, r.use_ignore_label) == (False, True, 1e-5, 0.0, 1.0, False)
    for dj in (IGNORE, REGIONS_IGNORE):
        with pytest.raises(NotImplementedError, match="no mask for the ignore label"):
            make("nnUNetTrainerDiceLossMI355", dj)._build_loss()


def test_no_smooth_trainer():
    l = make("nnUNetTrainerDiceCELoss_noSmoothMI355")._build_loss().loss
    assert type(l) is losses.DC_and_CE_loss and (l.smooth, l.do_bg, l.weight_ce, l.weight_dice, l.ignore_label) == (0, False, 1, 1, None)
    assert make("nnUNetTrainerDiceCELoss_noSmoothMI355", IGNORE)._build_loss().loss.ignore_label == 4
    r = make("nnUNetTrainerDiceCELoss_noSmoothMI355", REGIONS_IGNORE)._build_loss().loss
    assert type(r) is losses.DC_and_BCE_loss and (r.smooth, r.do_bg, r.use_ignore_label) == (0, True, True)


def test_ce_trainer():
    l = make("nnUNetTrainerCELossMI355")._build_loss().loss
    assert type(l) is losses.RobustCrossEntropyLoss and l.ignore_index == -100 and (l.weight_ce, l.weight_dice) == (1.0, 0.0)
    assert make("nnUNetTrainerCELossMI355", IGNORE)._build_loss().loss.ignore_index == 4
    assert losses.RobustCrossEntropyLoss().ignore_index == -100      # today's constructor call still works
    with pytest.raises(NotImplementedError, match="class weights"):
        losses.RobustCrossEntropyLoss(weight=torch.ones(4))


def test_topk_trainers():
    l = make("nnUNetTrainerTopk10LossMI355")._build_loss().loss
    assert type(l) is losses.TopKLoss and (l.k, l.label_smoothing, l.ignore_index) == (10, 0.0, -100)
    l = make("nnUNetTrainerTopk10LossLS01MI355", IGNORE)._build_loss().loss
    assert type(l) is losses.TopKLoss and (l.k, l.label_smoothing, l.ignore_index) == (10, 0.1, 4)
    l = make("nnUNetTrainerDiceTopK10LossMI355", IGNORE, batch_dice=True)._build_loss().loss
    assert type(l) is losses.DC_and_topk_loss
    assert (l.batch_dice, l.do_bg, l.smooth, l.weight_ce, l.weight_dice, l.ignore_label) == (True, False, 1e-5, 1.0, 1.0, 4)
    assert (l.ce.k, l.ce.label_smoothing, l.ce.ignore_index) == (10, 0.0, 4)
    assert make("nnUNetTrainerDiceTopK10LossMI355")._build_loss().loss.ce.ignore_index == -100
    with pytest.raises(NotImplementedError, match="class weights"):
        losses.TopKLoss(weight=torch.ones(4))
    with pytest.raises(ValueError, match="percentage"):
        losses.TopKLoss(k=0)
    d = losses.TopKLoss()
    assert (d.k, d.ignore_index, d.label_smoothing) == (10, -100, 0.0)


@pytest.mark.parametrize("name", ["nnUNetTrainerCELossMI355", "nnUNetTrainerTopk10LossMI355", "nnUNetTrainerTopk10LossLS01MI355",
                                  "nnUNetTrainerDiceTopK10LossMI355"])
def test_ce_and_topk_trainers_keep_the_regions_assertion(name):
    with pytest.raises(AssertionError, match="regions not supported by this trainer"):
        make(name, REGIONS)._build_loss()


@pytest.mark.parametrize("name", TR.VARIANTS)
def test_more_than_eight_heads_and_cascades_are_refused(name):
    many = dict(CH, labels=dict({"background": 0}, **{f"l{i}": i for i in range(1, 10)}))
    with pytest.raises(NotImplementedError, match="at most 8"):
        make(name, many)._build_loss()
    t = make(name)
    t.configuration_manager.configuration['previous_stage_name'] = '3d_lowres'
    with pytest.raises(NotImplementedError, match="cascade"):
        t._build_loss()


@pytest.mark.parametrize("name", ["nnUNetTrainerTopk10LossMI355", "nnUNetTrainerTopk10LossLS01MI355",
                                  "nnUNetTrainerDiceTopK10LossMI355"])
def test_k_zero_is_refused_with_a_message(name):
    # 4 x 4 x 4 under scales 1, 1/2, 1/4: the coarsest level has 1 voxel per sample, 2 at batch 2 -> k = int(2 * 10 / 100) = 0
    with pytest.raises(NotImplementedError, match=r"k = int\(2 \* 10 / 100\) = 0"):
        make(name, patch=(4, 4, 4))._build_loss()
    assert ops.topk_count(9, 10) == 0 and ops.topk_count(10, 10) == 1 and ops.topk_count(19, 10) == 1
    assert ops.topk_count(315, 10) == 31 and ops.topk_count(945, 10) == 94 and ops.topk_count(2 * 128 ** 3, 10) == 419430


def test_2d_plans_build_too():
    for name in TR.VARIANTS:
        t = make(name, patch=(32, 32), strides=[[1, 1], [2, 2], [2, 2]], configuration='2d')
        assert np.allclose(t._build_loss().weight_factors, TR.variant_weights(2))


def test_the_graph_key_needs_no_loss_flag():
    """The capture cache (_step_graph) belongs to one trainer instance, whose loss is built once by initialize(): two
    variants never share a captured graph, so _graph_flags stays the base trainer's."""
    for name in TR.VARIANTS:
        assert getattr(trainer, name)._graph_flags is trainer.nnUNetTrainerMI355._graph_flags


def test_header_declares_the_topk_entries_and_the_binding_matches():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvdseg_hip.h")).read(), flags=re.S)
    want = {"mvd_topk_workspace_bytes": 2, "mvd_topk_ce_fwd": 9, "mvd_topk_select": 7, "mvd_topk_finalize": 10, "mvd_topk_bwd": 16}
    for fn, n in want.items():
        m = re.search(r"\b(?:int|size_t)\s+" + fn + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, f"{fn} is not declared"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == n == len(_lib.SIGNATURES[fn][1]), fn
    mk = open(os.path.join(ROOT, "multimodal_mvd_seg_amd", "csrc", "Makefile")).read()
    assert "loss_topk.hip" in mk
    assert hasattr(ops, "DeepSupervisedTopKFn")


def test_host_wrapper_refuses_cpu_tensors():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        losses.TopKLoss()(torch.zeros(1, 2, 2, 2, 3), torch.zeros(1, 1, 2, 2, 3))
