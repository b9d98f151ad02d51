"""CPU tests of the host side of region-based training: trainer.LabelManager, ops.region_label_table and the
numpy model of ops.convert_seg_to_regions against tests/golden/label_manager.json, which records the reference's own
LabelManager and ConvertSegmentationToRegionsTransform (tools/make_golden.py regions).  Integer work: exact."""
import json
import os

import numpy as np
import pytest

import region_loss_ref as RR
from conftest import GOLDEN
from multimodal_mvd_seg_amd import ops
from multimodal_mvd_seg_amd.trainer import LabelManager, PlansManager

FIX = json.load(open(os.path.join(GOLDEN, "label_manager.json")))


def plain(v):
    if isinstance(v, (list, tuple)):
        return [plain(i) for i in v]
    return int(v) if isinstance(v, (int, np.integer)) else v


def label_dict(rec):
    return {k: (tuple(v) if rec["is_tuple"][k] else v) for k, v in rec["label_dict"].items()}


def test_fixture_is_reference_made_and_covers_the_modes():
    assert FIX["source"].startswith("reference ")
    ms = FIX["managers"]
    assert len(ms) >= 10
    assert any(m["has_regions"] and m["has_ignore_label"] for m in ms)
    assert any(not m["has_regions"] and m["has_ignore_label"] for m in ms)
    assert any(any(m["is_tuple"].values()) for m in ms) and any(m["has_regions"] and not any(m["is_tuple"].values()) for m in ms)
    assert any(m["has_regions"] and any(isinstance(r, list) and 0 in r for r in m["all_regions"]) for m in ms)
    assert len(FIX["convert_probabilities_to_segmentation"]) >= 4


@pytest.mark.parametrize("i", range(len(FIX["managers"])))
def test_label_manager_properties(i):
    rec = FIX["managers"][i]
    m = LabelManager(label_dict(rec), rec["regions_class_order"])
    assert m.has_regions == rec["has_regions"]
    assert m.has_ignore_label == rec["has_ignore_label"]
    assert m.ignore_label == rec["ignore_label"]
    assert plain(m.all_labels) == rec["all_labels"]
    assert (None if m.all_regions is None else plain(m.all_regions)) == rec["all_regions"]
    if rec["has_regions"]:
        assert plain(m.foreground_regions) == rec["foreground_regions"]
        # list entries become tuples, tuples stay (label_handling.py:93-94)
        assert all(isinstance(r, (tuple, int)) for r in m.all_regions)
    assert plain(m.foreground_labels) == rec["foreground_labels"]
    assert m.num_segmentation_heads == rec["num_segmentation_heads"]
    assert m.regions_class_order == rec["regions_class_order"]
    via_plans = PlansManager({}).get_label_manager({"labels": label_dict(rec), "regions_class_order": rec["regions_class_order"]})
    assert via_plans.num_segmentation_heads == rec["num_segmentation_heads"]


@pytest.mark.parametrize("i", range(len(FIX["rejected"])))
def test_label_manager_rejects_what_the_reference_rejects(i):
    rec = FIX["rejected"][i]
    with pytest.raises((AssertionError, RuntimeError)) as e:
        LabelManager(rec["label_dict"], rec["regions_class_order"])
    assert type(e.value).__name__ == rec["error"]


def test_filter_background():
    assert LabelManager.filter_background([0, 1, (0, 0), (0, 1), [0], 2]) == [1, (0, 1), 2]


@pytest.mark.parametrize("i", range(len(FIX["convert_probabilities_to_segmentation"])))
def test_overwrite_loop_model(i):
    rec = FIX["convert_probabilities_to_segmentation"][i]
    p = np.array(rec["probabilities"], dtype=np.float32)
    assert np.array_equal(RR.regions_to_segmentation(p, rec["regions_class_order"]), np.array(rec["segmentation"]))


@pytest.mark.parametrize("i", range(len(FIX["regions_transform"])))
def test_table_and_plane_model_equal_the_transform(i):
    rec = FIX["regions_transform"][i]
    seg = np.array(rec["seg"], dtype=np.float32)
    want = np.array(rec["planes"], dtype=np.float32)
    regions = rec["foreground_regions"]
    assert np.array_equal(RR.seg_to_regions(seg, regions, rec["ignore_label"]), want)
    # the table the kernels read: plane r of a voxel is bit r of table[label], the ignore plane bit 31
    lut = ops.region_label_table(regions, rec["ignore_label"])
    assert lut.dtype == np.uint32 and lut.shape == (256,)
    assert np.array_equal(lut, RR.label_table(regions, rec["ignore_label"]))
    bits = lut[seg[:, 0].astype(np.int64)]
    for r in range(len(regions)):
        assert np.array_equal(((bits >> r) & 1).astype(np.float32), want[:, r])
    if rec["ignore_label"] is not None:
        assert np.array_equal((bits >> 31).astype(np.float32), want[:, -1])
    else:
        assert not (lut >> 31).any()


def test_table_limits():
    with pytest.raises(NotImplementedError):
        ops.region_label_table([300])
    with pytest.raises(NotImplementedError):
        ops.region_label_table([1] * 32)


def test_losses_refuse_what_is_not_built():
    from multimodal_mvd_seg_amd import losses
    with pytest.raises(NotImplementedError, match="at most 8"):
        losses.DC_and_BCE_loss({}, {}, regions=[1, 2, 3, 4, 5, 6, 7, 8, 9])
    with pytest.raises(ValueError):
        losses.DC_and_BCE_loss({}, {}, use_ignore_label=True, regions=[1, 2])
    l = losses.DC_and_CE_loss({'batch_dice': False, 'smooth': 1e-5, 'do_bg': False, 'ddp': False}, {}, ignore_label=3)
    assert l.ignore_label == 3
    assert isinstance(losses.DC_and_BCE_loss({}, {}), losses._FusedDCCE)
