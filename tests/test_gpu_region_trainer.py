"""GPU tests of nnUNetTrainerMI355 in the label modes of DESIGN 17: regions, the ignore label, and both.  The train step is
compared with the oracle network (oracle/unet_oracle.py) fed to tests/region_loss_ref.py; the graphed step with the eager
step bit for bit; validation_step and perform_actual_validation with numpy in every integer.  Bars: DESIGN 8 (loss 1e-5
relative, parameters after steps 1e-5)."""
import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

import export_ref as REF
import region_loss_ref as RR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
STRIDES = [[1, 1, 1], [2, 2, 2], [2, 2, 2], [2, 2, 2]]   # three deep-supervision levels: weights 4/6, 2/6 and 0
PATCH = (32, 32, 32)
CH = {"channel_names": {"0": "a", "1": "b"}}
MODES = {
    "regions": dict(CH, labels={"background": 0, "whole": [1, 2, 3], "core": [2, 3], "enh": 3}, regions_class_order=[1, 2, 3]),
    "regions+ignore": dict(CH, labels={"background": 0, "whole": [1, 2, 3], "core": [2, 3], "enh": 3, "ignore": 4},
                           regions_class_order=[1, 2, 3]),
    "ignore": dict(CH, labels={"background": 0, "a": 1, "b": 2, "c": 3, "ignore": 4}),
}
PLAIN = dict(CH, labels={"background": 0, "a": 1, "b": 2, "c": 3})
REGIONS = [(1, 2, 3), (2, 3), 3]
MARGIN, MAX_EXCLUDED = 1e-4, 1e-3


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from multimodal_mvd_seg_amd import _lib
    _lib.load()


def heads(mode):
    return 4 if mode in ("ignore", "plain") else 3


def make_trainer(mode, graph=False, batch_dice=False, spacing=None, tb=None):
    from multimodal_mvd_seg_amd import trainer
    plans = trainer.make_plans(PATCH, STRIDES, batch_size=2, base_features=8, max_features=32, batch_dice=batch_dice)
    if spacing is not None:
        plans['configurations']['3d_fullres']['spacing'] = spacing
    if tb is not None:
        plans['transpose_backward'] = tb
    tr = trainer.nnUNetTrainerMI355(plans, "3d_fullres", 0, MODES.get(mode, PLAIN), device=DEV)
    tr.use_hip_graph = graph
    torch.manual_seed(0)
    tr.initialize()
    return tr


def batch(mode, seed, nlab=None):
    """data + float label-map targets per deep-supervision level (the top one downsampled by picking voxels, as the feed
    does); labels 0..3 and, in the ignore modes, 4"""
    g = torch.Generator().manual_seed(seed)
    nlab = nlab or (5 if "ignore" in mode else 4)
    data = torch.rand((2, 2, *PATCH), generator=g)
    top = torch.randint(0, nlab, (2, 1, 8, 8, 8), generator=g).float()
    top = top.repeat_interleave(4, 2).repeat_interleave(4, 3).repeat_interleave(4, 4)
    return {'data': data, 'target': [top, top[:, :, ::2, ::2, ::2].contiguous(), top[:, :, ::4, ::4, ::4].contiguous()]}


def ref_loss_fn(mode, batch_dice):
    from oracle import loss_oracle as LO
    ign = 4 if "ignore" in mode else None
    if mode == "ignore":
        one = lambda o, t: RR.dc_and_ce_masked(o, t, ign, batch_dice=batch_dice)
    else:
        one = lambda o, t: RR.dc_and_bce_labelmap(o, t, REGIONS, ign, batch_dice=batch_dice)
    w = [float(x) for x in LO.ds_weights(3)]
    return lambda outs, tgts: RR.deep_supervised(one, outs, tgts, w)


@pytest.mark.parametrize("batch_dice", [False, True])
@pytest.mark.parametrize("mode", list(MODES))
def test_train_steps_match_the_oracle_network_and_restatement(mode, batch_dice):
    from oracle import step_oracle as SO, unet_oracle as UO
    tr = make_trainer(mode, batch_dice=batch_dice)
    assert tr.label_manager.num_segmentation_heads == heads(mode)
    ora = UO.build_plainconv_unet(2, heads(mode), 4, STRIDES, base=8, max_features=32, seed=0)
    tr.network.load_state_dict(ora.state_dict())
    tr.optimizer.fp.invalidate_packs()
    opt = SO.make_optimizer(ora.parameters())
    loss_fn = ref_loss_fn(mode, batch_dice)
    tr.on_train_epoch_start()
    for step in range(3):
        b = batch(mode, 10 + step)
        l_ref, _, _ = SO.train_step(ora, loss_fn, opt, b)
        l = float(tr.train_step(b)["loss"])
        lerr = abs(l - float(l_ref)) / abs(float(l_ref))
        ref_params = dict(ora.named_parameters())
        perr = max(float((p.detach().cpu() - ref_params[n].detach()).abs().max()) for n, p in tr.network.named_parameters())
        print(f"{mode} batch_dice={batch_dice} step {step}: loss {l:.7f} oracle {float(l_ref):.7f} rel {lerr:.2e}; "
              f"worst param err {perr:.2e}")
        assert lerr <= 1e-5, lerr
        if step in (0, 2):
            assert perr <= 1e-5, perr


@pytest.mark.parametrize("mode", list(MODES))
def test_graphed_step_equals_the_eager_step_bit_for_bit(mode):
    a, b = make_trainer(mode, graph=False), make_trainer(mode, graph=True)
    b.network.load_state_dict(a.network.state_dict())
    b.optimizer.fp.invalidate_packs()
    batches = [batch(mode, 30 + i) for i in range(7)]
    la = [np.asarray(a.train_step(x)["loss"]).copy() for x in batches]
    lb = [np.asarray(b.train_step(x)["loss"]).copy() for x in batches]
    torch.cuda.synchronize()
    assert b._step_graph is not None and b._step_graph["graph"] is not None, "the step was never captured"
    assert a._graph_flags() != make_trainer("plain")._graph_flags()
    for i, (x, y) in enumerate(zip(la, lb)):
        assert np.array_equal(x, y), f"loss of step {i}: eager {x} graph {y}"
    for (n, p), (_, q) in zip(a.network.named_parameters(), b.network.named_parameters()):
        assert torch.equal(p.detach(), q.detach()), n


@pytest.mark.parametrize("mode", list(MODES))
def test_validation_step_counts_equal_numpy(mode):
    tr = make_trainer(mode)
    with torch.no_grad():
        for head in tr.network.decoder.seg_layers:
            for p in head.parameters():
                p.mul_(40.0)
    tr.optimizer.fp.invalidate_packs()
    b = batch(mode, 40)
    out = tr.validation_step(b)
    with torch.no_grad():
        z = tr.network(b['data'].to(DEV))[0].cpu().numpy()
    t = b['target'][0].numpy()
    if mode == "ignore":
        want = RR.argmax_counts_masked(z, t, 4)[1:]
    else:
        ign = 4 if "ignore" in mode else None
        want = RR.sigmoid_counts(z, RR.seg_to_regions(t, REGIONS, ign), ign is not None)
    assert len(out['tp_hard']) == 3 and want[:, 0].sum() > 0
    assert np.array_equal(out['tp_hard'], want[:, 0]) and np.array_equal(out['fp_hard'], want[:, 1]) \
        and np.array_equal(out['fn_hard'], want[:, 2])
    assert np.isfinite(float(out['loss']))


def _case(seed, nlab, tb):
    rng = np.random.default_rng(seed)
    data = ndi.gaussian_filter(rng.standard_normal((2, 36, 44, 40)), (0, 2, 2, 2)).astype(np.float32) * 4
    props = {'shape_before_cropping': (50, 70, 61), 'bbox_used_for_cropping': [[3, 48], [0, 63], [5, 61]],
             'shape_after_cropping_and_before_resampling': (45, 63, 56), 'spacing': [2.5, 0.7, 0.7]}
    full_t = tuple(props['shape_before_cropping'][a] for a in tb)
    gt = ndi.zoom(rng.integers(0, nlab, size=(6, 7, 8)), [s / c for s, c in zip(full_t, (6, 7, 8))], order=0, mode='nearest',
                  grid_mode=True).astype(np.int16)
    return {'data': torch.from_numpy(data), 'properties': props, 'seg': gt[None]}


@pytest.mark.parametrize("mode", list(MODES))
def test_perform_actual_validation_equals_the_scipy_oracle_in_every_integer(mode):
    from multimodal_mvd_seg_amd.inference import SlidingWindowPredictor
    tb = [1, 2, 0]
    tr = make_trainer(mode, spacing=[3.2, 1.0, 1.0], tb=tb)
    with torch.no_grad():
        for head in tr.network.decoder.seg_layers:
            for p in head.parameters():
                p.mul_(40.0)
    tr.optimizer.fp.invalidate_packs()
    ign = 4 if "ignore" in mode else None
    cases = [_case(0, 5 if ign else 4, tb), _case(1, 5 if ign else 4, tb)]
    metrics, segs = tr.perform_actual_validation(cases, return_segmentations=True)
    labels = [1, 2, 3] if mode == "ignore" else REGIONS
    assert list(metrics['mean'].keys()) == labels
    tr.network.decoder.deep_supervision = False
    predictor = SlidingWindowPredictor(tr.network, PATCH, heads(mode), tile_step_size=0.5, use_gaussian=True,
                                       use_mirroring=True, allowed_mirroring_axes=(0, 1, 2), device=DEV)
    for case, seg, got in zip(cases, segs, metrics['metric_per_case']):
        logits = predictor.predict_sliding_window_return_logits(case['data']).cpu().numpy()
        p = case['properties']
        new, full, lo = p['shape_after_cropping_and_before_resampling'], p['shape_before_cropping'], \
            [v[0] for v in p['bbox_used_for_cropping']]
        if mode == "ignore":
            seg_ref, _, mar = REF.export(logits, new, full, lo, tb, separate_z_axis=0)
        else:
            res = REF.resample_logits(logits, new, 0)
            prob = torch.sigmoid(torch.from_numpy(res.astype(np.float32))).numpy()
            seg_ref = REF.paste_transpose(RR.regions_to_segmentation(prob, [1, 2, 3]).astype(np.uint8), full, lo, tb)
            mar = REF.paste_transpose(np.abs(res).min(0), full, lo, tb, fill=np.inf)
        seg = seg.cpu().numpy()
        low = mar < MARGIN
        assert float(low.mean()) <= MAX_EXCLUDED and np.array_equal(seg[~low], seg_ref[~low])
        seg_ref[low] = seg[low]
        assert len(np.unique(seg)) > 1, "a constant prediction would test nothing"
        ref = REF.counts(case['seg'][0], seg_ref, labels, ign)
        for r, row in zip(labels, ref):
            m = got['metrics'][r]
            assert [m['TP'], m['FP'], m['FN'], m['TN']] == row.tolist(), (r, m, row)
    tr.network.decoder.deep_supervision = True


class _DS:
    """label volumes with -1 (outside the mask), the region labels 1..3 and the ignore label 4"""

    def __init__(self, shapes, seed):
        rng = np.random.default_rng(seed)
        self.cases = {}
        for i, shp in enumerate(shapes):
            data = rng.standard_normal((2, *shp)).astype(np.float32)
            seg = np.zeros((1, *shp), dtype=np.int16)
            zz, yy, xx = np.meshgrid(*[np.arange(v) for v in shp], indexing='ij')
            for lab in (1, 2, 3):
                ctr = rng.integers(10, np.array(shp) - 10)
                seg[0][(zz - ctr[0]) ** 2 + (yy - ctr[1]) ** 2 + (xx - ctr[2]) ** 2 < 60] = lab
            seg[0, :, :, : shp[2] // 4] = 4
            seg[0, :2] = -1
            loc = {c: np.argwhere(seg == c) for c in (1, 2, 3)}
            loc[(0, 1, 2, 3)] = np.argwhere((seg >= 0) & (seg <= 3))
            self.cases[f"c{i}"] = (data, seg, {"class_locations": loc})

    def keys(self):
        return self.cases.keys()

    def load_case(self, k):
        return self.cases[k]


def test_device_loader_batches_train_and_plain_training_is_undisturbed():
    tr = make_trainer("regions+ignore", graph=True)
    tr.on_train_epoch_start()
    dl = tr.get_device_dataloader(_DS([(60, 64, 56), (58, 60, 70)], 8))
    np.random.seed(0)
    seen = set()
    for _ in range(5):
        b = next(dl)
        assert float(b["target"][0].min()) >= 0          # RemoveLabel: -1 -> 0 in the feed, untouched by this change
        seen |= set(np.unique(b["target"][0].cpu().numpy()).astype(int).tolist())
        assert np.isfinite(float(tr.train_step(b)["loss"]))
    assert 4 in seen and seen & {1, 2, 3}
    # after all of that a plain-label trainer's steps are bit-identical to those of a fresh plain-label trainer in a
    # process that has used the new modes before as well as after
    a, b = make_trainer("plain", graph=True), make_trainer("plain", graph=False)
    b.network.load_state_dict(a.network.state_dict())
    b.optimizer.fp.invalidate_packs()
    batches = [batch("plain", 60 + i) for i in range(6)]
    la = [np.asarray(a.train_step(x)["loss"]).copy() for x in batches]
    tr.train_step(next(dl))
    lb = [np.asarray(b.train_step(x)["loss"]).copy() for x in batches]
    assert all(np.array_equal(x, y) for x, y in zip(la, lb))
    for (n, p), (_, q) in zip(a.network.named_parameters(), b.network.named_parameters()):
        assert torch.equal(p.detach(), q.detach()), n


def test_what_is_still_refused_says_so():
    from multimodal_mvd_seg_amd import trainer
    plans = trainer.make_plans(PATCH, STRIDES, batch_size=2, base_features=8, max_features=32)
    for mode in MODES:
        with pytest.raises(NotImplementedError, match="softmax heads only"):
            trainer.ContrastiveTrainerMI355(plans, "3d_fullres", 0, MODES[mode], device=DEV)
    many = dict(CH, labels=dict({"background": 0, "ignore": 10}, **{f"l{i}": i for i in range(1, 10)}))
    with pytest.raises(NotImplementedError, match="at most 8"):
        trainer.nnUNetTrainerMI355(plans, "3d_fullres", 0, many, device=DEV).initialize()
    # the limit is the loss kernels': a plain-label network with more heads is still built (inference, export)
    pm = trainer.PlansManager(plans)
    plain10 = dict(CH, labels=dict({"background": 0}, **{f"l{i}": i for i in range(1, 10)}))
    net = trainer.get_network_from_plans(pm, plain10, pm.get_configuration("3d_fullres"), 2)
    assert net.decoder.seg_layers[-1].weight.shape[0] == 10
    plans['configurations']['3d_fullres']['previous_stage_name'] = '3d_lowres'
    with pytest.raises(NotImplementedError, match="cascade"):
        trainer.nnUNetTrainerMI355(plans, "3d_fullres", 0, MODES["regions"], device=DEV).initialize()
