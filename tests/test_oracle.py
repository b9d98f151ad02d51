"""CPU tests: the oracle (oracle/) against the committed golden fixtures (tests/golden/), including the ones
generated from reference modules (robust_ce, soft_skeleton, polylr, network_topology, C++ persistence)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, load_npz
from oracle import cc_oracle, loss_oracle as LO, step_oracle as SO, unet_oracle as UO


@pytest.fixture(scope="module", autouse=True)
def _four_threads():
    """The fixtures were generated with 4 intra-op threads (tools/make_golden.py) and the bit-exact checks depend on how
    the CPU reductions are split: hold 4 while this module runs, whatever a module run before it set."""
    n = torch.get_num_threads()
    torch.set_num_threads(4)
    yield
    torch.set_num_threads(n)


def T(a):
    return torch.from_numpy(np.asarray(a))


def test_robust_ce_reference_fixture():
    z = load_npz("robust_ce.npz")
    logits = T(z["logits"]).requires_grad_()
    l = LO.RobustCrossEntropyLoss()(logits, T(z["target"]))
    l.backward()
    assert torch.equal(l.detach(), T(z["loss"]))
    assert torch.equal(logits.grad, T(z["glogits"]))


@pytest.mark.parametrize("name", sorted(f for f in os.listdir(GOLDEN) if f.startswith("soft_skel_")))
def test_soft_skel_reference_fixture(name):
    z = load_npz(name)
    x = T(z["x"]).requires_grad_()
    y = LO.soft_skel(x, int(z["iter"]))
    assert torch.equal(y.detach(), T(z["skel"]))  # bit-exact: min/max/relu/sub/mul/add only
    y.backward(T(z["gy"]))
    assert torch.equal(x.grad, T(z["gx"]))
    assert torch.equal(LO.soft_erode(x.detach()), T(z["erode"]))
    assert torch.equal(LO.soft_dilate(x.detach()), T(z["dilate"]))


def test_polylr_reference_fixture():
    d = json.load(open(os.path.join(GOLDEN, "polylr.json")))
    for e, lr in enumerate(d["lrs"]):
        assert SO.poly_lr(d["initial_lr"], e, d["max_steps"]) == lr


def test_topology_reference_fixture():
    d = json.load(open(os.path.join(GOLDEN, "topology_props.json")))["props"]
    for cfg in ("cfg1", "cfg2", "cfg5"):
        assert d[cfg]["pool_op_kernel_sizes"] == UO.CONFIGS[cfg]["strides"]
        assert all(k == [3, 3, 3] for k in d[cfg]["conv_kernel_sizes"])
        assert len(d[cfg]["conv_kernel_sizes"]) == UO.CONFIGS[cfg]["n_stages"]
    # the author's patch 64x128x256 ends with a (1,2,2) pooling -> per-axis strides are a real requirement
    assert d["author"]["pool_op_kernel_sizes"][-1] == [1, 2, 2]


def test_he_init_reference_fixture():
    d = json.load(open(os.path.join(GOLDEN, "he_init_stats.json")))["stats"]
    torch.manual_seed(0)
    net = UO.build_plainconv_unet(4, 5, 3, [[1, 1, 1], [2, 2, 2], [2, 2, 2]], seed=0)
    for m in net.modules():
        if isinstance(m, (torch.nn.Conv3d, torch.nn.ConvTranspose3d)):
            assert float(m.bias.abs().max()) == 0.0
    for name, st in d.items():
        assert abs(st["std"] - st["expected_std"]) / st["expected_std"] < 0.15
        assert st["bias_abs_max"] == 0.0


def test_param_counts_match_survey():
    n1 = UO.build_plainconv_unet(1, 5, 5, UO.CONFIGS["cfg1"]["strides"])
    n2 = UO.build_plainconv_unet(4, 5, 6, UO.CONFIGS["cfg2"]["strides"])
    c1 = sum(p.numel() for p in n1.parameters())
    c2 = sum(p.numel() for p in n2.parameters())
    assert abs(c1 - 16.55e6) < 0.02e6 and abs(c2 - 31.20e6) < 0.02e6
    keys = set(n2.state_dict().keys())
    for k in ("encoder.stages.0.0.convs.0.conv.weight", "encoder.stages.0.0.convs.0.all_modules.0.weight",
              "encoder.stages.5.0.convs.1.norm.bias", "decoder.encoder.stages.0.0.convs.0.conv.weight",
              "decoder.stages.0.convs.0.conv.weight", "decoder.transpconvs.4.weight", "decoder.seg_layers.4.bias"):
        assert k in keys, k


@pytest.mark.parametrize("name", ["distill_kl_c5_T1.npz", "distill_kl_c5_T4.npz", "distill_kl_c1_T1.npz",
                                  "distill_kl_c1_T4.npz"])
def test_distill_kl_fixture(name):
    z = load_npz(name)
    ys, yt = T(z["ys"]).requires_grad_(), T(z["yt"]).requires_grad_()
    l = LO.distill_kl(ys, yt, int(z["T"]))
    l.backward()
    assert torch.allclose(l.detach(), T(z["loss"]), rtol=1e-6, atol=0)
    assert torch.allclose(ys.grad, T(z["gys"]), rtol=1e-5, atol=1e-9)


def test_dc_ce_fixture_and_dice_counts():
    for bd in (0, 1):
        z = load_npz(f"dc_ce_batchdice{bd}.npz")
        logits = T(z["logits"]).requires_grad_()
        l = LO.build_loss(1, batch_dice=bool(bd), deep_supervision=False)(logits, T(z["target"]))
        l.backward()
        assert torch.allclose(l.detach(), T(z["loss"]), rtol=1e-6)
        assert torch.allclose(logits.grad, T(z["glogits"]), rtol=1e-5, atol=1e-9)
        tp, fp, fn = LO.validation_counts(logits.detach(), T(z["target"]))
        assert np.array_equal(tp, z["tp"]) and np.array_equal(fp, z["fp"]) and np.array_equal(fn, z["fn"])
        assert abs(LO.dice_from_counts(tp, fp, fn)[1] - float(z["dice_mean"])) < 1e-12


def test_ds_weights():
    assert np.allclose(LO.ds_weights(5), [0.53333333, 0.26666667, 0.13333333, 0.06666667, 0.0])
    assert np.allclose(LO.ds_weights(4), [0.57142857, 0.28571429, 0.14285714, 0.0])


def test_unet_tiny_step_fixture():
    """Round 3: the fixture is produced by the REFERENCE's train_step / configure_optimizers (nnUNetTrainer.py:888-925,
    :473-477) and decoder forward (UNetDecoder.py:1001-1027) executed on a stub trainer (tools/make_golden.py::
    _RefStepHarness); the oracle restatement must reproduce all three steps bit for bit."""
    z = load_npz("unet_tiny_step.npz")
    src = str(z["source"])
    assert src.startswith("reference training/nnUNetTrainer/nnUNetTrainer.py:888") and "UNetDecoder.py:1001" in src \
        and "nnUNetTrainer.py:473" in src, src
    strides = z["strides"].tolist()
    net = UO.build_plainconv_unet(2, int(z["num_classes"]), 3, strides, features_per_stage=z["features"].tolist())
    net.load_state_dict({k[4:]: T(z[k]) for k in z.files if k.startswith("sd0/")})
    batch = {"data": T(z["data"]), "target": [T(z[f"target{i}"]) for i in range(2)]}
    ref = SO.synthetic_batch(2, 2, (16, 16, 16), strides, num_classes=3, seed=1234)
    assert torch.equal(ref["data"], batch["data"]) and torch.equal(ref["target"][1], batch["target"][1])
    loss_fn = LO.build_loss(2)
    opt = SO.make_optimizer(net.parameters())
    for step in range(3):
        l, logits, gn = SO.train_step(net, loss_fn, opt, batch)
        assert l.dtype == np.float32 and np.array_equal(l, z[f"loss{step}"]), (step, l, z[f"loss{step}"])
        assert gn == float(z[f"gradnorm{step}"])
        if step == 0:
            for i, lg in enumerate(logits):
                assert torch.equal(lg, T(z[f"logits{i}"]))
            for n, p in net.named_parameters():
                assert torch.equal(p.grad, T(z["grad0/" + n])), n
        if step in (0, 2):
            for n, p in net.named_parameters():
                assert torch.equal(p.detach(), T(z[f"sd{step + 1}/" + n])), (step, n)


def test_decoder_forward_reference_fixture():
    """UNetDecoder_return_last_fea.forward (UNetDecoder.py:1001-1027: plain decoder, attn_skip = skips[-1]) executed
    on the fixture's skips; unet_oracle.UNetDecoder.forward reproduces logits (DS on: list + last feature; DS off: bare
    tensor) exactly."""
    z = load_npz("decoder_forward.npz")
    assert str(z["source"]).startswith("reference training/my_network/UNetDecoder.py:1001"), z["source"]
    strides = z["strides"].tolist()
    net = UO.build_plainconv_unet(2, int(z["num_classes"]), 3, strides, features_per_stage=z["features"].tolist())
    net.decoder.load_state_dict({k[3:]: T(z[k]) for k in z.files if k.startswith("sd/")}, strict=False)
    skips = [T(z[f"skip{i}"]) for i in range(3)]
    with torch.no_grad():
        out, feat = net.decoder(skips, True)
        assert isinstance(out, list) and len(out) == 2
        for i, lg in enumerate(out):
            assert torch.equal(lg, T(z[f"logits{i}"]))
        assert torch.equal(feat, T(z["feat"]))
        net.decoder.deep_supervision = False
        off = net.decoder(skips)
        assert torch.is_tensor(off) and torch.equal(off, T(z["logits_ds_off"]))


def test_ds_scales_and_optimizer_reference_fixture():
    """nnUNetTrainer._get_deep_supervision_scales (:296-302) and configure_optimizers (:473-477), executed."""
    d = json.load(open(os.path.join(GOLDEN, "ds_scales.json")))
    assert d["source"].startswith("reference training/nnUNetTrainer/nnUNetTrainer.py:296")
    for c in d["cases"]:
        got = SO.ds_scales(c["pool_op_kernel_sizes"])
        assert [list(map(float, i)) for i in got] == c["scales"]
    o = d["optimizer"]
    opt = SO.make_optimizer([torch.nn.Parameter(torch.zeros(1))])
    g0 = opt.param_groups[0]
    assert type(opt).__name__ == o["class"] and {k: g0[k] for k in o["hyper"]} == o["hyper"]
    assert [SO.poly_lr(o["hyper"]["lr"], e, o["num_epochs"]) for e in range(o["num_epochs"])] == o["lrs"]


def test_ddp_split_fixture():
    d = json.load(open(os.path.join(GOLDEN, "ddp_split.json")))["cases"]
    for key, v in d.items():
        gb, ws = map(int, key.split("_"))
        bs, ov = SO.ddp_batch_split(gb, ws)
        assert bs == v["batch_sizes"] and np.allclose(ov, v["oversample"])
        if gb % ws == 0:  # (the reference's remainder rule can go negative for odd splits; mirrored, not fixed)
            assert sum(bs) == gb


def _sorted_pairs(b, d):
    a = np.stack([b, d], 1)
    return a[np.lexsort((a[:, 1], a[:, 0]))]


def test_persistence_reference_fixture():
    """oracle/cc_oracle.c against diagrams produced by the reference's own C++ (hom.cpp / cohom.cpp)."""
    d = json.load(open(os.path.join(GOLDEN, "persistence_grid.json")))
    for case in d["cases"]:
        f = np.asarray(case["f"], dtype=np.float32).reshape(case["shape"])
        b, de, _ = cc_oracle.h0_persistence(f, case["conn"])
        want = np.array([[x, np.inf if y is None else y] for x, y in case["dgm0_sorted"]], dtype=np.float32)
        assert np.array_equal(_sorted_pairs(b, de), want)
    # the survey's known answer on the 5-vertex line: (0,inf),(0.5,3),(1,2),(2,2),(3,3)
    last = d["cases"][-1]["dgm0_sorted"]
    assert [tuple(p) for p in last] == [(0.0, None), (0.5, 3.0), (1.0, 2.0), (2.0, 2.0), (3.0, 3.0)]


def test_cc_label_fixture():
    d = json.load(open(os.path.join(GOLDEN, "cc_label.json")))
    for case in d["cases"]:
        mask = np.asarray(case["mask"], dtype=np.uint8).reshape(case["shape"])
        labels, n = cc_oracle.cc_label(mask, case["conn"])
        assert n == case["count"]
        assert np.array_equal(labels.reshape(-1), np.asarray(case["labels"], dtype=np.int32))


def test_cc_label_edge_cases():
    for shape in ((1, 1, 1), (1, 1, 7), (3, 1, 2)):
        for fill in (0, 1):
            m = np.full(shape, fill, dtype=np.uint8)
            labels, n = cc_oracle.cc_label(m, 6)
            assert n == fill and labels.max() == fill
    # count == number of essential H0 bars of the masked sub-level set
    rng = np.random.default_rng(3)
    f = rng.random((5, 6, 7)).astype(np.float32)
    _, death, _ = cc_oracle.h0_persistence(f, 6)
    assert int(np.isinf(death).sum()) == 1


def test_oracle_against_live_reference_modules():
    """What the reference's soft_skeleton, robust_ce_loss and network_initialization modules returned on these inputs
    (tests/golden/reference_modules.npz, written by tools/make_golden.py): the oracle reproduces it bit for bit."""
    z = load_npz("reference_modules.npz")
    assert str(z["source"]).startswith("reference ")
    x = T(z["x"])
    for it in (0, 2, 5):
        assert torch.equal(T(z[f"skel_iter{it}"]), LO.soft_skel(x, it))
    assert torch.equal(T(z["ce_loss"]), LO.RobustCrossEntropyLoss()(T(z["logits"]), T(z["target"])))
    torch.manual_seed(int(z["he_seed"]))
    b = torch.nn.Conv3d(4, 8, 3)
    b.apply(UO.InitWeights_He(1e-2))
    assert torch.equal(T(z["he_weight"]), b.weight)


def test_ref_extension_if_built():
    """The diagram the reference's C++ (hom.cpp, compiled into oracle/_ref by oracle/build_ref.py) produced on a 3x4x5
    grid with ties (tests/golden/ref_persistence_3x4x5.npz) equals the C oracle's; where oracle/_ref is built, the
    extension still produces it."""
    from oracle import build_ref
    fx = load_npz("ref_persistence_3x4x5.npz")
    assert str(fx["source"]).startswith("reference C++")
    f, want = fx["f"], fx["dgm0"]
    D, H, W = f.shape
    b, de, _ = cc_oracle.h0_persistence(f, 6)
    assert np.array_equal(want[np.lexsort((want[:, 1], want[:, 0]))], _sorted_pairs(b, de))
    m = build_ref.load()
    if m is None:
        return
    s = m.SimplicialComplex()
    for i in range(D * H * W):
        s.append([i])
    for z in range(D):
        for y in range(H):
            for x in range(W):
                for dz, dy, dx in ((0, 0, 1), (0, 1, 0), (1, 0, 0)):
                    if z + dz < D and y + dy < H and x + dx < W:
                        s.append([(z * H + y) * W + x, ((z + dz) * H + y + dy) * W + x + dx])
    s.initialize()
    s.extendFloat(torch.from_numpy(f.reshape(-1).copy()))
    dgm = m.persistenceForwardHom(s, 0, 0)[0].detach().numpy()
    b, de, _ = cc_oracle.h0_persistence(f, 6)
    assert np.array_equal(dgm[np.lexsort((dgm[:, 1], dgm[:, 0]))], _sorted_pairs(b, de))


def test_sliding_window_steps_known_answer_and_gaussian_map():
    """sliding_window_prediction.py:37-38 states the expected placement for (image 110, patch 64, step 0.5); the host
    Gaussian map (numpy, separable) must equal the scipy.ndimage.gaussian_filter construction the reference uses."""
    import importlib.util
    from oracle import infer_oracle as IO
    assert IO.compute_steps_for_sliding_window((110,), (64,), 0.5) == [[0, 23, 46]]
    assert IO.compute_steps_for_sliding_window((64, 70, 128), (64, 64, 64), 0.5) == [[0], [0, 6], [0, 32, 64]]
    src = open(os.path.join(os.path.dirname(__file__), "..", "multimodal_mvd_seg_amd", "inference.py")).read()
    ns = {}
    exec(compile(src.replace("from ._lib import call", "call = None"), "inference.py", "exec"), ns)  # host logic only
    for ts in [(8, 8, 8), (16, 12, 20), (5, 7, 9), (64, 64, 64)]:
        a = ns["compute_gaussian"](ts, 1. / 8, 1000.0)
        b = IO.compute_gaussian(ts, 1. / 8, 1000.0).numpy()
        assert np.abs(a - b).max() <= 1e-6 * b.max(), ts
        assert ns["compute_steps_for_sliding_window"](ts, tuple(max(2, t // 2) for t in ts), 0.5) == \
            IO.compute_steps_for_sliding_window(ts, tuple(max(2, t // 2) for t in ts), 0.5)
    img = torch.arange(2 * 3 * 4 * 5, dtype=torch.float32).reshape(2, 3, 4, 5)
    padded, revert = IO.pad_to_patch(img, (8, 4, 7))
    assert tuple(padded.shape) == (2, 8, 4, 7) and torch.equal(padded[revert], img)


def _blob_seg(rng, shape, thr=0.55):
    """Smooth random field -> multi-label segmentation with blobs of very different sizes."""
    from scipy import ndimage
    f = ndimage.gaussian_filter(rng.random(shape), 1.5)
    f = (f - f.min()) / (f.max() - f.min())
    seg = np.zeros(shape, dtype=np.int32)
    seg[f > thr] = 1
    seg[f > thr + 0.12] = 2
    seg[f < 0.25] = 3
    return seg


def test_cc_oracle_partition_matches_scipy_label():
    # independent pin of oracle/cc_oracle.c: same partition (and component count) as scipy.ndimage.label
    from scipy import ndimage
    rng = np.random.default_rng(11)
    for conn, rank in ((6, 1), (26, 3)):
        for p in (0.2, 0.45):
            m = rng.random((9, 11, 13)) < p
            labels, n = cc_oracle.cc_label(m, conn)
            ref, n_ref = ndimage.label(m, structure=ndimage.generate_binary_structure(3, rank))
            assert n == n_ref
            # a bijection between the two label sets, foreground only
            pairs = np.unique(np.stack([labels[m], ref[m]]), axis=1)
            assert pairs.shape[1] == n and len(set(pairs[0])) == n and len(set(pairs[1])) == n
            # canonical label = 1 + smallest linear index of the component
            flat = labels.reshape(-1)
            for l in np.unique(flat[flat > 0]):
                assert l == 1 + np.flatnonzero(flat == l)[0]


def test_postproc_oracle_known_answer():
    from oracle import postproc_oracle as PO
    seg = np.zeros((4, 6, 8), dtype=np.int32)
    seg[0, 0, 0:5] = 1          # 5 voxels
    seg[2, 2:4, 2:6] = 2        # 8 voxels (label 2, also in the set)
    seg[3, 5, 7] = 1            # 1 voxel  -> removed
    seg[0, 4:6, 6:8] = 1        # 4 voxels -> removed
    seg[1, 5, 0] = 3            # not in the label set: untouched
    out = PO.remove_all_but_largest_component_from_segmentation(seg, [1, 2], background_label=0)
    exp = seg.copy()
    exp[3, 5, 7] = 0
    exp[0, 4:6, 6:8] = 0
    assert np.array_equal(out, exp)
    out1 = PO.remove_all_but_largest_component_from_segmentation(seg, (1, 2), background_label=7, num_components=1)
    exp1 = exp.copy()
    exp1[0, 0, 0:5] = 7
    exp1[3, 5, 7] = 7
    exp1[0, 4:6, 6:8] = 7
    assert np.array_equal(out1, exp1)
    # diagonal touch joins under 26-connectivity only
    d = np.zeros((2, 2, 2), dtype=np.int32)
    d[0, 0, 0] = d[1, 1, 1] = 1
    m26, s26 = PO.remove_all_but_n_largest_component(d > 0, 1, 26)
    m6, s6 = PO.remove_all_but_n_largest_component(d > 0, 1, 6)
    assert s26 == [2] and s6 == [1] and m6[0, 0, 0] and not m6[1, 1, 1]
    # input is not modified, empty mask is a no-op
    z = np.zeros((3, 3, 3), dtype=np.int32)
    assert np.array_equal(PO.remove_all_but_largest_component_from_segmentation(z, 1), z)


def test_feed_oracle_resize_index_and_crop_pad_known_answer():
    from scipy import ndimage
    from oracle import feed_oracle as FO
    # closed-form order-0 index (what the HIP kernel computes) == scipy.ndimage.zoom(grid_mode=True), the call
    # skimage.transform.resize(order=0) makes
    for n, m in ((128, 64), (128, 32), (128, 16), (128, 8), (160, 80), (160, 10), (20, 10), (12, 5), (7, 3), (9, 4), (5, 5)):
        z = ndimage.zoom(np.arange(n, dtype=float), m / n, order=0, mode='nearest', grid_mode=True)
        assert np.array_equal(z, FO.nn_index(np.arange(m), n, m)), (n, m)
    rng = np.random.default_rng(0)
    t = rng.integers(0, 5, (2, 1, 8, 12, 16)).astype(np.float32)
    for scale in (0.5, 0.25, (1, 0.5, 0.5)):
        ref = FO.downsample_seg(t, scale)
        sc = [scale] * 3 if not isinstance(scale, tuple) else scale
        idx = [FO.nn_index(np.arange(int(round(t.shape[2 + i] * sc[i]))), t.shape[2 + i], int(round(t.shape[2 + i] * sc[i])))
               for i in range(3)]
        assert np.array_equal(ref, t[:, :, idx[0]][:, :, :, idx[1]][:, :, :, :, idx[2]])
    assert FO.downsample_seg(t, 1) is t
    # crop + pad: a box hanging over the low side of z and the high side of x
    vol = np.arange(2 * 3 * 4 * 5, dtype=np.float32).reshape(2, 3, 4, 5)
    out = FO.crop_pad(vol, [-1, 1, 3], (3, 2, 4), 0)
    assert out.shape == (2, 3, 2, 4)
    assert np.all(out[:, 0] == 0) and np.all(out[:, :, :, 2:] == 0)
    assert np.array_equal(out[:, 1:, :, :2], vol[:, 0:2, 1:3, 3:5])
    seg = np.ones((1, 3, 4, 5), dtype=np.int16)
    s = FO.crop_pad(seg, [-1, 1, 3], (3, 2, 4), -1)
    assert s.dtype == np.int16 and (s == -1).sum() == 24 - 2 * 2 * 2 and FO.remove_label(s).min() == 0
    assert np.array_equal(FO.mirror(vol, 0b101), vol[:, ::-1, :, ::-1])


def test_reference_extracted_fixtures_are_reference_sourced_and_the_oracle_matches_them():
    """distill_kl / l2_loss (other_loss.py:51-78), the per-rank batch split (nnUNetTrainer.py:304-349), the sliding-window
    placement + Gaussian map (sliding_window_prediction.py:10-56): fixtures generated by the reference function bodies
    themselves (tools/make_golden.py::ref_function); the oracle restatements must reproduce them exactly."""
    from oracle import infer_oracle as IO
    for name in ("distill_kl_c5_T1", "distill_kl_c5_T4", "distill_kl_c1_T1", "distill_kl_c1_T4"):
        z = load_npz(name + ".npz")
        assert str(z["source"]).startswith("reference nnUNet") or str(z["source"]).startswith("reference training/"), z["source"]
        ys, yt = T(z["ys"]).requires_grad_(), T(z["yt"]).requires_grad_()
        l = LO.distill_kl(ys, yt, int(z["T"]))
        l.backward()
        assert torch.equal(l.detach(), T(z["loss"])) and torch.equal(ys.grad, T(z["gys"])) and torch.equal(yt.grad, T(z["gyt"]))
    for name in ("feat_kl_T1", "feat_kl_T4"):
        z = load_npz(name + ".npz")
        assert str(z["source"]).startswith("reference ")
        a, b = T(z["a"]).requires_grad_(), T(z["b"]).requires_grad_()
        l = LO.l2_loss(a, b, True, int(z["T"]))
        l.backward()
        assert torch.equal(l.detach(), T(z["loss"])) and torch.equal(a.grad, T(z["ga"])) and torch.equal(b.grad, T(z["gb"]))
    z = load_npz("l2_loss_plain.npz")
    assert str(z["source"]).startswith("reference ")
    a, b = T(z["a"]).requires_grad_(), T(z["b"]).requires_grad_()
    l = LO.l2_loss(a, b, False)
    l.backward()
    assert torch.equal(l.detach(), T(z["loss"])) and torch.equal(a.grad, T(z["ga"])) and torch.equal(b.grad, T(z["gb"]))
    assert json.load(open(os.path.join(GOLDEN, "ddp_split.json")))["source"].startswith("reference ")
    d = json.load(open(os.path.join(GOLDEN, "sw_steps.json")))
    for c in d["steps"]:
        assert IO.compute_steps_for_sliding_window(c["image_size"], c["tile_size"], c["tile_step_size"]) == c["steps"]
    for c in d["gaussian"]:
        g = IO.compute_gaussian(tuple(c["tile_size"]), c["sigma_scale"], c["value_scaling_factor"]).numpy()
        assert np.abs(g.reshape(-1) - np.array(c["map"])).max() <= 1e-6 * max(c["map"])
