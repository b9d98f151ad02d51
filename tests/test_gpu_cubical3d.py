"""GPU tests of the 3-D cubical persistence loss (csrc/cubical3d.hip): the device keys + sort + host sweep against the
union-find restatement (itself held to the brute-force cubical complex in tests/test_cubical3d_host.py), the target's point
count against scipy.ndimage.label, the fused loss against the fp64 assignment problem, its gradient against fp64 torch on
the same pairing, run-to-run bit identity, and one eager trainer step with topo_term = 'cubical'."""
import functools

import numpy as np
import pytest
import torch

import cubical3d_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SHAPES = [(3, 4, 5), (4, 4, 4), (2, 5, 3), (1, 4, 4), (5, 3, 1), (6, 7, 9), (16, 24, 40)]
LOSS_SHAPES = [(4, 4, 4), (3, 4, 5), (6, 7, 9)]


@functools.lru_cache(maxsize=None)
def _case(shape, dim, levels):
    """(f [2,D,H,W] float32, restatement rows per sample); computed once, never modified"""
    f = np.stack([R.field(shape, 21 + sum(shape), levels), R.field(shape, 22 + sum(shape), levels)])
    f.setflags(write=False)
    return f, [R.restatement_rows(f[n], dim) for n in range(2)]


def _mask(shape, seed, density):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.float32)


def _ops():
    from multimodal_mvd_seg_amd import ops
    return ops


@pytest.mark.parametrize("levels", [None, 6])
@pytest.mark.parametrize("dim", [0, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_device_bars_equal_the_restatement(shape, dim, levels):
    f, want = _case(shape, dim, levels)
    got = _ops().cubical3d_persistence(torch.from_numpy(f.copy()).to(DEV), dim)
    assert len(got) == 2
    for n in range(2):
        g = got[n].cpu().numpy()
        assert g.dtype == np.int32 and g.ndim == 2 and g.shape[1] == 2
        flat = f[n].reshape(-1)
        if levels is None:
            assert g.tolist() == [list(r) for r in want[n]]               # tie free: the rows themselves
        else:
            assert R.multiset(R.rows_to_bars(f[n], g)) == R.multiset(R.rows_to_bars(f[n], want[n]))
        assert g.min(initial=0) >= 0 and g.max(initial=0) < flat.size
        assert (flat[g[:, 1]] > flat[g[:, 0]]).all()                       # the gather invariant: b < d, both from the field


@pytest.mark.parametrize("shape", [(6, 7, 9), (1, 1, 7)])
@pytest.mark.parametrize("levels", [None, 6])
def test_dimension_0_equals_the_26_connected_h0_pairing(shape, levels):
    """the one key kernel through both of its entry points: the dimension-0 rows are the finite bars of non-zero length of
    ops.h0_persistence(conn 26, sublevel)"""
    ops = _ops()
    x = torch.from_numpy(R.field(shape, 100 + 7 * sum(shape), levels)).to(DEV)
    rows = ops.cubical3d_persistence(x[None], 0)[0].cpu().numpy()
    rows = rows[np.argsort(rows[:, 0], kind="stable")]
    birth, death, dv = (t.numpy() for t in ops.h0_persistence(x, 26, True))
    keep = (dv >= 0) & (death > birth)
    want = np.stack([np.nonzero(keep)[0], dv[keep]], 1).astype(np.int32)
    assert rows.dtype == want.dtype and np.array_equal(rows, want)
    if shape == (6, 7, 9) and levels is None:
        assert len(rows) >= 20


@pytest.mark.parametrize("dim", [0, 2])
def test_constant_field_and_negative_zero(dim):
    ops = _ops()
    got = ops.cubical3d_persistence(torch.full((2, 4, 5, 6), 0.25, device=DEV), dim)
    assert [tuple(g.shape) for g in got] == [(0, 2), (0, 2)]
    # +0 and -0 are one value: a field of signed zeros is constant, and inside a field they tie like equal values
    z = torch.zeros(1, 4, 5, 6)
    z.view(-1)[::3] = -0.0
    assert ops.cubical3d_persistence(z.to(DEV), dim)[0].shape[0] == 0
    f = R.field((4, 5, 6), 9, 6)
    f[f == f.flat[7]] = 0.0
    f.reshape(-1)[::2] *= -1.0                                             # every second zero becomes -0.0, the rest flips sign
    assert np.signbit(f[f == 0]).any() and not np.signbit(f[f == 0]).all()
    g = ops.cubical3d_persistence(torch.from_numpy(f[None]).to(DEV), dim)[0].cpu().numpy()
    assert g.tolist() == [list(r) for r in R.restatement_rows(f, dim)]
    with pytest.raises(ValueError, match="NaN"):
        ops.cubical3d_persistence(torch.full((1, 2, 2, 2), float("nan"), device=DEV), dim)


@pytest.mark.parametrize("dim", [0, 2])
def test_target_counts_equal_scipy_label(dim):
    ops = _ops()
    for shape in [(6, 7, 9), (1, 6, 6), (16, 24, 40)]:
        masks = [_mask(shape, 3 + i, d) for i, d in enumerate((0.1, 0.5, 0.9))] + [np.zeros(shape, np.float32),
                                                                                    np.ones(shape, np.float32)]
        m = ops.cubical3d_target_count(torch.from_numpy(np.stack(masks)).to(DEV), dim).cpu().numpy()
        want = [R.target_m(x, dim) for x in masks]
        assert m.dtype == np.int32 and m.tolist() == want
        assert want[3] == 0 and want[4] == 0
    if dim == 2:   # the border rule: one enclosed voxel counts, the same voxel moved onto a face does not
        x = np.zeros((2, 4, 4, 4), np.float32)
        x[0, 1, 2, 2] = x[1, 0, 2, 2] = 1
        assert ops.cubical3d_target_count(torch.from_numpy(x).to(DEV), 2).tolist() == [1, 0]


@pytest.mark.parametrize("q", [1, 2, 3])
@pytest.mark.parametrize("dim", [0, 2])
@pytest.mark.parametrize("shape", LOSS_SHAPES)
def test_loss_equals_the_fp64_assignment_problem(shape, dim, q):
    from multimodal_mvd_seg_amd import losses
    f, rows = _case(shape, dim, None)
    masks = np.stack([_mask(shape, 40, 0.5), _mask(shape, 41, 0.15 if dim == 2 else 0.85)])
    ms = [R.target_m(x, dim) for x in masks]
    want = R.loss_lsa([R.rows_to_bars(f[n].astype(np.float64), rows[n]) for n in range(2)], ms, q)
    layer = losses.CubicalWassersteinLoss(dim, q)
    got = float(layer(torch.from_numpy(f.copy()).to(DEV), torch.from_numpy(masks).to(DEV)))
    print(f"shape {shape} dim {dim} q {q}: bars {[len(r) for r in rows]} m {ms} W {got:.9g} lsa {want:.9g}")
    assert layer.last_m.tolist() == ms
    assert abs(got - want) <= 1e-6 * max(1.0, abs(want))


def test_loss_with_more_target_points_than_bars_and_with_none():
    from multimodal_mvd_seg_amd import losses
    shape = (4, 5, 6)
    const = torch.full((1,) + shape, 0.3, device=DEV)                      # no bars at all
    mask = np.zeros((1,) + shape, np.float32)
    mask[0, 1, 1, 1] = mask[0, 2, 3, 3] = 1
    for q in (1, 2):
        got = float(losses.CubicalWassersteinLoss(2, q)(const, torch.from_numpy(mask).to(DEV)))
        assert abs(got - (2 * 0.5 ** q) ** (1 / q)) <= 1e-6
        assert float(losses.CubicalWassersteinLoss(2, q)(const, torch.zeros_like(const))) == 0.0


@pytest.mark.parametrize("q", [1, 2, 3])
@pytest.mark.parametrize("dim", [0, 2])
def test_gradient_equals_fp64_torch_on_the_same_pairing(dim, q):
    from multimodal_mvd_seg_amd import losses, ops
    shape = (6, 7, 9)
    f, rows = _case(shape, dim, None)
    masks = np.stack([_mask(shape, 40, 0.5), _mask(shape, 41, 0.15 if dim == 2 else 0.85)])
    x = torch.from_numpy(f.copy()).to(DEV).requires_grad_(True)
    layer = losses.CubicalWassersteinLoss(dim, q)
    loss = layer(x, torch.from_numpy(masks).to(DEV))
    loss.backward()
    g = x.grad.cpu().numpy()
    dev_rows = [r.cpu().numpy() for r in ops.cubical3d_persistence(x.detach(), dim)]
    x64 = torch.from_numpy(f.astype(np.float64)).requires_grad_(True)
    l64 = R.torch_loss(x64, dev_rows, layer.last_m.tolist(), q)
    l64.backward()
    g64 = x64.grad.numpy()
    assert abs(float(loss) - float(l64)) <= 1e-6 * max(1.0, abs(float(l64)))
    bar = 1e-6 * np.abs(g64).max()
    print(f"dim {dim} q {q}: max|g| {np.abs(g64).max():.3e} worst error {np.abs(g - g64).max():.3e} bar {bar:.3e}")
    assert np.abs(g64).max() > 0 and np.abs(g - g64).max() <= bar
    touched = np.zeros(g.shape, bool)
    for n in range(2):
        touched[n].reshape(-1)[dev_rows[n].reshape(-1)] = True
    assert (g[~touched] == 0).all() and (g64[~touched] == 0).all()


@pytest.mark.parametrize("dim", [0, 2])
def test_two_runs_are_bit_identical(dim):
    from multimodal_mvd_seg_amd import losses
    f = np.stack([R.field((16, 24, 40), 5, 6), R.field((16, 24, 40), 6, None)])   # ties: many bars share voxels
    t = torch.from_numpy(np.stack([_mask((16, 24, 40), 7, 0.3), _mask((16, 24, 40), 8, 0.7)])).to(DEV)
    out = []
    for _ in range(2):
        x = torch.from_numpy(f.copy()).to(DEV).requires_grad_(True)
        l = losses.CubicalWassersteinLoss(dim, 2)(x, t)
        l.backward()
        out.append((l.detach().cpu().numpy().tobytes(), x.grad.cpu().numpy().tobytes()))
    assert out[0] == out[1]
    assert np.frombuffer(out[0][1], np.float32).any()


@pytest.mark.parametrize("dim", [0, 2])
def test_bars_already_at_the_target_give_zero_loss_and_gradient(dim):
    from multimodal_mvd_seg_amd import losses, ops
    f = np.zeros((1, 5, 6, 7), np.float32)
    for p in [(1, 1, 1), (2, 3, 3), (3, 4, 5)]:
        f[(0,) + p] = 1.0
    if dim == 0:
        f = 1 - f           # isolated minima at 0 in a field of 1: the eldest is essential, the others are bars (0, 1)
    x = torch.from_numpy(f).to(DEV).requires_grad_(True)
    layer = losses.CubicalWassersteinLoss(dim, 2)
    loss = layer(x, torch.from_numpy(f).to(DEV))
    n_bars = ops.cubical3d_persistence(x.detach(), dim)[0].shape[0]
    assert n_bars == (3 if dim == 2 else 2) and layer.last_m.tolist() == [n_bars]
    loss.backward()
    assert float(loss) == 0.0 and not x.grad.any()


def test_diagram_layer_gathers_from_the_field_and_scatters_back():
    from multimodal_mvd_seg_amd import losses
    f, rows = _case((6, 7, 9), 2, None)
    x = torch.from_numpy(f.copy()).to(DEV).requires_grad_(True)
    dgms = losses.CubicalComplex3D(2)(x)
    assert len(dgms) == 2
    for n in range(2):
        assert np.array_equal(dgms[n].detach().cpu().numpy(), R.rows_to_bars(f[n], rows[n]))
    sum((d[:, 1] - d[:, 0]).sum() for d in dgms).backward()
    want = np.zeros(f.shape, np.float64)
    for n in range(2):
        r = np.asarray(rows[n]).reshape(-1, 2)
        np.add.at(want[n].reshape(-1), r[:, 1], 1.0)
        np.add.at(want[n].reshape(-1), r[:, 0], -1.0)
    assert np.array_equal(x.grad.cpu().numpy(), want.astype(np.float32))


# ------------------------------------------------------------------------------------------------------------ the trainer
STRIDES = [[1, 1, 1], [2, 2, 2], [2, 2, 2]]     # three stages: two deep-supervision outputs carry weight
DS = {"channel_names": {"0": "a"}, "labels": {"background": 0, "a": 1, "vessel": 2}, "file_ending": ".nii.gz"}


def _trainer(seed):
    from multimodal_mvd_seg_amd import trainer
    torch.manual_seed(seed)
    tr = trainer.ContrastiveTrainerMI355(trainer.make_plans((16, 16, 16), STRIDES, batch_size=2), "3d_fullres", 0,
                                         DS, device=DEV)
    tr.use_hip_graph = False
    tr.initialize()
    tr.on_train_epoch_start()
    return tr


def _batch(tr):
    from oracle import step_oracle as SO
    b = SO.synthetic_batch(2, 1, (16, 16, 16), STRIDES, num_classes=3, seed=3)
    return {"data": b["data"].to(DEV), "target": [t.to(DEV) for t in b["target"]]}


def _parent_forward_loss(tr, data, target):
    """_forward_loss of ContrastiveTrainerMI355 as it stood before topo_term existed: none of the new attributes is read"""
    from multimodal_mvd_seg_amd import losses, ops
    o1, o2, f1, f2 = tr.network(data)
    v = tr.vessel_channel
    l = tr.loss(o1, target) + tr.loss(o2, target)
    top1 = o1[0] if isinstance(o1, (list, tuple)) else o1
    top2 = o2[0] if isinstance(o2, (list, tuple)) else o2
    tgt0 = target[0] if isinstance(target, (list, tuple)) else target
    mutual = losses.kl_loss_compute1(top1[:, v], top2[:, v], tr.kl_T)
    if tr.feat_kl:
        mutual = mutual + losses.l2_loss(f1, f2, channel_wise=True, T=tr.kl_T)
    l = l + tr.lambda1 * mutual
    if tr.use_topo:
        prob = ops.SoftmaxSelectFn.apply(top1, v)
        tmask = ops.label_mask(tgt0, v).reshape(prob.shape)
        l = l + tr.lambda3 * losses.soft_cldice(prob, tmask, tr.skel_iter)
    return l


def test_trainer_step_with_the_cubical_term():
    from multimodal_mvd_seg_amd import losses, ops
    tr = _trainer(11)
    batch = _batch(tr)
    tr.topo_term, tr.lambda3 = "cubical", 0.5
    with pytest.raises(RuntimeError, match="cannot be captured"):
        tr.use_hip_graph = True
        tr.train_step(batch)
    tr.use_hip_graph = False
    v = tr.vessel_channel
    with torch.no_grad():
        tr.use_topo = False
        base = float(tr._forward_loss(batch["data"], batch["target"])[0])
        tr.use_topo = True
        o1 = tr.network(batch["data"])[0]
        top1 = o1[0] if isinstance(o1, (list, tuple)) else o1
        tgt0 = batch["target"][0] if isinstance(batch["target"], list) else batch["target"]
        term = float(losses.CubicalWassersteinLoss(2, 2)(top1[:, v].float().contiguous(),
                                                         ops.label_mask(tgt0, v).reshape(top1[:, v].shape)))
    before = [p.detach().clone() for p in tr.network.parameters()]
    res = tr.train_step(batch)
    want = base + 0.5 * term
    print(f"cubical trainer step: base {base:.7f} term {term:.7f} loss {float(res['loss']):.7f}")
    assert term > 0 and abs(float(tr.last_cubical) - term) <= 1e-6 * max(1.0, term)
    assert abs(float(res["loss"]) - want) <= 1e-6 * max(1.0, abs(want))
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, tr.network.parameters()))
    assert tr.last_topology is not None and tr.last_topology["cc_pred"].shape == (2,)


def test_trainer_default_flags_give_the_parent_loss_bits():
    tr = _trainer(12)
    batch = _batch(tr)
    assert tr.topo_term == "cldice"
    with torch.no_grad():
        a = tr._forward_loss(batch["data"], batch["target"])[0]
        b = _parent_forward_loss(tr, batch["data"], batch["target"])
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    tr2 = _trainer(12)
    l1 = tr.train_step(batch)["loss"]
    l2 = tr2.train_step(batch)["loss"]
    assert np.asarray(l1).tobytes() == np.asarray(l2).tobytes() == a.cpu().numpy().tobytes()
