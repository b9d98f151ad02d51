"""CPU tests of the 3-D cubical persistence loss: the two union-find restatements against the brute-force cubical complex,
the selection identity against the full assignment problem, the HOST pairing of the library (mvd_cub3d_pair_host is plain
C++) on keys built in numpy by the kernel's formula, and the refusals.  The device half is tests/test_gpu_cubical3d.py."""
import ctypes

import numpy as np
import pytest
import torch

import cubical3d_ref as R

SHAPES = [(3, 4, 5), (4, 4, 4), (2, 5, 3), (1, 4, 4), (5, 3, 1), (6, 7, 9)]


@pytest.mark.parametrize("levels", [None, 6])
@pytest.mark.parametrize("dim", [0, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_brute_force_equals_the_union_find_restatement(shape, dim, levels):
    f = R.field(shape, 100 + 7 * sum(shape), levels)
    want = R.brute_force_intervals(f, dim)
    got = R.multiset(R.rows_to_bars(f, R.restatement_rows(f, dim)))
    assert got == want
    if levels is None and min(shape) >= 3 and dim == 0:
        assert len(got) > 0


def _shell():
    f = np.full((5, 5, 5), 0.9, np.float32)
    f[1:4, 1:4, 1:4] = np.linspace(0.1, 0.36, 27, dtype=np.float32).reshape(3, 3, 3)   # the low shell, 3x3x3
    f[2, 2, 2] = 0.8                                                                      # around one high voxel
    return f


def test_closed_shell_gives_exactly_one_void():
    f = _shell()
    # the void closes when the last of the 6 face neighbours of the centre enters: the faces are what separates it
    faces = [f[1, 2, 2], f[3, 2, 2], f[2, 1, 2], f[2, 3, 2], f[2, 2, 1], f[2, 2, 3]]
    for fn in (lambda g: R.brute_force_intervals(g, 2),
               lambda g: R.multiset(R.rows_to_bars(g, R.restatement_rows(g, 2))),
               lambda g: R.multiset(R.rows_to_bars(g, R.pair_host(g[None], 2)[0]))):
        assert fn(f) == [(float(max(faces)), float(np.float32(0.8)))]
    rows = R.pair_host(f[None], 2)[0]
    assert rows[0, 1] == np.ravel_multi_index((2, 2, 2), f.shape)


def test_shell_with_one_face_raised_gives_none():
    f = _shell()
    f[1, 2, 2] = 0.95            # the centre now leaks to the outside block above its own value
    f[0, 2, 2] = 0.95
    assert R.brute_force_intervals(f, 2) == []
    assert R.restatement_rows(f, 2) == []
    assert len(R.pair_host(f[None], 2)[0]) == 0


def test_blob_touching_the_border_gives_none():
    f = np.full((4, 5, 5), 0.1, np.float32)
    f[0:2, 2, 2] = [0.9, 0.8]
    assert R.brute_force_intervals(f, 2) == []
    assert R.restatement_rows(f, 2) == []
    assert len(R.pair_host(f[None], 2)[0]) == 0


@pytest.mark.parametrize("q", [1, 2, 3])
def test_selection_equals_the_assignment_problem(q):
    rng = np.random.default_rng(5 + q)
    cases = [(n, m) for n in range(0, 9) for m in range(0, 5)] + [(0, 0), (2, 7), (0, 3), (5, 0)]
    for n, m in cases:
        for _ in range(3):
            b = rng.uniform(-0.6, 1.2, n)
            bd = np.stack([b, b + rng.uniform(0.0, 1.5, n)], 1)
            a, s = R.wq_lsa(bd, m, q), R.wq_selection(bd, m, q)
            assert abs(a - s) <= 1e-12 * max(1.0, abs(a)), (n, m, a, s)


def test_zero_persistence_bars_never_gain():
    for q in (1, 2, 3):
        b = np.linspace(-2, 2, 41)
        assert (R.costs(np.stack([b, b], 1), q)[2] <= 0).all()


@pytest.mark.parametrize("levels", [None, 6])
@pytest.mark.parametrize("dim", [0, 2])
@pytest.mark.parametrize("shape", SHAPES + [(16, 24, 40)])
def test_host_pairing_equals_the_restatement(shape, dim, levels):
    f = np.stack([R.field(shape, 11 + sum(shape), levels), R.field(shape, 12 + sum(shape), levels)])
    if levels is None:
        f[1].reshape(-1)[0] = -0.0
    got = R.pair_host(f, dim)
    for n in range(2):
        want = R.restatement_rows(f[n], dim)
        flat = f[n].reshape(-1)
        assert R.multiset(R.rows_to_bars(f[n], got[n])) == R.multiset(R.rows_to_bars(f[n], want))
        assert (flat[got[n][:, 1]] > flat[got[n][:, 0]]).all()          # f[birth voxel] = b < d = f[death voxel]
        assert got[n].min(initial=0) >= 0 and got[n].max(initial=0) < flat.size
        if levels is None:
            assert len(np.unique(flat)) == flat.size                      # tie free: the voxel rows themselves
            assert set(map(tuple, got[n].tolist())) == set(want)
        else:
            assert got[n].tolist() == [list(r) for r in want]            # same tie rules: the same sweep


def h0_rows(f, death, dv):
    """the dimension-0 cubical rows read off the conn-26 sublevel H0 pairing: its finite bars of non-zero length"""
    flat = np.asarray(f, dtype=np.float32).reshape(-1)
    keep = (dv >= 0) & (death > flat)
    return np.stack([np.nonzero(keep)[0], dv[keep]], 1).astype(np.int32)


def test_dimension_0_is_the_26_connected_h0_pairing():
    """mvd_cub3d_pair_host(dim 0) and mvd_h0_pair_host(conn 26, sublevel) run one sweep on one key array"""
    import test_h0_host as H0
    most = 0
    for shape in SHAPES + [(1, 1, 7)]:
        for levels in (None, 6):
            f = R.field(shape, 100 + 7 * sum(shape), levels)
            assert np.array_equal(R.sorted_keys(f, 0), H0.host_sorted_keys(f, 26, True))
            rows = R.pair_host(f[None], 0)[0]
            rows = rows[np.argsort(rows[:, 0], kind="stable")]
            _, death, dv, _ = H0.pair(f, 26, True)
            want = h0_rows(f, death, dv)
            assert rows.dtype == want.dtype and np.array_equal(rows, want), (shape, levels)
            most = max(most, len(rows))
    assert most >= 20


def test_host_pairing_is_the_same_over_the_thread_pool():
    f = np.stack([R.field((6, 7, 9), s, 6 if s % 2 else None) for s in range(20)])
    for dim in (0, 2):
        a, b = R.pair_host(f, dim, n_threads=16), R.pair_host(f, dim, n_threads=1)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_host_pairing_rejects_foreign_keys_and_dimension_1():
    from multimodal_mvd_seg_amd import _lib
    lib = _lib.load()
    f = R.field((3, 4, 5), 3)[None]
    keys = R.sorted_keys(f[0], 2)[None]
    bad = keys.copy()
    bad[0, [3, 4]] = bad[0, [4, 3]]
    with pytest.raises(RuntimeError, match="sorted filtration"):
        R.pair_host(f, 2, bad)
    bad = keys.copy()
    bad[0, -1] |= np.uint64(0x7fffffff)
    with pytest.raises(RuntimeError, match="sorted filtration"):
        R.pair_host(f, 2, bad)
    with pytest.raises(RuntimeError, match="n_keys"):
        R.pair_host(f, 2, keys[:, :-1])
    with pytest.raises(RuntimeError, match="matrix reduction"):
        R.pair_host(f, 1, keys)
    nv = ctypes.c_long()
    assert lib.mvd_cub3d_num_keys(3, 4, 5, 1, None) < 0 and lib.mvd_cub3d_num_keys(0, 4, 5, 2, None) < 0
    assert lib.mvd_cub3d_num_keys(3, 4, 5, 2, ctypes.byref(nv)) == 60 * 4 and nv.value == keys.shape[1]
    assert lib.mvd_cub3d_num_keys(3, 4, 5, 0, ctypes.byref(nv)) == 60 * 13 and nv.value == len(R.sorted_keys(f[0], 0))


def test_the_loss_refuses_what_it_does_not_build():
    from multimodal_mvd_seg_amd import losses, ops
    with pytest.raises(NotImplementedError, match="matrix reduction"):
        losses.CubicalWassersteinLoss(dim=1)
    with pytest.raises(NotImplementedError, match="matrix reduction"):
        losses.CubicalComplex3D(1)
    with pytest.raises(NotImplementedError, match="matrix reduction"):
        ops.cubical3d_persistence(torch.zeros(1, 2, 2, 2), 1)
    with pytest.raises(ValueError):
        losses.CubicalWassersteinLoss(dim=3)
    with pytest.raises(ValueError, match="q must be >= 1"):
        losses.CubicalWassersteinLoss(q=0.5)
    f, t = torch.zeros(1, 3, 3, 3), torch.zeros(1, 3, 3, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        losses.CubicalWassersteinLoss()(f, t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        losses.CubicalComplex3D(2)(f)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cubical3d_persistence(f, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cubical3d_target_count(t, 2)
    t[0, 1, 1, 1] = 0.5
    with pytest.raises(ValueError, match="binary"):
        losses.CubicalWassersteinLoss()(f, t)


def _trainer(cls="ContrastiveTrainerMI355"):
    from multimodal_mvd_seg_amd import trainer
    ds = {"channel_names": {"0": "a"}, "labels": {"background": 0, "a": 1, "vessel": 2}, "file_ending": ".nii.gz"}
    plans = trainer.make_plans((16, 16, 16), [[1, 1, 1], [2, 2, 2]])
    return getattr(trainer, cls)(plans, "3d_fullres", 0, ds, device=torch.device("cuda"))


@pytest.mark.parametrize("cls", ["ContrastiveTrainerMI355", "FinalNetTrainerMI355"])
def test_trainer_cubical_term_refuses_the_graphed_step(cls):
    tr = _trainer(cls)
    assert (tr.topo_term, tr.topo_feat_d, tr.topo_q) == ("cldice", 2, 2)
    tr.use_hip_graph = False
    assert tr._graph_allowed() is False
    tr.use_hip_graph = True
    assert tr._graph_allowed() is True               # the default term keeps the parent's answer
    tr.topo_term = "cubical"
    with pytest.raises(RuntimeError, match="cannot be captured"):
        tr._graph_allowed()
    tr.use_hip_graph = False
    assert tr._graph_allowed() is False
    tr.use_topo, tr.use_hip_graph = False, True      # no topology term at all: nothing to refuse
    assert tr._graph_allowed() is True


def test_trainer_default_flags_stay_on_the_soft_cldice_branch(monkeypatch):
    """_forward_loss with the default flags never reaches the cubical loss and calls soft_cldice exactly as before; with
    topo_term = 'cubical' it is the other way round."""
    from multimodal_mvd_seg_amd import losses, ops
    tr = _trainer()
    calls = []
    x = torch.zeros(2, 3, 4, 4, 4, requires_grad=True)
    tr.network = lambda data: ([x], [x], x, x)
    tr.loss = lambda o, t: o[0].sum() * 0
    tr.topo_cc = False
    monkeypatch.setattr(losses, "kl_loss_compute1", lambda a, b, T: a.sum() * 0)
    monkeypatch.setattr(losses, "l2_loss", lambda a, b, channel_wise, T: a.sum() * 0)
    monkeypatch.setattr(ops.SoftmaxSelectFn, "apply", lambda top, v: top[:, v:v + 1])
    monkeypatch.setattr(ops, "label_mask", lambda t, v: (t == v).float())
    monkeypatch.setattr(losses, "soft_cldice", lambda p, t, it: calls.append(("cldice", tuple(p.shape), it)) or p.sum() * 0 + 2)

    class Spy:
        def __init__(self, dim, q):
            calls.append(("cubical", dim, q))

        def __call__(self, field, target):
            calls.append(("field", tuple(field.shape), field.dtype, tuple(target.shape)))
            return field.sum() * 0 + 3

    monkeypatch.setattr(losses, "CubicalWassersteinLoss", Spy)
    tgt = [torch.full((2, 1, 4, 4, 4), 2.0)]
    l, _ = tr._forward_loss(None, tgt)
    assert calls == [("cldice", (2, 1, 4, 4, 4), 3)] and float(l) == 2.0
    calls.clear()
    tr.topo_term, tr.topo_feat_d, tr.topo_q, tr.lambda3 = "cubical", 0, 3, 0.5
    l, _ = tr._forward_loss(None, tgt)
    assert calls == [("cubical", 0, 3), ("field", (2, 4, 4, 4), torch.float32, (2, 4, 4, 4))] and float(l) == 1.5
    tr.topo_term = "nonsense"
    with pytest.raises(ValueError, match="topo_term"):
        tr._forward_loss(None, tgt)
