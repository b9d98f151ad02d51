"""GPU tests of the 2-D level-set persistence (csrc/levelset2d.hip) and the persistence topological loss on it, against
fixtures the reference's own code computed (tests/golden/levelset2d_diagrams.npz, topoloss_*.npz; generator:
tools/make_golden_levelset2d.py).  Diagrams are integer / comparison work: compared exactly.  Each bar length is one fp32
subtraction of two input values: compared exactly.  The loss and its gradient are sums of exact products: the bounds in
the tests are the rounding of those sums (u = 2^-24), with the terms taken from the fixtures.  The expected gradient is the
reference's taken one problem per forward + backward: its TopoLoss shares one complex between the problems of a batched call
and then maps every gradient through the last problem's critical vertices."""
import math

import numpy as np
import pytest
import torch

from levelset2d_ref import counts, fixture, split, srt

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -24
DIAGRAMS = "levelset2d_diagrams.npz"
NAMES = ["1x1", "1x5", "5x1", "2x2", "3x2", "5x4", "8x8", "7x9", "16x12", "32x32"]
LOSS_SIZES = ["5x4", "16x12", "32x32"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from multimodal_mvd_seg_amd import _lib
    _lib.load()


def _bars(x, channels, sublevel, maxdim=1):
    from multimodal_mvd_seg_amd import ops
    bars, er = ops.levelset2d_persistence(x, channels, sublevel, maxdim)
    return bars.cpu().numpy(), er.cpu().numpy()


@pytest.mark.parametrize("sublevel", [True, False])
@pytest.mark.parametrize("name", NAMES)
def test_device_keys_sort_and_pairing_equal_the_reference_diagrams(name, sublevel):
    d = fixture(DIAGRAMS)
    f = d[name + "/f"]
    tag = name + ("/sub" if sublevel else "/super")
    want0, want1 = d[tag + "/dgm0"], d[tag + "/dgm1"]
    H, W = f.shape
    V, E, T = counts(H, W)
    bars, er = _bars(torch.from_numpy(f).to(DEV)[None, None], [0], sublevel)
    assert bars.shape == (1, V + T, 4) and er.shape == (1, E)
    d0, d1 = split(bars[0], V)
    assert np.array_equal(srt(d0[:, :2]), srt(want0[:, :2])) and np.array_equal(srt(d1[:, :2]), srt(want1[:, :2]))
    if bool(d[name + "/tie_free"]):
        assert np.array_equal(srt(d0), want0) and np.array_equal(srt(d1), want1)      # critical vertices, row for row


def test_layer_returns_device_diagrams_like_the_reference_layer():
    from multimodal_mvd_seg_amd import losses
    d = fixture(DIAGRAMS)
    f = d["16x12/f"]
    for sublevel in (True, False):
        layer = losses.LevelSetLayer2D(size=(16, 12), maxdim=1, sublevel=sublevel, alg='cohom')
        dgms, issub = layer(torch.from_numpy(f).to(DEV))
        assert issub is sublevel and len(dgms) == 2 and all(t.is_cuda for t in dgms)
        tag = "16x12/" + ("sub" if sublevel else "super")
        for k in range(2):
            assert np.array_equal(srt(dgms[k].cpu().numpy()), d[f"{tag}/dgm{k}"][:, :2])
    dgms, _ = losses.LevelSetLayer2D(size=(16, 12), maxdim=0)(torch.from_numpy(f).to(DEV))
    assert len(dgms) == 1 and np.array_equal(srt(dgms[0].cpu().numpy()), d["16x12/sub/dgm0"][:, :2])


@pytest.mark.parametrize("ties", [False, True])
def test_a_batch_of_planes_equals_the_single_plane_calls_bit_for_bit(ties):
    g = torch.Generator().manual_seed(11)
    x = torch.randn((2, 3, 9, 7), generator=g)
    if ties:
        x = torch.round(x * 2) / 2
    x = x.to(DEV)
    bars, er = _bars(x, [1, 2], False)
    p = 0
    for b in range(2):
        for c in (1, 2):
            one, eone = _bars(x[b:b + 1, c:c + 1].contiguous(), [0], False)
            assert np.array_equal(bars[p], one[0]) and np.array_equal(er[p], eone[0]), (b, c)
            p += 1


def _loss_case(size):
    z = fixture(f"topoloss_{size}.npz")
    return z, torch.from_numpy(z["y_pred"]).to(DEV), torch.from_numpy(z["y_raw"]).to(DEV), [int(i) for i in z["idx"]]


@pytest.mark.parametrize("size", LOSS_SIZES)
def test_topk_bar_lengths_are_bit_equal_to_the_reference(size):
    from multimodal_mvd_seg_amd import losses, ops
    z, y_pred, _, idx = _loss_case(size)
    dgms = ops.LevelSetDiagram2DFn.apply(y_pred, [i + 1 for i in idx], False, 1)
    for k in (5, 20):
        want = z[f"k{k}/topk"].reshape(-1, 2, k)                      # problem p = b * len(idx) + n
        for dim in range(2):
            got = losses.TopKBarcodeLengths(dim, k)((dgms, False)).cpu().numpy()
            assert got.shape == (want.shape[0], k)
            assert np.array_equal(got.view(np.uint32), want[:, dim].copy().view(np.uint32)), (k, dim)
    # one diagram at a time, as the reference layer is used
    one = losses.TopKBarcodeLengths(1, 20)(((dgms[0][2], dgms[1][2]), False)).cpu().numpy()
    assert np.array_equal(one, z["k20/topk"].reshape(-1, 2, 20)[2, 1])


@pytest.mark.parametrize("with_raw", [False, True])
@pytest.mark.parametrize("max_k", [5, 20])
@pytest.mark.parametrize("size", LOSS_SIZES)
def test_topoloss_value_and_gradient_follow_the_reference(size, max_k, with_raw):
    from multimodal_mvd_seg_amd import losses
    z, y_pred, y_raw, idx = _loss_case(size)
    W, H = (int(v) for v in size.split("x"))
    tag = f"k{max_k}/"
    sub = tag + ("with_raw/" if with_raw else "topo_only/")
    label = torch.from_numpy(z[tag + "topo_label"]).to(DEV)
    sw = 10 if with_raw else 0
    loss = losses.TopoLoss((W, H), topo_weight=1, sqdiff_weight=sw, max_k=max_k)

    def run():
        yp = y_pred.clone().requires_grad_(True)
        l = loss(yp, y_raw if with_raw else None, label, idx=idx)
        l.backward()
        return float(l), yp.grad.cpu().numpy()

    got, grad = run()
    want, wgrad = float(z[sub + "loss"]), z[sub + "grad"]
    # value: a sum of at most 2 max_k exact squares per problem
    bound = 2 * max_k * U * float(z[tag + "sum_len_sq"])
    a, b = z["y_pred"].astype(np.float64), z["y_raw"].astype(np.float64)
    N = a.size
    gm = np.zeros_like(a)
    if with_raw:
        # 10 * mean((a-b)^2) in fp32 on both sides: 3 roundings per element, a pairwise sum of N terms, the division and
        # the weight, then the rounding of the final addition
        mse = float(((a - b) ** 2).mean())
        bound += (3 + math.ceil(math.log2(N)) + 2) * U * sw * mse + U * abs(want)
        gm = sw * 2 * (a - b) / N
    print(f"{size} k={max_k} raw={with_raw}: loss {got:.9g} reference {want:.9g} |diff| {abs(got - want):.3g} bound {bound:.3g}")
    assert abs(got - want) <= bound
    # gradient: every contribution is an exact product scaled once; m bars meeting at a vertex are summed with m - 1 roundings
    m, asum = z[tag + "grad_bars_meeting"], z[tag + "grad_abs_sum"].astype(np.float64)
    gbound = np.maximum(m - 1, 0) * U * asum
    if with_raw:
        gbound = gbound + 4 * U * np.abs(gm) + U * np.abs(wgrad) * 2     # the MSE gradient (4 roundings) and the two additions
    diff = np.abs(grad.astype(np.float64) - wgrad)
    print(f"   gradient: max |diff| {diff.max():.3g}, max bound {gbound.max():.3g}, vertices with bars {int((m > 0).sum())}")
    assert (diff <= gbound).all()
    if not with_raw:
        assert (grad[wgrad == 0] == 0).all() and (grad[m == 0] == 0).all()
    got2, grad2 = run()
    assert got2 == got and np.array_equal(grad2.view(np.uint32), grad.view(np.uint32))


def test_diagram_gradient_lands_on_the_critical_vertices_in_a_fixed_order():
    from multimodal_mvd_seg_amd import ops
    g = torch.Generator().manual_seed(5)
    x = (torch.round(torch.randn((2, 3, 9, 7), generator=g) * 2) / 2).to(DEV)       # heavy ties: many bars share a vertex
    H, W = 9, 7
    V, E, T = counts(H, W)

    def run(maxdim):
        xx = x.clone().requires_grad_(True)
        dgms = ops.LevelSetDiagram2DFn.apply(xx, [2, 0], True, maxdim)
        ws = [torch.randint(-8, 9, d.shape, generator=torch.Generator().manual_seed(k)).float().to(DEV) for k, d in enumerate(dgms)]
        tot = sum((torch.where(torch.isfinite(d), d, torch.zeros_like(d)) * w).sum() for d, w in zip(dgms, ws))
        tot.backward()
        return xx.grad.cpu().numpy(), [w.cpu().numpy() for w in ws]

    for maxdim in (1, 0):
        grad, ws = run(maxdim)
        bars = _bars(x, [2, 0], True, maxdim)[0]
        want = np.zeros((2, 3, V))
        for p in range(4):
            b, c = p // 2, (2, 0)[p % 2]
            rows = [bars[p][:V]] + ([bars[p][V:]] if maxdim else [])
            for r, w in zip(rows, ws):
                for col in range(2):
                    ok = r[:, 2 + col] >= 0
                    np.add.at(want[b, c], r[ok, 2 + col], w[p][ok, col])            # small integers: exact in any order
        assert np.array_equal(grad.reshape(2, 3, V), want), maxdim
        assert (grad[:, 1] == 0).all()
        assert np.array_equal(run(maxdim)[0], grad)


def _mask(rows):
    return torch.tensor([[int(ch) for ch in r] for r in rows], dtype=torch.float32)


MASKS = {
    "one blob": (["000000", "011100", "011100", "000000"], (1, 0)),
    "two blobs": (["110000", "110011", "000011", "000000"], (2, 0)),
    "ring": (["00000", "01110", "01010", "01110", "00000"], (1, 1)),
    "ring with a dot inside": (["0000000", "0111110", "0100010", "0101010", "0100010", "0111110", "0000000"], (2, 1)),
    "diagonal neighbours along the Freudenthal diagonal": (["000", "010", "001"], (1, 0)),
    "diagonal neighbours across it": (["000", "001", "010"], (2, 0)),
    "empty": (["000", "000"], (0, 0)),
    "full": (["111", "111", "111"], (1, 0)),
}


@pytest.mark.parametrize("name", list(MASKS))
def test_betti_topo_label_counts_components_and_holes(name):
    from multimodal_mvd_seg_amd import losses
    rows, (b0, b1) = MASKS[name]
    m = _mask(rows)
    # class 1 is the mask, class 2 is absent, class 0 is its complement; two samples: the mask and its transpose-free copy
    t = torch.stack([m, m])[:, None].to(DEV)
    lab = losses.betti_topo_label(t, 3)
    assert lab.is_cuda and lab.dtype == torch.int32 and tuple(lab.shape) == (2, 3, 2)
    lab = lab.cpu().numpy()
    assert lab[0, 1].tolist() == [b0, b1] and lab[1, 1].tolist() == [b0, b1], lab
    assert lab[0, 2].tolist() == [0, 0]


def test_betti_numbers_of_the_background_of_a_ring():
    from multimodal_mvd_seg_amd import losses
    m = _mask(MASKS["ring"][0])
    lab = losses.betti_topo_label(m[None].to(DEV), 2).cpu().numpy()
    # background: the outer frame and the enclosed pixel; the frame is itself a loop around the ring
    assert lab[0, 0].tolist() == [2, 1] and lab[0, 1].tolist() == [1, 1]


# ------------------------------------------------------------------------------------------------------------------- trainer
CH = {"channel_names": {"0": "a", "1": "b"}}
PLAIN = dict(CH, labels={"background": 0, "a": 1, "b": 2, "c": 3})


def _trainer(precision="fp32"):
    from multimodal_mvd_seg_amd import trainer
    plans = trainer.make_plans((32, 32), [[1, 1], [2, 2], [2, 2]], batch_size=2, base_features=8, max_features=16, configuration="2d")
    tr = trainer.nnUNetTrainerTopoLossMI355(plans, "2d", 0, PLAIN, device=DEV)
    tr.precision = precision
    torch.manual_seed(0)
    return tr


def test_trainer_step_adds_the_topological_term_to_the_parent_loss():
    from multimodal_mvd_seg_amd import losses, ops
    tr = _trainer()
    assert tr.use_hip_graph is False
    tr.initialize()
    tr.on_train_epoch_start()
    g = torch.Generator().manual_seed(3)
    data = torch.rand((2, 2, 32, 32), generator=g)
    top = torch.randint(0, 4, (2, 1, 8, 8), generator=g).float().repeat_interleave(4, 2).repeat_interleave(4, 3)
    batch = {'data': data, 'target': [top, top[:, :, ::2, ::2].contiguous()]}
    with torch.no_grad():
        outs = tr.network(data.to(DEV))
        assert len(outs) == 2 and tuple(outs[0].shape) == (2, 4, 32, 32)
        base = tr.loss(outs, [t.to(DEV) for t in batch['target']])
        y_pred = torch.cat([ops.SoftmaxSelectFn.apply(outs[0], c) for c in range(4)], 1)
        label = losses.betti_topo_label(top.to(DEV), 4)
        term = losses.TopoLoss((32, 32), sqdiff_weight=0, max_k=20)(y_pred, None, label[:, 1:], idx=[0, 1, 2])
        want = (base + tr.topo_lambda * term).cpu().numpy()
        assert float(term) != 0.0
        # the probabilities are the softmax: the separately computed term moves by no more than its conditioning allows
        loose = losses.TopoLoss((32, 32), sqdiff_weight=0, max_k=20)(torch.softmax(outs[0], 1), None, label[:, 1:], idx=[0, 1, 2])
        assert abs(float(loose) - float(term)) <= 1e-5 * max(abs(float(term)), 1e-3)
    before = [p.detach().clone() for p in tr.network.parameters()]
    got = np.asarray(tr.train_step(batch)["loss"])
    print(f"step loss {float(got):.7f} = parent {float(base):.7f} + {tr.topo_lambda} * {float(term):.7f}")
    assert np.array_equal(got, want), (got, want)
    assert np.array_equal(tr.last_topo.cpu().numpy(), term.cpu().numpy())
    changed = sum(int(not torch.equal(a, b.detach())) for a, b in zip(before, tr.network.parameters()))
    # all but the bias of the coarsest head: that level has deep-supervision weight 0 and its bias starts at 0
    assert changed >= len(before) - 1
    tr.use_hip_graph = True
    with pytest.raises(RuntimeError, match="cannot be captured"):
        tr.train_step(batch)


def test_trainer_refuses_bf16():
    tr = _trainer("bf16")
    with pytest.raises(NotImplementedError, match="only fp32 is built"):
        tr.initialize()
