"""CPU tests of tests/topk_ref.py, the fp64 restatement the top-k kernels are tested against: it reproduces the
reference's own TopKLoss (tests/golden/topk_loss.npz, written by tools/make_golden.py topk_loss) to 1e-12, equals
torch.topk on tie-free inputs, and implements the equal-share tie rule."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import topk_ref as TR
from conftest import load_npz


@pytest.fixture(scope="module")
def golden():
    return load_npz("topk_loss.npz")


def _case(z, name):
    logits = torch.from_numpy(z[f"{name}/logits"]).double().requires_grad_(True)
    return logits, torch.from_numpy(z[f"{name}/target"]), int(z[f"{name}/ignore_index"]), float(z[f"{name}/label_smoothing"])


def test_restatement_reproduces_every_record_of_the_reference(golden):
    names = [str(n) for n in golden["cases"]]
    assert len(names) >= 9 and "mostly_ignored" in names and "k_is_1" in names
    for name in names:
        logits, target, ign, eps = _case(golden, name)
        loss = TR.topk_loss(logits, target, 10, ign, eps)
        loss.backward()
        assert TR.topk_count(target.numel(), 10) == int(golden[f"{name}/k"])
        lerr = abs(float(loss) - float(golden[f"{name}/loss"]))
        gerr = float((logits.grad - torch.from_numpy(golden[f"{name}/dlogits"])).abs().max())
        print(f"{name}: loss {float(loss):.12f} |d| {lerr:.1e}; dlogits max |d| {gerr:.1e}")
        assert lerr <= 1e-12 and gerr <= 1e-12, (name, lerr, gerr)
    assert bool(golden["k_zero_is_nan"])


def test_mostly_ignored_is_the_sum_of_the_valid_voxels_over_k(golden):
    logits, target, ign, eps = _case(golden, "mostly_ignored")
    assert tuple(logits.shape) == (2, 3, 4, 4, 4) and int((target != ign).sum()) == 3 and int(golden["mostly_ignored/k"]) == 12
    ce = TR.ce_per_voxel(logits, target, ign, eps).detach()
    want = float(ce[(target[:, 0] != ign)].sum()) / 12
    loss, _, t, cnt_gt, cnt_eq, w = TR.topk_loss(logits, target, 10, ign, eps, parts=True)
    assert abs(float(loss) - want) <= 1e-15 and abs(float(golden["mostly_ignored/loss"]) - want) <= 1e-15
    assert float(t) == 0.0 and cnt_gt == 3 and cnt_eq == 125


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_equals_torch_topk_on_tie_free_inputs(seed, eps):
    torch.manual_seed(seed)
    z = (torch.randn(3, 5, 5, 7, 9, dtype=torch.float64) * 2).requires_grad_(True)
    t = torch.randint(0, 5, (3, 1, 5, 7, 9)).float()
    ce = F.cross_entropy(z, t[:, 0].long(), reduction='none', label_smoothing=eps)
    k = int(ce.numel() * 10 / 100)
    assert k == 94
    want = torch.topk(ce.view(-1), k, sorted=False)[0].mean()
    gw, = torch.autograd.grad(want, z)
    loss, _, thr, cnt_gt, cnt_eq, w = TR.topk_loss(z, t, 10, -100, eps, parts=True)
    g, = torch.autograd.grad(loss, z)
    assert cnt_eq == 1 and cnt_gt == k - 1
    assert abs(float(loss) - float(want)) <= 1e-15 and torch.equal(g, gw)
    assert int((w > 0).sum()) == k


def test_all_equal_input_gives_log_k_and_uniform_weights():
    for K in (2, 3, 5, 8):
        z = torch.zeros(1, K, 5, 7, 9, dtype=torch.float64)
        t = torch.randint(0, K, (1, 1, 5, 7, 9), generator=torch.Generator().manual_seed(K)).float()
        loss, ce, thr, cnt_gt, cnt_eq, w = TR.topk_loss(z, t, parts=True)
        n, k = 315, 31
        assert cnt_gt == 0 and cnt_eq == n
        assert abs(float(loss) - np.log(K)) <= 1e-14
        assert torch.allclose(w, torch.full_like(w, 1.0 / n), rtol=0, atol=1e-18) and abs(float(w.sum()) * k - k) <= 1e-12
        assert abs(float(w[0, 0, 0, 0]) - (k / n) / k) <= 1e-18   # each voxel's share of the k slots: k / n


def test_ties_at_the_threshold_share_the_remaining_weight():
    ce = torch.tensor([5.0, 4.0, 3.0, 3.0, 3.0, 2.0, 1.0, 0.0, 0.0, 0.0], dtype=torch.float64)
    t, cnt_gt, cnt_eq, w = TR.select(ce, 3)
    assert (float(t), cnt_gt, cnt_eq) == (3.0, 2, 3)
    assert torch.allclose(w, torch.tensor([1 / 3, 1 / 3, 1 / 9, 1 / 9, 1 / 9, 0, 0, 0, 0, 0], dtype=torch.float64), atol=1e-16)
    assert abs(float((w * ce).sum()) - float(torch.topk(ce, 3)[0].mean())) <= 1e-15
    with pytest.raises(ValueError):
        TR.select(ce, 0)


def test_label_smoothing_and_ignore_follow_the_issue_formula():
    torch.manual_seed(3)
    z = torch.randn(2, 4, 3, 3, 3, dtype=torch.float64)
    t = torch.randint(0, 5, (2, 1, 3, 3, 3)).float()   # label 4 = ignored
    ce = TR.ce_per_voxel(z, t, 4, 0.1)
    lp = torch.log_softmax(z, 1)
    y = t[:, 0].long().clamp(max=3)
    want = 0.9 * (-lp.gather(1, y[:, None])[:, 0]) + 0.1 / 4 * (-lp).sum(1)
    want = torch.where(t[:, 0] == 4, torch.zeros_like(want), want)
    assert float((ce - want).abs().max()) <= 1e-14 and int((ce == 0).sum()) == int((t == 4).sum()) > 0


def test_compositions_of_the_six_trainers():
    torch.manual_seed(4)
    outs = [torch.randn(2, 4, 8, 8, 8, dtype=torch.float64), torch.randn(2, 4, 4, 4, 4, dtype=torch.float64)]
    tg = [torch.randint(0, 4, (2, 1, 8, 8, 8)).float(), torch.randint(0, 4, (2, 1, 4, 4, 4)).float()]
    w = TR.variant_weights(2)
    assert np.allclose(w, [2 / 3, 1 / 3]) and np.allclose(TR.variant_weights(3), [4 / 7, 2 / 7, 1 / 7])
    lp0, lp1 = [F.cross_entropy(o, t[:, 0].long(), reduction='none') for o, t in zip(outs, tg)]
    tk = lambda c: torch.topk(c.reshape(-1), int(c.numel() * 10 / 100))[0].mean()
    got = TR.variant_loss("nnUNetTrainerTopk10LossMI355", outs, tg)
    assert abs(float(got) - float(w[0] * tk(lp0) + w[1] * tk(lp1))) <= 1e-14
    got = TR.variant_loss("nnUNetTrainerCELossMI355", outs, tg)
    assert abs(float(got) - float(w[0] * lp0.mean() + w[1] * lp1.mean())) <= 1e-14
    dice = TR.variant_loss("nnUNetTrainerDiceLossMI355", outs, tg)
    both = TR.variant_loss("nnUNetTrainerDiceTopK10LossMI355", outs, tg)
    assert abs(float(both) - float(dice) - float(TR.variant_loss("nnUNetTrainerTopk10LossMI355", outs, tg))) <= 1e-14
    ls = TR.variant_loss("nnUNetTrainerTopk10LossLS01MI355", outs, tg)
    assert float(ls) != float(TR.variant_loss("nnUNetTrainerTopk10LossMI355", outs, tg))
    ns = TR.variant_loss("nnUNetTrainerDiceCELoss_noSmoothMI355", outs, tg)
    assert abs(float(ns) - float(TR.variant_loss("nnUNetTrainerCELossMI355", outs, tg)) - float(dice)) < 1e-6   # smooth 0 vs 1e-5
    with pytest.raises(NotImplementedError):
        TR.variant_level_loss("nnUNetTrainerDiceLossMI355", ignore_label=4)
    with pytest.raises(AssertionError):
        TR.variant_level_loss("nnUNetTrainerCELossMI355", regions=[(1, 2), 2])
    # the ignore label: the CE trainers skip those voxels, the Dice of DC_and_topk is masked by them
    tg_i = [t.clone() for t in tg]
    tg_i[0][:, :, :2] = 4
    a = TR.variant_loss("nnUNetTrainerDiceTopK10LossMI355", outs, tg_i, ignore_label=4)
    o2 = [outs[0].clone(), outs[1]]
    o2[0][:, :, :2] += 3.0    # logits of ignored voxels do not matter
    assert abs(float(a) - float(TR.variant_loss("nnUNetTrainerDiceTopK10LossMI355", o2, tg_i, ignore_label=4))) <= 1e-14
