"""The float64 evaluation that tests/test_gpu_losses.py compares the device against (tests/losses_ref.py) must itself
reproduce the committed fp32 fixtures of the plain losses: loss within 1e-6 relative, gradients within 1e-5 * max|g|.
The single-process reference of the DDP batch-dice gather has no fixture; finite differences pin it.  No GPU needed."""
import numpy as np
import pytest
import torch

import losses_ref as LR
from conftest import load_npz
from oracle import loss_oracle as LO

LOSS_TOL, GRAD_TOL = 1e-6, 1e-5


def T(a):
    return torch.from_numpy(np.asarray(a))


def close(got, loss, grads, what):
    l, g = got
    lerr = abs(float(l) - float(loss)) / abs(float(loss))
    assert l.dtype == torch.float64 and lerr <= LOSS_TOL, (what, lerr)
    assert len(g) == len(grads)
    for a, b in zip(g, grads):
        b = T(b).double()
        assert a.dtype == torch.float64 and a.shape == b.shape
        err, m = float((a - b).abs().max()), float(b.abs().max())
        assert err <= GRAD_TOL * m, (what, err, m)


@pytest.mark.parametrize("bd", [0, 1])
def test_dc_ce_fixture(bd):
    z = load_npz(f"dc_ce_batchdice{bd}.npz")
    close(LR.dc_ce(T(z["logits"]), T(z["target"]), bool(bd), False, 1e-5), z["loss"], [z["glogits"]], f"dc_ce {bd}")
    counts = LR.argmax_counts(T(z["logits"]), T(z["target"]))
    for i, k in enumerate(("tp", "fp", "fn")):
        assert np.array_equal(counts[1:, i], z[k].astype(np.int64))


def test_robust_ce_fixture():
    z = load_npz("robust_ce.npz")
    close(LR.ce_only(T(z["logits"]), T(z["target"])), z["loss"], [z["glogits"]], "robust_ce")


@pytest.mark.parametrize("name", ["distill_kl_c5_T1", "distill_kl_c5_T4", "distill_kl_c1_T1", "distill_kl_c1_T4"])
def test_distill_kl_fixture(name):
    z = load_npz(name + ".npz")
    close(LR.kl(T(z["ys"]), T(z["yt"]), int(z["T"])), z["loss"], [z["gys"], z["gyt"]], name)
    only_t = LR.kl(T(z["ys"]), T(z["yt"]), int(z["T"]), need=(False, True))
    assert only_t[1][0] is None
    close((only_t[0], only_t[1][1:]), z["loss"], [z["gyt"]], name + " (teacher only)")


@pytest.mark.parametrize("name", ["feat_kl_T1", "feat_kl_T4"])
def test_feature_kl_fixture(name):
    z = load_npz(name + ".npz")
    close(LR.kl(T(z["a"]), T(z["b"]), int(z["T"]), "l2"), z["loss"], [z["ga"], z["gb"]], name)
    cl = torch.channels_last_3d       # the layout of the operand does not enter
    close(LR.kl(T(z["a"]).contiguous(memory_format=cl), T(z["b"]), int(z["T"]), "l2"), z["loss"], [z["ga"], z["gb"]], name)


def test_l2_loss_plain_fixture():
    z = load_npz("l2_loss_plain.npz")
    close(LR.mse(T(z["a"]), T(z["b"])), z["loss"], [z["ga"], z["gb"]], "l2_loss_plain")


def test_soft_cldice_fixture():
    """the scalar tail on the oracle's own fp64 skeletons, its gradients chained through the skeleton of `pred`"""
    z = load_npz("soft_cldice.npz")
    it, smooth = int(z["iter"]), float(z["smooth"])
    pred = T(z["pred"]).double().requires_grad_(True)
    sp = LO.soft_skel(pred, it)
    st = LO.soft_skel(T(z["target"]).double(), it)
    l, (d_sp, d_pr) = LR.cldice_tail(sp.detach(), T(z["target"]), st, T(z["pred"]), smooth)
    gpred = d_pr + torch.autograd.grad(sp, pred, d_sp)[0]
    close((l, [gpred]), z["loss"], [z["gpred"]], "soft_cldice")
    want = LO.soft_cldice(pred, T(z["target"]).double(), it, smooth)
    assert abs(float(l) - float(want)) <= 1e-14


@pytest.mark.parametrize("do_bg", [False, True])
def test_gathered_batch_dice_reference_against_finite_differences(do_bg):
    g = torch.Generator().manual_seed(5)
    K, shape = 3, (3, 3, 3)
    z = torch.randn((2, K, *shape), generator=g)
    zo = torch.randn((3, K, *shape), generator=g)
    t = torch.randint(0, K, (2, 1, *shape), generator=g).float()
    to = torch.randint(0, K, (3, 1, *shape), generator=g).float()
    w_ce, w_dice, mult, smooth = 0.3, 1.7, 2.0, 1e-5
    loss, (grad,), (ce, dice, gce, gdc) = LR.dc_ce_gathered(z, t, zo, to, do_bg, smooth, w_ce, w_dice, mult)
    assert float(loss) == w_ce * float(ce) + w_dice * float(dice)
    assert torch.equal(grad, w_ce * gce + mult * w_dice * gdc)
    # the Dice term is the oracle's batch Dice of the five samples, the CE term that of the two local ones
    both = LO.MemoryEfficientSoftDiceLoss(apply_nonlin=LO.softmax_helper_dim1, batch_dice=True, do_bg=do_bg, smooth=smooth)
    assert float(dice) == float(both(torch.cat([zo, z]).double(), torch.cat([to, t])))
    assert float(ce) == float(LO.RobustCrossEntropyLoss()(z.double(), t))
    h = 1e-6
    idx = torch.randint(0, z.numel(), (12,), generator=g).tolist() + [0, z.numel() - 1]
    for i in idx:
        e = torch.zeros(z.numel(), dtype=torch.float64)
        e[i] = h
        e = e.reshape(z.shape)
        up = LR.dc_ce_gathered(z.double() + e, t, zo, to, do_bg, smooth, w_ce, w_dice, mult)[2]
        dn = LR.dc_ce_gathered(z.double() - e, t, zo, to, do_bg, smooth, w_ce, w_dice, mult)[2]
        for k, (ana, name) in enumerate(((gce, "ce"), (gdc, "dice"))):
            fd = (float(up[k]) - float(dn[k])) / (2 * h)
            a = float(ana.reshape(-1)[i])
            assert abs(fd - a) <= 1e-7 * float(ana.abs().max()) + 1e-9, (name, i, fd, a)
    # another batch in front changes the local Dice gradient: the reference is not the local-only loss
    local = LR.dc_ce(z, t, True, do_bg, smooth, w_ce, w_dice)
    assert float((grad - local[1][0]).abs().max()) > 1e-3 * float(grad.abs().max())
