"""CPU tests that pin tests/region_loss_ref.py, the fp64 restatement the region / ignore-label kernels are compared with
(DESIGN 17): with nothing ignored the masked forms equal the unmasked ones, the masked softmax form equals the oracle's
DC+CE, and the analytic gradient of mvd_dcbce_bwd equals autograd.  Equalities to 1e-12 relative."""
import numpy as np
import pytest
import torch

import region_loss_ref as RR
from oracle import loss_oracle as LO

REGIONS = [(1, 2, 3), (2, 3), 3]


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def case(seed, N=2, R=3, shape=(5, 6, 7), nlab=4):
    g = torch.Generator().manual_seed(seed)
    z = (torch.randn((N, R, *shape), generator=g, dtype=torch.float64) * 3)
    seg = torch.randint(0, nlab, (N, 1, *shape), generator=g).float()
    return z, seg


@pytest.mark.parametrize("batch_dice", [False, True])
def test_all_valid_mask_equals_unmasked_bce(batch_dice):
    z, seg = case(1)
    planes = torch.from_numpy(RR.seg_to_regions(seg.numpy(), REGIONS))
    plain = RR.dc_and_bce(z, planes, batch_dice=batch_dice, parts=True)
    withm = RR.dc_and_bce(z, torch.cat([planes, torch.zeros_like(planes[:, :1])], 1), use_ignore_label=True,
                          batch_dice=batch_dice, parts=True)
    # the Dice parts are equal; upstream's masked BCE divides by voxels, not voxels x heads (mirrored, not "fixed")
    assert rel(withm[2], plain[2]) < 1e-12
    assert rel(withm[1], plain[1] * z.shape[1]) < 1e-12


@pytest.mark.parametrize("batch_dice", [False, True])
@pytest.mark.parametrize("K", [2, 5])
def test_masked_ce_without_ignored_voxels_equals_the_oracle(K, batch_dice):
    z, seg = case(2, R=K, nlab=K)
    want = LO.DC_and_CE_loss({'batch_dice': batch_dice, 'smooth': 1e-5, 'do_bg': False, 'ddp': False}, {})(z, seg)
    assert rel(RR.dc_and_ce_masked(z, seg, None, batch_dice=batch_dice), want) < 1e-12
    assert rel(RR.dc_and_ce_masked(z, seg, K, batch_dice=batch_dice), want) < 1e-12   # label K never occurs
    # and with ignored voxels it is the oracle's own ignore_label branch
    seg[:, :, :2] = K
    want = LO.DC_and_CE_loss({'batch_dice': batch_dice, 'smooth': 1e-5, 'do_bg': False, 'ddp': False}, {},
                             ignore_label=K)(z, seg)
    assert rel(RR.dc_and_ce_masked(z, seg, K, batch_dice=batch_dice), want) < 1e-12


def test_masked_ce_with_every_voxel_ignored_is_finite():
    z, seg = case(3, R=3, nlab=3)
    seg[:] = 3
    total, ce, dice = RR.dc_and_ce_masked(z, seg, 3, parts=True)
    assert float(ce) == 0.0 and np.isfinite(float(total))


@pytest.mark.parametrize("use_ignore", [False, True])
@pytest.mark.parametrize("batch_dice", [False, True])
@pytest.mark.parametrize("do_bg", [True, False])
def test_analytic_region_gradient_equals_autograd(use_ignore, batch_dice, do_bg):
    z, seg = case(4, nlab=5 if use_ignore else 4)
    planes = torch.from_numpy(RR.seg_to_regions(seg.numpy(), REGIONS, 4 if use_ignore else None))
    z.requires_grad_(True)
    RR.dc_and_bce(z, planes, use_ignore_label=use_ignore, batch_dice=batch_dice, do_bg=do_bg, w_ce=0.7, w_dice=1.3).backward()
    got = RR.region_grad_formula(z.detach(), planes, use_ignore, batch_dice, do_bg, w_ce=0.7, w_dice=1.3)
    assert rel(got, z.grad) < 1e-12


def test_label_map_and_plane_targets_agree():
    z, seg = case(5, nlab=5)
    a = RR.dc_and_bce_labelmap(z, seg, REGIONS, 4)
    b = RR.dc_and_bce(z, torch.from_numpy(RR.seg_to_regions(seg.numpy(), REGIONS, 4)), use_ignore_label=True)
    assert float(a) == float(b)


def test_count_models_match_the_oracle_counts():
    z, seg = case(6, R=4, nlab=4)
    tp, fp, fn = LO.validation_counts(z.float(), seg)
    got = RR.argmax_counts_masked(z.float().numpy(), seg.numpy(), ignore_label=99)
    assert np.array_equal(got[1:, 0], tp) and np.array_equal(got[1:, 1], fp) and np.array_equal(got[1:, 2], fn)
    zz = z[:, :3].float()
    zz[0, 0, 0, 0, :3] = 0.0   # exactly 0: sigmoid is 0.5, not > 0.5
    planes = RR.seg_to_regions(seg.numpy(), REGIONS)
    pred = (torch.sigmoid(zz) > 0.5).float()
    tp, fp, fn, _ = LO.get_tp_fp_fn_tn(pred, torch.from_numpy(planes), axes=[0, 2, 3, 4])
    got = RR.sigmoid_counts(zz.numpy(), planes)
    assert np.array_equal(got, torch.stack([tp, fp, fn], 1).long().numpy())
