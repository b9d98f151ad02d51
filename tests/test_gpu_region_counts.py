"""GPU tests of the online-evaluation counts for region heads and for the ignore label (mvd_sigmoid_counts,
mvd_argmax_counts_masked; nnUNetTrainer.py:969-1002) against numpy, in every integer."""
import numpy as np
import pytest
import torch

import region_loss_ref as RR
from multimodal_mvd_seg_amd import ops

DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu
REGIONS = [(1, 2, 3), (2, 3), 3]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from multimodal_mvd_seg_amd import _lib
    _lib.load()


def make(seed, N, C, shape, nlab):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn((N, C, *shape), generator=g) * 2
    seg = torch.randint(0, nlab, (N, 1, *shape), generator=g).float()
    return z, seg


@pytest.mark.parametrize("ignore", [None, 4])
@pytest.mark.parametrize("shape", [(5, 7, 9), (64, 65, 67)])
def test_sigmoid_counts(shape, ignore):
    z, seg = make(1, 2, 3, shape, 4 if ignore is None else 5)
    z.view(-1)[::7] = 0.0                 # logits exactly 0: sigmoid = 0.5, not predicted
    z.view(-1)[3::11] = -0.0
    planes = RR.seg_to_regions(seg.numpy(), REGIONS, ignore)
    want = RR.sigmoid_counts(z.numpy(), planes, ignore is not None)
    # the same through torch's own expression on these logits (none lies in (0, 1.2e-7))
    pred = (torch.sigmoid(z) > 0.5).numpy()
    assert np.array_equal(pred, z.numpy() > 0)
    got = ops.sigmoid_counts(z.to(DEV), seg.to(DEV), REGIONS, ignore).cpu().numpy()
    assert got.dtype == np.int64 and np.array_equal(got, want), (got, want)
    got = ops.sigmoid_counts(z.to(DEV), torch.from_numpy(planes).to(DEV), has_ignore_plane=ignore is not None).cpu().numpy()
    assert np.array_equal(got, want)


@pytest.mark.parametrize("R", [1, 8])
def test_sigmoid_counts_head_counts(R):
    regions = [tuple(range(r + 1, R + 2)) for r in range(R)]
    z, seg = make(2, 3, R, (11, 13, 6), R + 3)
    planes = RR.seg_to_regions(seg.numpy(), regions, R + 2)
    got = ops.sigmoid_counts(z.to(DEV), seg.to(DEV), regions, R + 2).cpu().numpy()
    assert np.array_equal(got, RR.sigmoid_counts(z.numpy(), planes, True))


@pytest.mark.parametrize("K", [2, 5])
@pytest.mark.parametrize("shape", [(5, 7, 9), (64, 65, 67)])
def test_argmax_counts_masked(shape, K):
    z, seg = make(3, 2, K, shape, K + 1)
    z[:, 1] = z[:, 0]                      # exact ties: the first maximum wins
    got = ops.argmax_counts_masked(z.to(DEV), seg.to(DEV), K).cpu().numpy()
    want = RR.argmax_counts_masked(z.numpy(), seg.numpy(), K)
    assert got.dtype == np.int64 and np.array_equal(got, want), (got, want)
    # nothing ignored: the unmasked kernel's counts
    seg2 = seg.clamp(max=K - 1)
    assert np.array_equal(ops.argmax_counts_masked(z.to(DEV), seg2.to(DEV), K).cpu().numpy(),
                          ops.argmax_counts(z.to(DEV), seg2.to(DEV)).cpu().numpy())


def test_all_ignored_batch_counts_nothing():
    z, seg = make(4, 2, 3, (9, 8, 7), 4)
    seg[:] = 4
    assert not ops.sigmoid_counts(z.to(DEV), seg.to(DEV), REGIONS, 4).cpu().numpy().any()
    z4, _ = make(5, 2, 4, (9, 8, 7), 4)
    assert not ops.argmax_counts_masked(z4.to(DEV), seg.to(DEV), 4).cpu().numpy().any()
