"""CPU check that the logits of tests/test_gpu_region_export.py stay under that test's cap by the oracle alone: the share
of voxels with a head's fp64 interpolated logit inside (-1e-4, 1e-4) is at most 1e-3 (std 8 clipped to +-64)."""
import numpy as np
import pytest

import export_ref as REF

CASES = [((37, 45, 52), (61, 83, 70), None), ((37, 45, 52), (20, 31, 40), None), ((37, 45, 52), (61, 83, 70), 0),
         ((37, 45, 52), (61, 83, 70), 2), ((10, 13, 17), (15, 21, 19), None)]


@pytest.mark.parametrize("shape,new,axis", CASES)
def test_test_logits_stay_under_the_cap(shape, new, axis):
    x = REF.smooth_logits(3, shape, seed=0 if shape[0] == 37 else 7)
    res = REF.resample_logits(x, new, axis)
    share = float((np.abs(res).min(0) < 1e-4).mean())
    print(f"{shape}->{new} sep-z {axis}: share under the margin {share:.2e}")
    assert share <= 1e-3
