"""CPU tests of the HOST half of the 2-D level-set persistence (mvd_ls2d_pair_host in libmvdseg_hip.so is plain C++; the
device half -- cell keys + segmented radix sort -- is exercised by tests/test_levelset2d_gpu.py).  The keys are built and
sorted here in numpy by the kernel's formula, paired by the library and compared with the diagrams the reference's own
C++ extension and LevelSetLayer2D give (tests/golden/levelset2d_diagrams.npz, tools/make_golden_levelset2d.py)."""
import ctypes

import numpy as np
import pytest

from levelset2d_ref import counts, fixture, host_sorted_keys, pair_host, split, srt
from multimodal_mvd_seg_amd import _lib

FIX = "levelset2d_diagrams.npz"
NAMES = ["1x1", "1x5", "5x1", "2x2", "3x2", "5x4", "8x8", "7x9", "16x12", "32x32"]


def _case(name, sublevel):
    d = fixture(FIX)
    f = d[name + "/f"]
    tag = name + ("/sub" if sublevel else "/super")
    return f, bool(d[name + "/tie_free"]), d[tag + "/dgm0"], d[tag + "/dgm1"]


def test_fixture_lists_the_cases():
    assert list(fixture(FIX)["names"]) == NAMES


@pytest.mark.parametrize("sublevel", [True, False])
@pytest.mark.parametrize("name", NAMES)
def test_host_pairing_equals_reference_diagrams(name, sublevel):
    f, tie_free, want0, want1 = _case(name, sublevel)
    H, W = f.shape
    V, E, T = counts(H, W)
    bars, er = pair_host(host_sorted_keys(f, sublevel), 1, H, W, sublevel)
    d0, d1 = split(bars[0], V)
    assert d0.shape[0] == V and d1.shape[0] == T == E - V + 1          # numPairs, complex.cpp:129-131
    if H == 1 or W == 1:
        assert d1.shape[0] == 0
    # multisets of (birth, death)
    assert np.array_equal(srt(d0[:, :2]), srt(want0[:, :2])), "dgm0"
    assert np.array_equal(srt(d1[:, :2]), srt(want1[:, :2])), "dgm1"
    assert int(np.isinf(d0[:, 1]).sum()) == 1 and np.isfinite(d1).all()
    if tie_free:
        # the rows are unique: critical vertices row for row
        assert np.array_equal(srt(d0), want0) and np.array_equal(srt(d1), want1)
    # every critical vertex carries exactly the endpoint's value
    flat = f.reshape(-1)
    for d in (d0, d1):
        for col in (0, 1):
            ok = d[:, 2 + col] >= 0
            assert np.array_equal(flat[d[ok, 2 + col].astype(np.int64)], d[ok, col])
        assert (d[np.isinf(d[:, 1]), 3] == -1).all() and (d[np.isfinite(d[:, 1]), 3] >= 0).all()
    # every edge is the death of one dimension-0 bar or the birth of one dimension-1 bar
    assert np.array_equal(np.sort(er[0]), np.sort(np.concatenate([np.flatnonzero(np.isfinite(d0[:, 1])), V + np.arange(T)])))


@pytest.mark.parametrize("name", ["8x8", "7x9"])
def test_tied_fields_pair_the_same_way_twice_and_in_a_batch(name):
    f, tie_free, _, _ = _case(name, False)
    assert not tie_free
    H, W = f.shape
    keys = host_sorted_keys(f, False)
    a, ea = pair_host(keys, 1, H, W, False)
    b, eb = pair_host(keys, 1, H, W, False)
    assert np.array_equal(a, b) and np.array_equal(ea, eb)
    # 20 problems over the thread pool: problems 0, 2, ... are this field, the others its negative
    both = np.stack([keys, host_sorted_keys(-f, False)] * 10)
    c, ec = pair_host(both, 20, H, W, False)
    single, es = pair_host(both[1], 1, H, W, False)
    for p in range(20):
        assert np.array_equal(c[p], (a if p % 2 == 0 else single)[0]) and np.array_equal(ec[p], (ea if p % 2 == 0 else es)[0])


def test_maxdim0_is_the_dimension0_half():
    f, _, want0, _ = _case("16x12", True)
    H, W = f.shape
    bars, _ = pair_host(host_sorted_keys(f, True, 0), 1, H, W, True, maxdim=0)
    assert bars.shape[1] == H * W
    assert np.array_equal(srt(split(bars[0], H * W)[0]), want0)


def test_host_pairing_rejects_unsorted_and_foreign_keys():
    lib = _lib.load()
    f = np.arange(12, dtype=np.float32).reshape(3, 4)
    keys = host_sorted_keys(f, True)
    V, E, T = counts(3, 4)
    bars, er = np.zeros((V + T, 4), np.int32), np.zeros(E, np.int32)
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)
    bad = keys.copy()
    bad[[3, 4]] = bad[[4, 3]]
    assert lib.mvd_ls2d_pair_host(ptr(bad), 1, 3, 4, 1, 1, ptr(bars), ptr(er), 1) != 0
    assert b"sorted filtration" in lib.mvd_last_error()
    bad = keys.copy()
    bad[-1] |= np.uint64(0x3fffffff)             # a triangle index outside the grid
    assert lib.mvd_ls2d_pair_host(ptr(bad), 1, 3, 4, 1, 1, ptr(bars), ptr(er), 1) != 0
    assert lib.mvd_ls2d_num_cells(0, 4, 1, None, None, None) < 0 and lib.mvd_ls2d_num_cells(3, 4, 2, None, None, None) < 0
