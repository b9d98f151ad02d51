"""GPU tests of the cascade stage's kernels (csrc/feed_cascade.hip): exact equality against scipy.ndimage
through tests/cascade_ref.py."""
import numpy as np
import pytest
import torch

import cascade_ref as REF
from multimodal_mvd_seg_amd import dataloading as DLD

DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def gpu_morph(planes, steps, return_bits=False):
    """planes bool [K,D,H,W]; steps (c, op, radius) -> the planes after pack, the steps in turn, unpack."""
    K, shape = planes.shape[0], planes.shape[1:]
    x = G(planes.astype(np.float32))
    bits = DLD.cascade_bitplanes(K, shape, DEV)
    tmp = DLD.cascade_bitplanes(2, shape, DEV)
    DLD.cascade_pack(x, bits)
    for c, op, radius in steps:
        DLD.cascade_morph(bits, tmp, K, shape, c, op, DLD.ball_rows(radius))
    out = torch.full_like(x, 7.0)
    DLD.cascade_unpack(bits, out)
    o = out.cpu().numpy()
    assert np.isin(o, (0.0, 1.0)).all()
    return (o != 0, bits.cpu().numpy()) if return_bits else o != 0


SHAPES = [(3, 5, 5), (9, 10, 37), (6, 7, 64), (5, 6, 70), (17, 18, 130), (4, 20, 128)]
RADII = [1.0, 1.5, 2.3, 3.7, 7.99]
DENSITIES = [0.05, 0.5, 0.95]


def contents(shape):
    """name -> mask; the random masks hold at least one set and one clear voxel away from each other, so that scipy's
    dilation and erosion both change them at every radius (asserted on the oracle in the test)."""
    rng = np.random.default_rng(sum(shape))
    out = {}
    for d in DENSITIES:
        m = rng.random(shape) < d
        m.flat[0], m.flat[-1] = True, False
        out[f"random{d}"] = m
    out["empty"] = np.zeros(shape, dtype=bool)
    out["full"] = np.ones(shape, dtype=bool)
    faces = np.zeros(shape, dtype=bool)
    faces[0] = faces[-1] = True
    faces[:, 0] = faces[:, -1] = True
    faces[:, :, 0] = faces[:, :, -1] = True
    out["faces"] = faces
    return out


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("shape", SHAPES)
def test_every_operator_matches_scipy(shape, radius):
    for name, m in contents(shape).items():
        for op in range(4):
            want = REF.morph_op(m, op, radius)
            got, bits = gpu_morph(m[None], [(0, op, radius)], return_bits=True)
            assert np.array_equal(got[0], want), (name, REF.OPS[op])
            if name.startswith("random") and op < 2:
                assert not np.array_equal(want, m), "vacuous case: the oracle leaves the mask unchanged"
            if shape[2] % 64:  # the pad bits of the last word stay clear
                last = bits.view(np.uint64).reshape(shape[0], shape[1], -1)[:, :, -1]
                assert not (last >> np.uint64(shape[2] % 64)).any(), (name, REF.OPS[op])
    full = np.ones(shape, dtype=bool)
    assert gpu_morph(full[None], [(0, 1, radius)])[0].all()    # border_value=True keeps a full plane full
    assert gpu_morph(full[None], [(0, 0, radius)])[0].all()    # and the dilation neither leaks nor loses anything


@pytest.mark.parametrize("radius", [7.154414195618729, 5.602586713613308, 6.4, 4.881776316810024, 3.5, 7.0])
def test_radii_whose_grid_points_lie_on_the_sphere(radius):
    """Odd and even sides between the tabulated ones; at n = 15 the points (2, 3, 6) / 7 of r lie exactly on the sphere,
    where the host table must round as the ball does."""
    shape = (12, 16, 66)
    m = _onehot_planes(shape, 3, 2)[0]
    for op in range(4):
        want = REF.morph_op(m, op, radius)
        assert np.array_equal(gpu_morph(m[None], [(0, op, radius)])[0], want), REF.OPS[op]
    assert not np.array_equal(REF.morph_op(m, 0, radius), m) and not np.array_equal(REF.morph_op(m, 1, radius), m)


def test_even_sided_element_offsets():
    """ball(1.5) is 4^3 with the 8 voxels {1,2}^3; scipy centres it at index 2: a voxel dilates to offsets {-1, 0}, a hole
    erodes to offsets {0, +1}."""
    m = np.zeros((7, 7, 70), dtype=bool)
    m[3, 3, 64] = True
    got = gpu_morph(m[None], [(0, 0, 1.5)])[0]
    assert sorted(map(tuple, np.argwhere(got) - (3, 3, 64))) == sorted(
        (a, b, c) for a in (-1, 0) for b in (-1, 0) for c in (-1, 0))
    got = gpu_morph(~m[None], [(0, 1, 1.5)])[0]
    assert sorted(map(tuple, np.argwhere(~got) - (3, 3, 64))) == sorted(
        (a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1))


def _onehot_planes(shape, K, seed):
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, K + 1, [-(-s // 3) for s in shape])  # 3^3 blocks rather than salt and pepper
    lab = coarse.repeat(3, 0).repeat(3, 1).repeat(3, 2)[:shape[0], :shape[1], :shape[2]]
    return np.stack([lab == k + 1 for k in range(K)])


def test_added_voxel_rule_and_shuffled_order():
    shape = (10, 12, 70)
    planes = _onehot_planes(shape, 3, 1)
    # a voxel set in BOTH other channels that the dilation of channel 0 adds
    z, y, x = np.argwhere(REF.morph_op(planes[0], 0, 2.3) & ~planes[0])[0]
    planes[1, z, y, x] = planes[2, z, y, x] = True
    steps = [(2, 0, 2.3), (0, 0, 2.3), (1, 2, 3.7), (0, 3, 1.5), (2, 1, 1.0)]   # a shuffled channel order, all operators
    want = planes.copy()
    first = planes.copy()
    REF.apply_operator(first, 0, 0, 2.3)
    assert not first[1, z, y, x] and not first[2, z, y, x] and first[0, z, y, x]
    got1 = gpu_morph(planes, [(0, 0, 2.3)])
    assert np.array_equal(got1, first)
    for c, op, r in steps:
        REF.apply_operator(want, c, op, r)
    got, bits = gpu_morph(planes, steps, return_bits=True)
    assert np.array_equal(got, want)
    assert not np.array_equal(want, planes)
    again, bits2 = gpu_morph(planes, steps, return_bits=True)
    assert np.array_equal(bits, bits2)    # two identical calls give equal bits


def test_pack_unpack_roundtrip_and_layout():
    rng = np.random.default_rng(5)
    for shape in SHAPES:
        m = rng.random((2, *shape)) < 0.5
        got, bits = gpu_morph(m, [], return_bits=True)
        assert np.array_equal(got, m)
        Wq = -(-shape[2] // 64)
        b = bits.view(np.uint64).reshape(2, shape[0], shape[1], Wq)
        x = np.arange(shape[2])
        assert np.array_equal(((b[..., x // 64] >> (x % 64).astype(np.uint64)) & np.uint64(1)).astype(bool), m)


# ------------------------------------------------------------------------------------------------ one-hot move
@pytest.mark.parametrize("labels", [(1, 2, 3), (2, 5)])
def test_onehot_move_after_the_mirrored_padded_store(labels):
    """Seg channel 1 as the feed stores it: cropped with an overhang (pad -1 -> 0), mirrored; then the one-hot planes."""
    rng = np.random.default_rng(len(labels))
    seg = rng.integers(0, 6, (2, 9, 11, 13)).astype(np.int16)
    patch, lbs = (8, 12, 70), (-2, 3, -30)
    for mask in (0, 5, 7):
        stored = torch.empty((2, *patch), dtype=torch.float32, device=DEV)
        DLD.crop_pad_seg(G(seg), stored, lbs, mask, -1, replace=(-1, 0))
        out = torch.full((len(labels), *patch), 7.0, dtype=torch.float32, device=DEV)
        DLD.cascade_onehot(stored[1], out, labels)
        # oracle: numpy crop / pad / mirror of channel 1
        pad = np.full(patch, -1, dtype=np.int64)
        for z in range(patch[0]):
            for y in range(patch[1]):
                sz, sy = lbs[0] + z, lbs[1] + y
                if 0 <= sz < 9 and 0 <= sy < 11:
                    xs = np.arange(patch[2]) + lbs[2]
                    ok = (xs >= 0) & (xs < 13)
                    pad[z, y, ok] = seg[1, sz, sy, xs[ok]]
        pad[pad == -1] = 0
        for ax in range(3):
            if mask & (1 << ax):
                pad = np.flip(pad, ax)
        want = REF.move_seg_as_onehot(pad, labels)
        assert (pad == 0).sum() > (seg[1] == 0).sum()     # the pad region is there
        assert np.array_equal(out.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ removal
def gpu_remove(chan, u, other=None, fraction=0.15):
    shape = chan.shape
    x = G(chan.astype(np.float32))
    o = None if other is None else G(other.astype(np.float32))
    ws = DLD.cascade_remove_workspace(shape, DEV)
    chosen = torch.full((2,), -5, dtype=torch.int32, device=DEV)
    DLD.cascade_remove(x, u, DLD.cascade_removal_threshold(int(np.prod(shape)), fraction), ws, chosen, other=o)
    return x.cpu().numpy(), (None if o is None else o.cpu().numpy()), chosen.cpu().numpy()


def removal_mask():
    """20^3: a 1200-voxel component (never removable: 8000 * 0.15 == 1200.0), an 1199-voxel one, and many small ones."""
    m = np.zeros((20, 20, 20), dtype=bool)
    m[0:6, 0:10, 0:20] = True                 # 1200
    assert m.sum() == 1200
    m[8:14, 0:10, 0:20] = True
    m[13, 9, 19] = False                      # 1199
    rng = np.random.default_rng(9)
    small = rng.random((5, 9, 20)) < 0.08     # isolated specks and small clusters
    m[15:20, 11:20, :] = small
    m[16, 0:8, 0:3] = True                    # a 24-voxel bar
    return m


def test_removal_threshold_edge_and_picks():
    m = removal_mask()
    lab, sizes = REF.label_with_component_sizes(m)
    assert 1200 in sizes.values() and 1199 in sizes.values()
    valid = [i for i, s in sizes.items() if s < 1200]
    assert len(valid) > 20 and len(sizes) == len(valid) + 1
    big_ordinal = valid.index([i for i, s in sizes.items() if s == 1199][0])
    us = [0.0, np.nextafter(1.0, 0.0), 0.5, (big_ordinal + 0.5) / len(valid)]
    seen = set()
    for u in us:
        want = m.astype(np.float32)
        ordinal, n_valid = REF.remove_component(want, u=u)
        got, _, chosen = gpu_remove(m, u)
        assert np.array_equal(got, want), u
        assert chosen[1] == n_valid == len(valid)
        assert chosen[0] == 1 + np.flatnonzero(lab.ravel() == valid[ordinal])[0]
        assert (got != m).sum() == sizes[valid[ordinal]]
        seen.add(ordinal)
    assert seen == {0, len(valid) - 1, len(valid) // 2, big_ordinal}
    # the 1200-voxel component survives every possible pick
    for k in range(len(valid)):
        got, _, _ = gpu_remove(m, (k + 0.5) / len(valid))
        assert got[0:6, 0:10, 0:20].all()


def test_removal_is_a_noop_without_a_valid_component():
    m = np.zeros((20, 20, 20), dtype=bool)
    m[0:6, 0:10, 0:20] = True
    for mask in (m, np.zeros_like(m)):
        other = np.zeros_like(mask)
        got, o, chosen = gpu_remove(mask, 0.7, other=other)
        assert np.array_equal(got, mask.astype(np.float32)) and not o.any()
        assert tuple(chosen) == (0, 0)


def test_removal_fills_the_other_class_and_repeats_bit_for_bit():
    m = removal_mask()
    other = np.zeros_like(m)
    other[19, 19, 19] = True
    want, wo = m.astype(np.float32), other.astype(np.float32)
    REF.remove_component(want, u=0.31, other=wo)
    got, o, chosen = gpu_remove(m, 0.31, other=other)
    assert np.array_equal(got, want) and np.array_equal(o, wo)
    assert (o != other).any()
    got2, o2, chosen2 = gpu_remove(m, 0.31, other=other)
    assert np.array_equal(got, got2) and np.array_equal(o, o2) and np.array_equal(chosen, chosen2)


def test_removal_roots_span_several_counting_workgroups():
    """24 x 24 x 40 = 23040 voxels: the counting kernel runs 23 workgroups of about 1000 voxels; isolated voxels on a
    lattice put roots into ten of them; picks in the first, a middle and the last one."""
    m = np.zeros((24, 24, 40), dtype=bool)
    m[::4, ::4, ::5] = True
    n = int(m.sum())
    assert n == 6 * 6 * 8
    idx = np.flatnonzero(m.ravel())
    assert len(set(idx // 1002)) >= 10
    for k in (0, 1, 37, 144, n - 2, n - 1):
        got, _, chosen = gpu_remove(m, (k + 0.5) / n)
        assert tuple(chosen) == (idx[k] + 1, n)
        want = m.copy()
        want.ravel()[idx[k]] = False
        assert np.array_equal(got != 0, want)
