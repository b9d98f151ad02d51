"""scipy / numpy restatement of the feed's dummy 2-D mode for tests/test_feed_dummy2d_host.py and
tests/test_gpu_feed_dummy2d.py: Convert3DTo2DTransform folds [C, D, H, W] into [C*D, H, W], batchgenerators'
augment_spatial (dim == 2) moves every slice by one in-plane map, Convert2DTo3DTransform unfolds it again
(nnUNetTrainer.py:695-717); SimulateLowResolutionTransform runs with ignore_axes=(0,).

Tolerances are those of tests/test_gpu_feed_spatial.py (check_data / check_seg), plus the bound on the excused share."""
import numpy as np
from scipy import ndimage

MAX_EXCUSED_SHARE = 1e-3  # of a case's voxels


def rotation_2d(a):
    """create_matrix_rotation_2d."""
    return np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])


def coords2d(spatial, n2, f2):
    """augment_spatial's in-plane coordinates [2, fh, fw] for spatial = (a_x, 0, 0, sc): zero-centred mesh, c . R as a row
    vector, * sc, + (n/2 - 0.5)."""
    mesh = np.array(np.meshgrid(*[np.arange(i) for i in f2], indexing='ij')).astype(float)
    for d in range(2):
        mesh[d] -= (f2[d] - 1) / 2.
    ax, ay, az, sc = spatial
    assert ay == 0 and az == 0
    c = np.dot(mesh.reshape(2, -1).transpose(), rotation_2d(ax)).transpose().reshape(mesh.shape)
    c = c * sc
    for d in range(2):
        c[d] += n2[d] / 2. - 0.5
    return c


def ref_data(x, c):
    """[C, D, H, W] -> [C, D, fh, fw]: 2-D map_coordinates(order=3, 'constant', 0) of every slice on its own."""
    return np.stack([np.stack([ndimage.map_coordinates(x[i, z].astype(np.float64), c, order=3, mode='constant', cval=0)
                               for z in range(x.shape[1])]) for i in range(x.shape[0])]).astype(np.float32)


def ref_seg(s, c):
    """interpolate_img(order=1, cval=-1, is_seg=True) per slice, then RemoveLabelTransform(-1, 0); also the fp64
    indicators' closest distance to 0.5 (ambiguous votes)."""
    out = np.zeros((*s.shape[:2], *c.shape[1:]), dtype=np.float32)
    amb = np.full(out.shape, np.inf)
    for ch in range(s.shape[0]):
        for z in range(s.shape[1]):
            for lab in np.unique(s[ch, z]):
                ind = ndimage.map_coordinates((s[ch, z] == lab).astype(float), c, order=1, mode='constant', cval=-1)
                out[ch, z][ind >= 0.5] = lab
                amb[ch, z] = np.minimum(amb[ch, z], np.abs(ind - 0.5))
    out[out == -1] = 0
    return out, amb


def face_dist(c, n2):
    return np.min(np.stack([np.minimum(np.abs(c[d]), np.abs(c[d] - (n2[d] - 1))) for d in range(2)]), 0)


def outside(c, n2):
    return np.any(np.stack([(c[d] < 0) | (c[d] > n2[d] - 1) for d in range(2)]), 0)


def mirror(a, mask):
    """MirrorTransform on the last three axes (bit 0: D, 1: H, 2: W)."""
    for ax in range(3):
        if mask & (1 << ax):
            a = np.flip(a, axis=a.ndim - 3 + ax)
    return np.ascontiguousarray(a)


def _slices(a2, D):
    return np.ascontiguousarray(np.broadcast_to(a2, (D, *a2.shape)))


def check_data(got, x, c, n2, mask):
    """got [C, D, fh, fw]: the GPU output (already mirrored) vs scipy per slice; exact cval outside, 1e-4 * max(1, max|x|)
    elsewhere except within 1e-5 voxel of a face.  Returns (max error, excused share)."""
    D = x.shape[1]
    ref = mirror(ref_data(x, c), mask)
    out = mirror(_slices(outside(c, n2), D), mask)
    fd = mirror(_slices(face_dist(c, n2), D), mask)
    assert np.all(got[:, out] == 0.0)
    excused = ~out & (fd <= 1e-5)
    share = float(excused.mean())
    ok = ~out & ~excused
    tol = 1e-4 * max(1.0, float(np.abs(x).max()))
    err = np.abs(got - ref)[:, ok]
    worst = float(err.max()) if err.size else 0.0
    print(f"data: max err {worst:.3e} (tol {tol:.3e}), excused share {share:.2e}, outside {out.mean():.2f}")
    assert share <= MAX_EXCUSED_SHARE, share
    assert worst <= tol, worst
    return worst, share


def check_seg(got, s, c, n2, mask):
    """Exact, except votes within 1e-5 of 0.5 and positions within 1e-5 voxel of a face; that excused set may hold at
    most 0.1 % of the voxels.  Returns the excused share."""
    D = s.shape[1]
    ref, amb = ref_seg(s, c)
    ref, amb = mirror(ref, mask), mirror(amb, mask)
    fd = mirror(_slices(face_dist(c, n2), D), mask)
    bad = got != ref
    excused = (amb <= 1e-5) | (fd[None] <= 1e-5)
    share = float(excused.mean())
    print(f"seg: mismatches {int(bad.sum())}, unexcused {int((bad & ~excused).sum())}, excused share {share:.2e}")
    assert share <= MAX_EXCUSED_SHARE, share
    assert not np.any(bad & ~excused), int((bad & ~excused).sum())
    assert bad.sum() < 1e-4 * bad.size + 1
    return share


def replay_spatial_2d(p_rot, p_scale, rot, scale, p_axis=1.0):
    """augment_spatial's draws for one sample with dim == 2 (restated): the y / z axis draws sit inside `if dim == 3`.
    Returns (spatial or None, number of draws)."""
    n, a_x, sc, mod = 0, 0., 1., False
    u = np.random.uniform(); n += 1
    if u < p_rot:
        u = np.random.uniform(); n += 1
        if u <= p_axis:
            a_x = np.random.uniform(*rot['x']); n += 1
        mod = True
    u = np.random.uniform(); n += 1
    if u < p_scale:
        r = np.random.random(); n += 1
        if r < 0.5 and scale[0] < 1:
            sc = np.random.uniform(scale[0], 1)
        else:
            sc = np.random.uniform(max(scale[0], 1), scale[1])
        n += 1
        mod = True
    return ((float(a_x), 0., 0., float(sc)) if mod else None), n


def lowres_inplane(x, z):
    """augment_linear_downsampling_scipy(order_downsample=0, order_upsample=3, ignore_axes=(0,)) of one channel [D, H, W]:
    target_shape[0] = shape[0]; skimage resize == scipy zoom(mode='nearest', grid_mode=True) over the 3-D array with a unit
    factor on axis 0, then the clip to the downsampled range.  Returns (result, downsampled)."""
    shp = np.asarray(x.shape)
    t = np.maximum(np.round(shp * z).astype(int), 1)
    t[0] = shp[0]
    d = ndimage.zoom(x.astype(np.float64), t / shp, order=0, mode='nearest', grid_mode=True)
    assert tuple(d.shape) == tuple(t)
    up = ndimage.zoom(d, shp / t, order=3, mode='nearest', grid_mode=True)
    assert up.shape == x.shape
    return np.clip(up, d.min(), d.max()), d
