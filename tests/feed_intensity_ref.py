"""fp64 numpy / scipy restatement of the feed's intensity stage, for the tests.

Each function is the numeric core of one batchgenerators transform with nnU-Net's arguments (nnUNetTrainer.py:719-736),
applied to one channel or one sample [C,D,H,W] in the reference's (un-mirrored) orientation.  `chain` runs a whole
sample's plan entry in the reference order and re-mirrors, so its result compares with what the loader stores.
"""
import numpy as np
from scipy import ndimage

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)
_M32 = np.uint64(0xFFFFFFFF)


def _mulhilo(a, b):
    """64 x 64 -> 128-bit products of uint64 arrays: (hi, lo)."""
    a0, a1 = a & _M32, a >> np.uint64(32)
    b0, b1 = b & _M32, b >> np.uint64(32)
    p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    mid = (p00 >> np.uint64(32)) + (p01 & _M32) + (p10 & _M32)
    hi = p11 + (p01 >> np.uint64(32)) + (p10 >> np.uint64(32)) + (mid >> np.uint64(32))
    return hi, a * b


def philox_raw(key, n):
    """The first n outputs of numpy.random.Philox(key=key).random_raw(): Philox4x64-10 of the counters 1, 2, ... (numpy
    increments the counter before each block of 4 words)."""
    key = int(key)
    with np.errstate(over='ignore'):
        nb = (n + 3) // 4
        c = [np.arange(1, nb + 1, dtype=np.uint64), np.zeros(nb, np.uint64), np.zeros(nb, np.uint64),
             np.zeros(nb, np.uint64)]
        k0, k1 = np.uint64(key & 0xFFFFFFFFFFFFFFFF), np.uint64(key >> 64)
        m0, m1 = np.uint64(0xD2E7470EE14C6C93), np.uint64(0xCA5A826395121157)
        for r in range(10):
            if r:
                k0, k1 = k0 + np.uint64(0x9E3779B97F4A7C15), k1 + np.uint64(0xBB67AE8584CAA73B)
            hi0, lo0 = _mulhilo(np.full(nb, m0), c[0])
            hi1, lo1 = _mulhilo(np.full(nb, m1), c[2])
            c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
    return np.stack(c, 1).reshape(-1)[:n]


def normals(key, n):
    """The device's N(0, 1) field: Box-Muller of the raw words (include/mvdseg_hip.h)."""
    w = philox_raw(key, n)
    u1 = (2.0 * (w >> np.uint64(41)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (2.0 * ((w >> np.uint64(18)) & np.uint64(0x7FFFFF)).astype(np.float64) + 1.0) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def mirror(a, mask):
    for ax in range(3):
        if mask & (1 << ax):
            a = np.flip(a, axis=a.ndim - 3 + ax)
    return np.ascontiguousarray(a)


def noise_field(key, shape, flip_mask):
    """The field the device adds to a sample of `shape` [C,D,H,W], in the reference orientation (it is drawn per
    STORED voxel, i.e. after the mirror)."""
    return mirror(normals(key, int(np.prod(shape))).reshape(shape), flip_mask)


def blur(x, sigma):
    return ndimage.gaussian_filter(x.astype(np.float64), sigma, order=0, mode='reflect', truncate=4.0)


def contrast(x, f):
    mn, lo, hi = x.mean(), x.min(), x.max()
    return np.clip((x - mn) * f + mn, lo, hi)


def target_shape(shape, z):
    return np.maximum(np.round(np.asarray(shape) * z).astype(int), 1)


def lowres(x, z):
    """augment_linear_downsampling_scipy(order_downsample=0, order_upsample=3) of one channel: skimage resize(mode='edge',
    anti_aliasing=False, clip=True) == scipy zoom(mode='nearest', grid_mode=True) + the clip to the input's range."""
    shp = np.asarray(x.shape)
    t = target_shape(shp, z)
    d = ndimage.zoom(x.astype(np.float64), t / shp, order=0, mode='nearest', grid_mode=True)
    assert tuple(d.shape) == tuple(t)
    up = ndimage.zoom(d, shp / t, order=3, mode='nearest', grid_mode=True)
    assert up.shape == x.shape
    return np.clip(up, d.min(), d.max()), d


def gamma(x, g, invert=False):
    """augment_gamma(retain_stats=True, epsilon=1e-7) of one channel."""
    x = -x if invert else x.astype(np.float64)
    mn, sd = x.mean(), x.std()
    lo = x.min()
    r = x.max() - lo
    y = np.power((x - lo) / (r + 1e-7), g) * (r + 1e-7) + lo
    y = y - y.mean()
    y = y / (y.std() + 1e-8) * sd + mn
    return -y if invert else y


def chain(x, it, flip_mask):
    """One sample's intensity plan entry (dataloading.draw_intensity) on x [C,D,H,W] as the loader stores it (mirrored
    on flip_mask): un-mirror, run noise -> blur -> brightness -> contrast -> low-res -> gamma (inverted) -> gamma in fp64,
    mirror again."""
    x = mirror(x.astype(np.float64), flip_mask)
    C = x.shape[0]
    if it['noise'] is not None:
        sigma, key = it['noise']
        x = x + sigma * noise_field(key, x.shape, flip_mask)
    if it['blur'] is not None:
        x = np.stack([blur(x[c], s) if s is not None else x[c] for c, s in enumerate(it['blur'])])
    if it['brightness'] is not None:
        x = x * np.asarray(it['brightness'])[:, None, None, None]
    if it['contrast'] is not None:
        x = np.stack([contrast(x[c], it['contrast'][c]) for c in range(C)])
    if it['lowres'] is not None:
        x = np.stack([lowres(x[c], z)[0] if z is not None else x[c] for c, z in enumerate(it['lowres'])])
    if it['gamma_inverted'] is not None:
        x = np.stack([gamma(x[c], g, True) for c, g in enumerate(it['gamma_inverted'])])
    if it['gamma'] is not None:
        x = np.stack([gamma(x[c], g) for c, g in enumerate(it['gamma'])])
    return mirror(x, flip_mask)


def mask(x, seg, channels):
    """MaskTransform(channels, mask_idx_in_seg=0, set_outside_to=0) on a sample, seg [Cs,D,H,W] before RemoveLabel."""
    x = x.copy()
    for c in channels:
        x[c][seg[0] < 0] = 0
    return x
