"""fp64 numpy / scipy restatement of the feed's DA5 stage, for the tests.

Each function is the numeric core of one transform of nnUNetTrainerDA5.get_training_transforms on one channel [D,H,W] or
one sample [C,D,H,W]; `chain` runs one sample's entries of a dataloading.draw_da5 plan in the reference order on the
stage's input (the un-mirrored crop / warp result).  Blur, low-res, gamma, noise and mask come from feed_intensity_ref.
"""
import numpy as np
from scipy import ndimage, signal

import feed_intensity_ref as IREF


def median(x, s):
    return ndimage.median_filter(x, size=int(s), mode='reflect')


def median_brute(x, s):
    """The window i - s//2 .. i + (s-1) - s//2 per axis over the symmetric padding, sorted; rank s^3 // 2."""
    s = int(s)
    lo, hi = s // 2, s - 1 - s // 2
    p = np.pad(x, [(lo, hi)] * 3, mode='symmetric')
    out = np.empty_like(x)
    for z in range(x.shape[0]):
        for y in range(x.shape[1]):
            for w in range(x.shape[2]):
                out[z, y, w] = np.sort(p[z:z + s, y:y + s, w:w + s].ravel())[s ** 3 // 2]
    return out


def sharpen(x, strength):
    x = x.astype(np.float64)
    k = np.zeros((3, 3, 3))
    k[1, 1, 1] = 6
    for ax in range(3):
        for o in (0, 2):
            idx = [1, 1, 1]
            idx[ax] = o
            k[tuple(idx)] = -1
    k = k * strength
    k[1, 1, 1] += 1
    return np.clip(signal.convolve(x, k, mode='same'), x.min(), x.max())


def gauss_field(shape, scale, loc):
    g = np.ones(shape)
    for d in range(3):
        i = np.arange(shape[d], dtype=np.float64)
        e = np.exp(-(i - loc[d]) ** 2 / (2 * scale[d] ** 2))
        g = g * e.reshape([-1 if a == d else 1 for a in range(3)])
    return g / g.max()


def gradient(x, scale, loc, amount):
    return x.astype(np.float64) + amount * gauss_field(x.shape, scale, loc)


def local_gamma(x, scale, loc, amount):
    x = x.astype(np.float64)
    mn, mx = x.min(), x.max()
    x01 = (x - mn) / max(mx - mn, 1e-8)
    return x01 ** (1 + (amount - 1) * gauss_field(x.shape, scale, loc)) * (mx - mn) + mn


def blank(x, rects):
    x = x.astype(np.float64).copy()
    for lb, size in rects:
        sl = tuple(slice(l, l + s) for l, s in zip(lb, size))
        x[sl] = x[sl].mean()
    return x


def contrast_noclip(x, f):
    x = x.astype(np.float64)
    return (x - x.mean()) * f + x.mean()


def signed(x, rot90=None, transpose=None, flip_mask=0):
    """Rot90Transform, TransposeAxesTransform and the mirror on the spatial axes of x [C,D,H,W]."""
    if rot90 is not None:
        x = np.rot90(x, rot90[0], tuple(a + 1 for a in rot90[1]))
    if transpose is not None:
        x = np.transpose(x, (0, *[a + 1 for a in transpose]))
    return IREF.mirror(x, flip_mask)


def per_channel(x, vals, fn):
    return np.stack([fn(x[c], v) if v is not None else x[c] for c, v in enumerate(vals)])


def chain(x, d, j):
    x = signed(x.astype(np.float64), d['rot90'][j], d['transpose'][j])
    if d['median'][j] is not None:
        x = per_channel(x, d['median'][j], median)
    if d['blur'][j] is not None:
        x = per_channel(x, d['blur'][j], IREF.blur)
    if d['noise'][j] is not None:
        sigma, key = d['noise'][j]
        x = x + sigma * IREF.noise_field(key, x.shape, 0)
    if d['brightness'][j] is not None:
        x = per_channel(x, d['brightness'][j], lambda a, v: a + v)
    if d['contrast'][j] is not None:
        x = per_channel(x, d['contrast'][j], IREF.contrast if d['oneof_contrast'] == 0 else contrast_noclip)
    if d['lowres'][j] is not None:
        x = per_channel(x, d['lowres'][j], lambda a, z: IREF.lowres(a, z)[0])
    for key in ('gamma1', 'gamma2'):
        if d[key][j] is not None:
            x = per_channel(x, d[key][j], lambda a, g: IREF.gamma(a, g, True))
    x = IREF.mirror(x, d['mirror'][j])
    if d['blank'][j] is not None:
        x = per_channel(x, d['blank'][j], blank)
    if d['gradient'][j] is not None:
        x = per_channel(x, d['gradient'][j], lambda a, p: gradient(a, *p))
    if d['local_gamma'][j] is not None:
        x = per_channel(x, d['local_gamma'][j], lambda a, p: local_gamma(a, *p))
    if d['sharpen'][j] is not None:
        x = per_channel(x, d['sharpen'][j], sharpen)
    return x
