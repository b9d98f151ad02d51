"""Shared helpers of the level-set persistence tests: the key formula of csrc/levelset2d.hip::k_ls2d_keys restated in numpy,
the host pairing entry driven through ctypes, and the fixture readers."""
import ctypes
import os

import numpy as np

from conftest import GOLDEN
from multimodal_mvd_seg_amd import _lib

_FIX = {}


def fixture(name):
    if name not in _FIX:
        z = np.load(os.path.join(GOLDEN, name), allow_pickle=False)
        _FIX[name] = {k: z[k] for k in z.files}
    return _FIX[name]


def counts(H, W, maxdim=1):
    V = H * W
    E = H * (W - 1) + (H - 1) * W + (H - 1) * (W - 1)
    T = 2 * (H - 1) * (W - 1) if maxdim >= 1 else 0
    return V, E, T


def _ord(v):
    u = v.astype(np.float32).view(np.uint32).astype(np.uint64)
    return np.where(u & 0x80000000, (~u) & 0xFFFFFFFF, u | 0x80000000)


def cells(H, W):
    """(edges [E,2], triangles [T,3]) of init_freudenthal_2d(W, H) in append order within each dimension."""
    ind = np.arange(H * W).reshape(H, W)
    eh = np.stack([ind[:, :-1].ravel(), ind[:, :-1].ravel() + 1], 1)
    ev = np.stack([ind[:-1, :].ravel(), ind[:-1, :].ravel() + W], 1)
    sq = ind[:-1, :-1].ravel()
    ed = np.stack([sq, sq + W + 1], 1)
    tri = np.stack([np.stack([sq, sq + 1, sq + W + 1], 1), np.stack([sq, sq + W, sq + W + 1], 1)], 1).reshape(-1, 3)
    return np.concatenate([eh, ev, ed], 0).astype(np.int64), tri.astype(np.int64)


def host_sorted_keys(f, sublevel, maxdim=1):
    H, W = f.shape
    g = (f if sublevel else -f).astype(np.float32).reshape(-1)
    g = np.where(g == 0, np.float32(0), g)
    edges, tris = cells(H, W)
    keys = [(_ord(g) << np.uint64(32)) | np.arange(g.size, dtype=np.uint64)]
    if edges.shape[0]:
        keys.append((_ord(g[edges].max(1)) << np.uint64(32)) | np.uint64(1 << 30) | np.arange(edges.shape[0], dtype=np.uint64))
    if maxdim >= 1 and tris.shape[0]:
        keys.append((_ord(g[tris].max(1)) << np.uint64(32)) | np.uint64(2 << 30) | np.arange(tris.shape[0], dtype=np.uint64))
    return np.sort(np.concatenate(keys))


def pair_host(keys, P, H, W, sublevel, maxdim=1, threads=16):
    """bars [P, V+T, 4] int32 and edge_row [P, E] of mvd_ls2d_pair_host on host keys [P, n]."""
    lib = _lib.load()
    V, E, T = counts(H, W, maxdim)
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    assert keys.size == P * lib.mvd_ls2d_num_cells(H, W, maxdim, None, None, None)
    bars = np.zeros((P, V + T, 4), dtype=np.int32)
    er = np.zeros((P, max(E, 1)), dtype=np.int32)
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)
    rc = lib.mvd_ls2d_pair_host(ptr(keys), P, H, W, int(sublevel), maxdim, ptr(bars), ptr(er), threads)
    assert rc == 0, lib.mvd_last_error()
    return bars, er[:, :E]


def split(bars, V):
    """(dgm0 [V,4], dgm1 [T,4]) float32 rows (birth, death, birth vertex, death vertex) of one problem's bars."""
    vals = bars[:, :2].copy().view(np.float32)
    rows = np.concatenate([vals, bars[:, 2:].astype(np.float32)], 1)
    return rows[:V], rows[V:]


def srt(a):
    return a[np.lexsort(tuple(a[:, c] for c in range(a.shape[1] - 1, -1, -1)))] if a.shape[0] else a
