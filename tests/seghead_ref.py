"""Case table of the segmentation-head tests (tests/test_gpu_seghead.py runs it on the device, tests/test_seghead_cases_host.py
checks on the CPU that it still reaches every kernel) and the host data of a case.

csrc/loss.hip picks one of five forward kernels, two input-gradient kernels and three weight-gradient kernels per call.
Each case below DECLARES the three it was written for; the host test asks the library (mvd_seghead_{fwd,dx,dw}_path) and
fails when a threshold has moved and a kernel would go untested.  Path numbers as in include/mvdseg_hip.h:
forward 0 k_seghead_fwd, 1 k_seghead_fwd_vox, 2 / 4 / 8 k_seghead_fwd_voxp<P>; dx 0 k_seghead_dx, 1 k_seghead_dx4;
dw 0 k_seghead_dw, 1 k_seghead_dw4, 2 k_seghead_dw4v."""
import collections
import functools

import torch

from oracle import fp64_ops as O

D64 = torch.float64
BF16 = torch.bfloat16
DTYPES = ("fp32", "bf16")
ALIGNED = 15     # x | w << 1 | dlogits << 2 | dx << 3 on a 16-byte boundary: what ops.SegHeadFn passes (torch allocations)
AL_X, AL_W, AL_DL, AL_DX = 1, 2, 4, 8

Case = collections.namedtuple("Case", "N sp C K fwd dx dw")

# channel widths by the forward kernel they were chosen for: (forward path, served by the 4-channel-group kernels dx4 / dw4*)
FAMILIES = {
    "generic": (0, False, (1, 3, 33, 70)),         # C % 4 != 0: one and three channels, a 32-chunk + 1, two chunks + 6
    "vox": (1, True, (4, 12, 20, 32, 48, 100)),    # C % 4 == 0 below 64 or no multiple of 32; 12: 85 rows + one idle thread;
                                                   # 32: the predicate-free branch, the others the ragged last chunk
    "voxp2": (2, True, (64, 96)),                  # 96: lane 0 takes two 32-channel chunks, lane 1 one
    "voxp4": (4, True, (128, 160, 224)),           # 160: lane 0 two chunks, lanes 1-3 one; 224: lane 3 one
    "voxp8": (8, True, (256, 288, 320, 1024)),     # 288, 320: uneven; 1024: one row of 256 groups, the widest dx4 serves
    "wide": (1, False, (1028,)),                   # C / 4 > 256: forward per voxel, generic dx and dw
}
FAMILY_OF = {C: name for name, (_, _, cs) in FAMILIES.items() for C in cs}
ALL_C = tuple(sorted(FAMILY_OF))

# volumes: (extents, V % 4 == 0).  The three small ones take every width and K = 1..8.
SMALL = (((1, 1, 1), False),     # single voxel
         ((5, 7, 9), False),     # V = 315: odd, ragged last block of every forward kernel, dx generic, dw4
         ((4, 6, 10), True))     # V = 240: quads, no multiple of 256: dx4, dw4v
# (N, extents, quads, widths, blocks of the weight-gradient pass): the loops and chunk geometry of the backward kernels;
# K in {1, 5, 8}
LARGER = ((5, (2, 2, 2), True, (4, 12, 320, 1024), 1),    # V = 8: the 12-voxel step of dw4v at C = 320 is longer than a sample
          (40, (1, 2, 2), True, (4, 32, 320), 2),         # V = 4: one 128-voxel chunk spans 32 samples
          (1, (12, 16, 20), True, (32, 33, 96, 320), 60),  # V = 3840: 60 weight-gradient blocks of 64 voxels
          (2, (16, 16, 20), True, (32, 70), 80),          # N V = 10240: seghead_chunk capped at 128 blocks, chunks of 128
          (1, (45, 40, 64), True, (3, 32), 225),          # V = 115200: the four-in-flight loop of k_reduce_partials, some lanes
          (1, (41, 41, 41), False, (4, 33, 64), 120),     # V = 68921: odd, the nb = total / 512 regime (chunks of 576)
          (2, (70, 64, 64), True, (4,), 1120))            # N V = 573440
K_ALL = tuple(range(1, 9))
K_LARGER = (1, 5, 8)


def _declare(N, sp, quads, C, K):
    fwd, grouped, _ = FAMILIES[FAMILY_OF[C]]
    return Case(N, sp, C, K, fwd, 1 if grouped and quads else 0, (2 if quads else 1) if grouped else 0)


def _table():
    cases = []
    for sp, quads in SMALL:
        for C in ALL_C:
            for K in K_ALL:
                # N in {1, 3}: three samples on the single voxel, alternating with K on the other two
                N = 3 if sp == (1, 1, 1) else (1 + 2 * ((K + (sp[0] == 4)) % 2))
                cases.append(_declare(N, sp, quads, C, K))
    for N, sp, quads, cs, _ in LARGER:
        for C in cs:
            for K in K_LARGER:
                cases.append(_declare(N, sp, quads, C, K))
    return tuple(cases)


CASES = _table()

# forward / dx only, integer data, a second or two each
BIG_FWD = Case(1, (64, 128, 128), 64, 3, 1, None, None)    # N V = 2^20: k_seghead_fwd_vox with two whole 32-channel chunks
BIG_DX = Case(1, (66, 128, 128), 32, 2, None, 1, None)     # 270336 quads over 32 rows: 8448 blocks wanted, 8192 launched


def case_id(c):
    return f"N{c.N}-{'x'.join(map(str, c.sp))}-C{c.C}-K{c.K}"


def vol(c):
    return c.sp[0] * c.sp[1] * c.sp[2]


# ------------------------------------------------------------------------------------------------ host data of a case
def _ndhwc(t):
    """[N,*sp,C] -> logical [N,C,*sp] stored NDHWC (no copy)"""
    return t.permute(0, 4, 1, 2, 3)


def ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _seed(c, salt):
    return salt + c.N * 7 + vol(c) * 13 + c.C * 101 + c.K * 1009


# Both functions below cache their last results, because pytest runs the two dtypes (and the accumulate / misaligned variants)
# of a case one after the other; in any other order they are simply computed again.  The tensors they return are SHARED
# between those tests and READ-ONLY: copy before any in-place operation (the device tests only ever upload them).
@functools.lru_cache(maxsize=2)
def integer_case(c):
    """(x, w, b, dl) as small integers and their exact (logits, dx, dw, db) in fp32: every partial sum stays below 2^24, so any
    order of fp32 additions gives the same value, and |dx| <= 2 K <= 16 is exact in bf16 as well.  Shared by both dtypes."""
    g = torch.Generator().manual_seed(_seed(c, 1))
    x = _ndhwc(ints(g, (c.N, *c.sp, c.C), -2, 2))
    w = ints(g, (c.K, c.C, 1, 1, 1), -2, 2)
    b = ints(g, (c.K,), -3, 3)
    dl = ints(g, (c.N, c.K, *c.sp), -1, 1)
    y = O.seghead_fwd(x, w, b)
    dx, dw, db = O.seghead_bwd(x, w, dl)
    assert max(float(t.abs().max()) for t in (y, dx, dw, db)) < 2 ** 24
    return (x, w, b, dl), tuple(t.float() for t in (y, dx, dw, db))


@functools.lru_cache(maxsize=2)
def random_case(c, dtype):
    """(x, w, b, dl) in fp32 (x rounded to bf16 values for the bf16 runs) and the fp64 (logits, dx, dw, db) on those values.
    The operands have non-zero means, so that no reference tensor is a sum that cancels to nothing: the bars are relative to
    the reference's largest magnitude."""
    g = torch.Generator().manual_seed(_seed(c, 2))
    x = _ndhwc(torch.randn((c.N, *c.sp, c.C), generator=g) * 1.5 + 0.3)
    if dtype == "bf16":
        x = x.to(BF16).float()
    w = torch.randn((c.K, c.C, 1, 1, 1), generator=g) * 0.2 + 0.05
    b = torch.randn((c.K,), generator=g) * 0.1
    dl = torch.randn((c.N, c.K, *c.sp), generator=g) + 0.25
    return (x, w, b, dl), (O.seghead_fwd(x, w, b),) + O.seghead_bwd(x, w, dl)
