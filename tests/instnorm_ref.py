"""Case table of the InstanceNorm path tests (tests/test_gpu_instnorm_paths.py runs it on the device,
tests/test_instnorm_cases_host.py checks on the CPU that it still reaches every kernel at every geometry edge), a plain
Python restatement of the launch plan of csrc/instnorm.hip (norm_geom / in_plan, written from that code), and the host data
and fp64 references of a case.

A case is (N, V, C, x type, y type, entry point, single launch on or off): V is a flat voxel count -- the C ABI takes
[N][V][C] -- and the entry point is one of
  "norm"      mvd_instnorm_lrelu_fwd / _bwd, or _fwd_bf16 / _bwd_bf16 by the types (dy has y's type, dx has x's)
  "head"      the forward as "norm", the backward through mvd_instnorm_lrelu_bwd_head (K = HEAD_K)
  "prestats"  mvd_instnorm_lrelu_fwd_prestats on synthetic tile sums (fp32)
  "tiles"     mvd_instnorm_stats_from_tiles (fp32), or mvd_instnorm_finalize_tiles + mvd_instnorm_lrelu_apply_bf16 (bf16)
Each case DECLARES the kernels it runs (its family, below) and the geometry classes it is there for; the host test asks the
library's own plan (mvd_instnorm_plan) and fails when a threshold has moved."""
import collections
import functools

import torch

from oracle import fp64_ops as O

D64, BF16 = torch.float64, torch.bfloat16
EPS, SLOPE = 1e-5, 0.01
HEAD_K = 3
SMALL_MAX_DEFAULT = 327680   # kInSmallMaxDefault
SMW, SM_MAXR, NRB = 4, 16, 4

# kernel ids (MVD_IN_* of include/mvdseg_hip.h)
(NONE, SMALL_FWD, SMALL_BWD, STATS4, STATS1, TILES_REDUCE, FINALIZE_TILES, APPLY_ROWS, APPLY1, APPLY_SS16, BWD_STATS4,
 BWD_STATS1, BWD_STATS_HEAD, BWD_APPLY_ROWS, BWD_APPLY1, BWD_APPLY_HEAD) = range(16)
KERNEL_NAMES = ("none", "small_fwd", "small_bwd", "stats4", "stats1", "tiles_reduce", "finalize_tiles", "apply_rows", "apply1",
                "apply_ss16", "bwd_stats4", "bwd_stats1", "bwd_stats_head", "bwd_apply_rows", "bwd_apply1", "bwd_apply_head")
TYPES = (("fp32", "fp32"), ("fp32", "bf16"), ("bf16", "bf16"))

Plan = collections.namedtuple("Plan", "stats apply threads R CG nblk chunk agrid achunk tgrid tchunk CW R2")
PLAN_LEN = len(Plan._fields)


# ------------------------------------------------------------------------------------- the launch plan, restated
def cdiv(a, b):
    return (a + b - 1) // b


def norm_geom(N, V, C):
    """(CG, R, threads, nblk, chunk)"""
    CG = C // 4 if C % 4 == 0 else C
    R = max(256 // CG, 1)
    threads = cdiv(R * CG, 64) * 64        # <= 1024 for C <= 1024 (tests/test_norm_geom_host.py)
    want = max(2048 // N, 1)
    nblk = min(max(V // (R * 16), 1), want)
    return CG, R, threads, nblk, cdiv(V, nblk)


def small_threads(V, C, nb, small_max):
    """block size of the single launch, 0: three launches.  nb: the batch of a backward call, 0 forward"""
    if C % 4 != 0 or V <= 0:
        return 0
    elems = V * C
    if (elems * nb > 2 * small_max) if nb > 2 else (elems > small_max):
        return 0
    for t in (64, 256):
        if (t // SMW) * SM_MAXR >= V:
            return t
    return 0


def plan(d, N, V, C, xb, yb, ntiles=0, head=False, small_max=SMALL_MAX_DEFAULT):
    """the Plan of an entry point (d 0 forward, 1 backward), None where the library refuses"""
    v4 = C % 4 == 0
    if not (0 < N <= 65535 and V > 0 and 0 < C <= 1024) or d not in (0, 1) or ntiles < 0 or (d == 1 and ntiles):
        return None
    if (not v4 and (xb or yb)) or (xb and not yb and not (d == 0 and head)):
        return None
    CG, R, threads, nblk, chunk = norm_geom(N, V, C)

    def tiles():
        nb = min(cdiv(ntiles, 64), nblk, 64)
        tchunk = cdiv(ntiles, nb)
        CW = min(C, 256)
        return cdiv(ntiles, tchunk), tchunk, CW, 256 // CW

    def rows():
        nb = min(max(V // (R * 8), 1), max(8192 // N, 1))
        achunk = cdiv(V, nb)
        return cdiv(V, achunk), achunk

    if d == 0 and head:
        if xb if ntiles else not v4:
            return None
        if ntiles:
            tg, tc, CW, R2 = tiles()
            return Plan(TILES_REDUCE, NONE, threads, R, CG, tg, 0, 0, 0, tg, tc, CW, R2)
        return Plan(STATS4, NONE, threads, R, CG, nblk, chunk, 0, 0, 0, 0, 0, 0)
    if head and not (v4 and not xb and not yb):
        return None
    if not xb and not yb and not head:
        th = small_threads(V, C, N if d else 0, small_max)
        if th:
            k = SMALL_BWD if d else SMALL_FWD
            return Plan(k, k, th, th // SMW, SMW, 1, V, cdiv(C // 4, SMW), V, 0, 0, 0, 0)
    ag, ac = rows() if v4 else (min(cdiv(V * C, 256), max(4096 // N, 1)), 0)
    if d == 1:
        if head and threads > 256:
            return None
        st = BWD_STATS_HEAD if head else BWD_STATS4 if v4 else BWD_STATS1
        ap = BWD_APPLY_HEAD if head else BWD_APPLY_ROWS if v4 else BWD_APPLY1
        return Plan(st, ap, threads, R, CG, nblk, chunk, ag, ac, 0, 0, 0, 0)
    if ntiles and yb:
        return Plan(FINALIZE_TILES, APPLY_SS16, threads, R, CG, 0, 0, ag, ac, 1, ntiles, 0, 0) if xb else None
    ap = APPLY1 if not v4 else APPLY_SS16 if xb else APPLY_ROWS
    if ntiles:
        tg, tc, CW, R2 = tiles()
        return Plan(TILES_REDUCE, ap, threads, R, CG, tg, 0, ag, ac, tg, tc, CW, R2)
    return Plan(STATS4 if v4 else STATS1, ap, threads, R, CG, nblk, chunk, ag, ac, 0, 0, 0, 0)


def workspace_bytes(N, V, C):
    return N * norm_geom(N, V, C)[3] * C * 16 + N * C * 8 + 256


# ------------------------------------------------------------------------------------- geometry classes of a plan
def _rems(V, chunk, grid, R, step):
    """remainders (mod step) of the per-thread row counts of a row-mapped kernel whose unrolled loop takes `step` rows: thread
    row r of block b walks v = b chunk + r, + R, ... below min(V, (b + 1) chunk).  Only counts that enter the unrolled loop."""
    got = set()
    for ln in {max(0, min(V, (b + 1) * chunk) - b * chunk) for b in (0, (V - 1) // chunk, grid - 1)}:  # whole, ragged, last
        for r in range(min(R, ln)):
            n = cdiv(ln - r, R)
            if n >= step:
                got.add(n % step)
    return got


def _regime(nblk):
    return "nblk=1" if nblk == 1 else "nblk=2..64" if nblk <= 64 else "nblk=65..128" if nblk <= 128 else "nblk>128"


def classes(p, N, V, C, ntiles=0):
    """{(kernel id, geometry class)} of one launch plan `p` (the library's numbers or the restatement's)"""
    out = set()
    both = [k for k in (p.stats, p.apply) if k != NONE]
    for k in both:
        out.add((k, "any"))
        out.add((k, "N=1" if N == 1 else "N=2" if N == 2 else "N=3" if N == 3 else "N>2048" if N > 2048 else "N=other"))
    if p.stats in (SMALL_FWD, SMALL_BWD):
        return out
    rowk = [k for k in both if k not in (APPLY1, BWD_APPLY1, TILES_REDUCE, FINALIZE_TILES)]
    for k in rowk:
        if p.R * p.CG < p.threads:
            out.add((k, "idle_lanes"))
        if p.R in (1, 256):
            out.add((k, f"R={p.R}"))
    st = p.stats
    if st in (STATS4, STATS1, BWD_STATS4, BWD_STATS1, BWD_STATS_HEAD):
        out.add((st, _regime(p.nblk)))
        last = V - (p.nblk - 1) * p.chunk
        if last <= 0:
            out.add((st, "empty_block"))
        if V % p.chunk:
            out.add((st, "ragged_stats"))
        if st == STATS4:
            out |= {(st, f"rem{r}") for r in _rems(V, p.chunk, p.nblk, p.R, 4)}
        if st in (BWD_STATS4, BWD_STATS_HEAD):
            out |= {(st, f"rem{r}") for r in _rems(V, p.chunk, p.nblk, p.R, 2)}
    if st == TILES_REDUCE:
        out.add((st, _regime(p.nblk)))
        out.add((st, "C<256" if C < 256 else "C=256" if C == 256 else "C>256"))
        cap = cdiv(ntiles, 64)
        nblk = norm_geom(N, V, C)[3]
        out.add((st, "cap_nblk" if nblk < min(cap, 64) else "cap_64" if cap > 64 else "uncapped"))
        out |= {(st, f"rem{r}") for r in _rems(ntiles, p.tchunk, p.tgrid, p.R2, 4)}
    if st in (TILES_REDUCE, FINALIZE_TILES):
        out.add((st, "ntiles<64" if ntiles < 64 else "ntiles=64..255" if ntiles < 256 else
                 "ntiles>=256,%64" if ntiles % 64 else "ntiles>=256"))
    if st == FINALIZE_TILES:
        out |= {(st, f"rem{r}") for r in _rems(ntiles, ntiles, 1, 64, 4)}
    ap = p.apply
    if ap in (APPLY_ROWS, APPLY_SS16, BWD_APPLY_ROWS, BWD_APPLY_HEAD):
        if V % p.achunk:
            out.add((ap, "ragged_apply"))
        out |= {(ap, f"rem{r}") for r in _rems(V, p.achunk, p.agrid, p.R, NRB if ap in (BWD_APPLY_ROWS, BWD_APPLY_HEAD) else 4)}
    if ap in (APPLY1, BWD_APPLY1) and V * C > p.agrid * 256:
        out.add((ap, "grid_stride"))
    return out


# ------------------------------------------------------------------------------------- the case table
Case = collections.namedtuple("Case", "N V C xt yt entry small ntiles fwd bwd why")

# kernels by family and type combination: ((forward statistics, apply), (backward statistics, apply))
ROWS = {("fp32", "fp32"): ((STATS4, APPLY_ROWS), (BWD_STATS4, BWD_APPLY_ROWS)),
        ("fp32", "bf16"): ((STATS4, APPLY_ROWS), (BWD_STATS4, BWD_APPLY_ROWS)),
        ("bf16", "bf16"): ((STATS4, APPLY_SS16), (BWD_STATS4, BWD_APPLY_ROWS))}
SCALAR = ((STATS1, APPLY1), (BWD_STATS1, BWD_APPLY1))
SMALL = ((SMALL_FWD, SMALL_FWD), (SMALL_BWD, SMALL_BWD))

# three-launch shapes with C % 4 == 0: (N, V, C, single launch, classes the shape is there for).  Each runs in the three
# type combinations.  nblk / chunk are those of norm_geom, "apply" those of the apply pass.
ROW_SHAPES = (
    (2, 2431, 320, True, ("nblk=2..64", "ragged_stats", "ragged_apply", "idle_lanes", "N=2")),  # 50 blocks of 49, last 30; 98 apply blocks, last 6; 240 of 256 lanes
    (3, 2431, 96, True, ("nblk=2..64", "ragged_stats", "idle_lanes", "N=3")),       # 240 of 256 lanes, R = 10
    (1, 4999, 36, True, ("nblk=2..64", "ragged_stats", "idle_lanes", "N=1")),       # 252 of 256 lanes, R = 28
    (1, 700, 1024, True, ("nblk=2..64", "empty_block", "R=1")),                     # 43 blocks of 17: block 42 starts at 714
    (1, 1700, 1024, True, ("nblk=65..128", "empty_block", "R=1")),                  # 106 blocks of 17: blocks 100..105 are empty
    (2, 1500, 512, True, ("nblk=2..64", "ragged_stats", "ragged_apply")),
    (1, 5003, 64, True, ("nblk=2..64", "ragged_stats", "ragged_apply")),
    (2, 6007, 128, True, ("nblk=2..64", "ragged_stats")),
    (2, 9000, 32, True, ("nblk=2..64", "ragged_stats")),
    (1, 6197, 320, True, ("nblk>128", "ragged_stats", "idle_lanes")),               # 129 blocks of 49, last 1 voxel
    (1, 70001, 4, True, ("nblk=2..64", "R=256", "ragged_stats")),                   # one channel group: R = 256
    (1, 1031, 256, True, ("nblk=2..64", "ragged_stats")),                           # just over the single launch's 1024 voxels
    (2, 300, 32, False, ("nblk=1",)),                                               # one statistics block, several apply blocks
    (1, 77, 128, False, ("nblk=1", "N=1")),                                         # fewer rows than the unrolled loops take
    (2049, 40, 32, False, ("nblk=1", "N>2048")),                                    # 2048 / N = 0: the cap falls to one block
    (3, 1100, 64, True, ("nblk=2..64", "N=3")),
)
SCALAR_SHAPES = (
    (2, 1633, 5, True, ("nblk=2..64", "idle_lanes", "ragged_stats", "N=2")),        # nblk = 2, 255 of 256 threads
    (2, 300, 257, True, ("nblk=2..64", "idle_lanes", "R=1")),                       # 320 threads, 257 in use
    (1, 700, 1022, True, ("nblk=2..64", "empty_block", "R=1", "idle_lanes")),       # 1024 threads, 43 blocks of 17
    (1, 70001, 1, True, ("nblk=2..64", "R=256", "ragged_stats", "N=1")),
    (3, 27, 5, True, ("nblk=1", "N=3")),
    (1, 2100, 257, True, ("nblk>128", "R=1")),                                      # 131 blocks
    (1, 1700, 30, True, ("nblk=2..64", "idle_lanes")),                              # R = 8: 240 of 256 threads
    (1, 1200, 1022, True, ("nblk=65..128", "grid_stride", "R=1")),                  # 75 blocks of 16; 4792 apply blocks wanted, 4096 run
    (2049, 40, 5, True, ("nblk=1", "N>2048")),
)
# single launch and head form: covered by tests/test_gpu_instnorm_small.py and tests/test_gpu_seghead.py, here for completeness
SMALL_SHAPES = ((2, 512, 320, True, ("any",)), (1, 210, 36, True, ("any",)))
HEAD_SHAPES = ((2, 2431, 32, True, ("nblk=2..64", "ragged_stats", "ragged_apply")), (1, 700, 1024, True, ("empty_block", "R=1")))
# synthetic tiles: (N, V, C, ntiles, classes)
TILE_SHAPES = (
    (2, 1500, 32, 37, ("ntiles<64", "C<256", "uncapped", "nblk=1")),
    (2, 4500, 256, 130, ("ntiles=64..255", "C=256", "uncapped")),
    (1, 6000, 320, 333, ("ntiles>=256,%64", "C>256")),                # the second pass of the channel loop
    (1, 33000, 32, 4200, ("cap_64", "ntiles>=256,%64", "C<256")),     # 66 blocks wanted, 64 run
    (2, 1500, 32, 200, ("cap_nblk", "ntiles=64..255")),               # 4 blocks wanted, the workspace holds 2
    (3, 2600, 320, 70, ("ntiles=64..255", "C>256", "N=3")),
    (1, 5000, 64, 512, ("ntiles>=256", "C<256")),
    (1, 4000, 32, 448, ("ntiles>=256", "C<256")),                     # seven tiles per lane of k_in_finalize_tiles: remainder 3
)


def _table():
    cases = []
    for N, V, C, small, why in ROW_SHAPES:
        for t in TYPES:
            cases.append(Case(N, V, C, *t, "norm", small, 0, *ROWS[t], why))
    for N, V, C, small, why in SCALAR_SHAPES:
        cases.append(Case(N, V, C, "fp32", "fp32", "norm", small, 0, *SCALAR, why))
    for N, V, C, small, why in SMALL_SHAPES:
        cases.append(Case(N, V, C, "fp32", "fp32", "norm", small, 0, *SMALL, why))
    for N, V, C, small, why in HEAD_SHAPES:
        cases.append(Case(N, V, C, "fp32", "fp32", "head", small, 0, (STATS4, APPLY_ROWS), (BWD_STATS_HEAD, BWD_APPLY_HEAD), why))
    for N, V, C, nt, why in TILE_SHAPES:
        cases.append(Case(N, V, C, "fp32", "fp32", "prestats", False, nt, (TILES_REDUCE, APPLY_ROWS), None, why))
        cases.append(Case(N, V, C, "fp32", "fp32", "tiles", False, nt, (TILES_REDUCE, NONE), None, why))
        cases.append(Case(N, V, C, "bf16", "bf16", "tiles", False, nt, (FINALIZE_TILES, APPLY_SS16), None,
                          tuple(w for w in why if w.startswith("ntiles"))))
    return tuple(cases)


CASES = _table()


def case_id(c):
    return f"{c.entry}-N{c.N}-V{c.V}-C{c.C}-{c.xt}-{c.yt}" + (f"-T{c.ntiles}" if c.ntiles else "") + ("" if c.small else "-3l")


def small_max_of(c):
    """what mvd_set_instnorm_small_max gets for the case: the default limit, or 0 (never the single launch)"""
    return SMALL_MAX_DEFAULT if c.small else 0


def plan_args(c, d):
    """arguments of plan() / mvd_instnorm_plan after the direction: N, V, C, x_is_bf16, y_is_bf16, ntiles, head"""
    head = (c.entry == "head" and d == 1) or (c.entry == "tiles" and c.xt == "fp32")
    return c.N, c.V, c.C, int(c.xt == "bf16"), int(c.yt == "bf16"), c.ntiles if d == 0 else 0, int(head)


# ------------------------------------------------------------------------------------- host data and fp64 references
def _seed(c, salt=0):
    return salt + c.N * 7 + c.V * 13 + c.C * 101 + c.ntiles * 1009


def make_x(N, V, C, seed, offset=None):
    """x [N][V][C] fp32: per (n, c) a standard deviation in [0.5, 2] and a mean of at most 1.5 of them (|mean| <= 2 std is
    what the 1-ulp bar of mean / rstd is derived for); offset: mean / std of every channel instead"""
    g = torch.Generator().manual_seed(seed)
    sd = torch.rand(N, 1, C, generator=g) * 1.5 + 0.5
    m = (torch.rand(N, 1, C, generator=g) * 3 - 1.5) if offset is None else torch.full((N, 1, C), float(offset))
    return (torch.randn(N, V, C, generator=g) + m) * sd, g


def as5d(t):
    """[N][V][C] -> the logical [N, C, 1, 1, V] view oracle/fp64_ops.py and ops.py take (NDHWC storage, no copy)"""
    return t.permute(0, 2, 1).unsqueeze(2).unsqueeze(2)


def tile_sizes(V, ntiles):
    """V voxels in ntiles consecutive groups of at most 128 (as even as they come)"""
    base, extra = divmod(V, ntiles)
    assert 1 <= base and base + (extra > 0) <= 128, (V, ntiles)
    return [base + (i < extra) for i in range(ntiles)]


def tile_sums(x64, ntiles):
    """[N][ntiles][C][2] fp32: (sum x, sum x^2) of each tile, summed in fp64 and rounded to fp32 -- what a conv epilogue hands
    over (its own sums are fp32; the kernels under test only add the pairs)"""
    N, V, C = x64.shape
    idx = torch.repeat_interleave(torch.arange(ntiles), torch.tensor(tile_sizes(V, ntiles)))
    out = torch.zeros(N, ntiles, C, 2, dtype=D64)
    out[..., 0].index_add_(1, idx, x64)
    out[..., 1].index_add_(1, idx, x64 * x64)
    return out.float()


def stats_from_tile_sums(ts, V, eps=EPS):
    """(mean, rstd) [N][C] in fp64 from the rounded tile sums"""
    s = ts.to(D64).sum(1)
    mean = s[..., 0] / V
    var = (s[..., 1] / V - mean * mean).clamp_min(0)
    return mean, 1.0 / torch.sqrt(var + eps)


def apply64(x64, mean, rstd, gamma, beta, slope=SLOPE):
    """(y, z, xhat) [N][V][C] in fp64 for given statistics"""
    xhat = (x64 - mean.unsqueeze(1)) * rstd.unsqueeze(1)
    z = xhat * gamma + beta
    return torch.where(z > 0, z, z * slope), z, xhat


Data = collections.namedtuple("Data", "x gamma beta dy tiles hw dl x64 dy64 mean rstd y z xhat")


# the result is SHARED between the tests of a case and READ-ONLY (the device tests only upload it)
@functools.lru_cache(maxsize=2)
def case_data(c, offset=None):
    """host inputs of a case (fp32 tensors holding bf16-representable values where the type is bf16) and the fp64 forward on
    exactly those values; statistics of a tile case from the rounded tile sums"""
    x, g = make_x(c.N, c.V, c.C, _seed(c, 1), offset)
    if c.xt == "bf16":
        x = x.to(BF16).float()
    gamma = torch.rand(c.C, generator=g) + 0.5
    beta = torch.randn(c.C, generator=g) * 0.2
    x64 = x.to(D64)
    tiles = hw = dl = None
    if c.entry == "head":
        dl = torch.randn(c.N, HEAD_K, c.V, generator=g) + 0.25
        hw = torch.randn(HEAD_K, c.C, generator=g) * 0.2 + 0.05
        dy64 = torch.einsum('nkv,kc->nvc', dl.to(D64), hw.to(D64))
        dy = None
    else:
        dy = torch.randn(c.N, c.V, c.C, generator=g)
        if c.yt == "bf16":
            dy = dy.to(BF16).float()
        dy64 = dy.to(D64)
    if c.ntiles:
        tiles = tile_sums(x64, c.ntiles)
        mean, rstd = stats_from_tile_sums(tiles, c.V)
        y, z, xhat = apply64(x64, mean, rstd, gamma.to(D64), beta.to(D64))
    else:
        y5, z5, xh5, rstd = O.instnorm_lrelu_fwd(as5d(x64), gamma.to(D64), beta.to(D64), EPS, SLOPE)
        y, z, xhat = (t.squeeze(2).squeeze(2).permute(0, 2, 1) for t in (y5, z5, xh5))
        mean = x64.mean(1)
    return Data(x, gamma, beta, dy, tiles, hw, dl, x64, dy64, mean, rstd, y, z, xhat)


def bwd64(d, mask):
    """(dx [N][V][C], dgamma, dbeta) in fp64 with the LeakyReLU branches of `mask` [N][V][C]"""
    dx, dg, db = O.instnorm_lrelu_bwd(as5d(d.dy64), as5d(d.xhat), d.rstd, d.gamma.to(D64), as5d(mask), SLOPE)
    return dx.squeeze(2).squeeze(2).permute(0, 2, 1), dg, db


def ulps(a, ref):
    """distance in float32 steps between two float32 tensors (ordered-integer distance; exact for finite values)"""
    def key(t):
        i = t.contiguous().view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return (key(a) - key(ref)).abs()


# ------------------------------------------------------------------------------------- the entry points, for the refusals
POINTERS = ("x", "g", "b", "y", "mean", "rstd", "ws", "dy", "dx", "dg", "db", "w", "tiles", "scale", "shift")


def entry_calls(N, V, C, ws_bytes, ntiles=5):
    """{key: (entry point, its argument list with the pointers by name)}: bind() puts addresses in"""
    tail = ("ws", ws_bytes, None)
    return {
        "fwd": ("mvd_instnorm_lrelu_fwd", ["x", "g", "b", "y", "mean", "rstd", N, V, C, EPS, SLOPE, *tail]),
        "prestats": ("mvd_instnorm_lrelu_fwd_prestats", ["x", "tiles", ntiles, "g", "b", "y", "mean", "rstd", N, V, C, EPS, SLOPE,
                                                         *tail]),
        "fwd_bf16/x32": ("mvd_instnorm_lrelu_fwd_bf16", ["x", 0, "g", "b", "y", "mean", "rstd", N, V, C, EPS, SLOPE, *tail]),
        "fwd_bf16/x16": ("mvd_instnorm_lrelu_fwd_bf16", ["x", 1, "g", "b", "y", "mean", "rstd", N, V, C, EPS, SLOPE, *tail]),
        "stats_bf16": ("mvd_instnorm_stats_bf16", ["x", 1, "g", "b", "mean", "rstd", "scale", "shift", N, V, C, EPS, *tail]),
        "apply_bf16": ("mvd_instnorm_lrelu_apply_bf16", ["x", "scale", "shift", "y", N, V, C, SLOPE, None]),
        "bwd": ("mvd_instnorm_lrelu_bwd", ["x", "dy", "g", "b", "mean", "rstd", "dx", "dg", "db", N, V, C, SLOPE, *tail]),
        "bwd_bf16/x32": ("mvd_instnorm_lrelu_bwd_bf16", ["x", 0, "dy", "g", "b", "mean", "rstd", "dx", "dg", "db", N, V, C, SLOPE,
                                                         *tail]),
        "bwd_bf16/x16": ("mvd_instnorm_lrelu_bwd_bf16", ["x", 1, "dy", "g", "b", "mean", "rstd", "dx", "dg", "db", N, V, C, SLOPE,
                                                         *tail]),
        "bwd_head": ("mvd_instnorm_lrelu_bwd_head", ["x", "dy", "w", 3, "g", "b", "mean", "rstd", "dx", "dg", "db", N, V, C, SLOPE,
                                                     *tail]),
    }


def bind(p, args, shift=None, by=0):
    """the argument list with the addresses of `p` ({name: address}); the pointer named `shift` moved by `by` bytes"""
    return [(p[a] + (by if a == shift else 0)) if isinstance(a, str) else a for a in args]


def misaligned_calls(N, V, C, ws_bytes):
    """(entry point, key, tensor, bytes): x, y, dy and dx of every entry point one element off (4 bytes fp32, 2 bytes bf16)"""
    out = []
    for key, (name, args) in entry_calls(N, V, C, ws_bytes).items():
        x16, y16 = key.endswith("x16") or key in ("stats_bf16", "apply_bf16"), "bf16" in key
        for which, by in (("x", 2 if x16 else 4), ("y", 2 if y16 else 4), ("dy", 2 if y16 else 4), ("dx", 2 if x16 else 4)):
            if which in args and not (which == "dy" and key == "bwd_head"):   # (the planar logit gradient is read by the float)
                out.append((name, key, which, by))
    return out
