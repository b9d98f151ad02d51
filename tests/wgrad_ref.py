"""The weight-gradient case table: every kernel wgrad_plan (csrc/conv_mfma.hip) can choose, at the geometry edges where such
kernels go wrong.  tests/test_wgrad_cases_host.py checks on the CPU, from the LIBRARY's plan (mvd_conv_wgrad_plan: the plan
the launch code itself consumes), which kernel and which classes each case reaches and that every cell of its matrix has a
case; tests/test_gpu_wgrad_paths.py runs every case against fp64.  Nothing here restates a threshold: a moved threshold
moves a case out of its cell and turns the host module red."""
import collections
import ctypes
import os

from multimodal_mvd_seg_amd import _lib

PLAN_FIELDS = ("kernel reduce bias TPW NA NB SH TRI TD TH TW ntd nth ntw ntiles nsplit partials ncb nkb bias_rows needed_ws "
               "ws_bytes wino_mode wino3_on wino3_min bias_fold bf16_kernel engine_mode env_big16 env_tri16 env_db env_16z "
               "env_16zs env_reduce_g16").split()
PLAN_LEN = len(PLAN_FIELDS)
Plan = collections.namedtuple("Plan", PLAN_FIELDS)
KERNEL_NAMES = ("none", "wino3", "wino2w12", "wino", "smallc", "mfma", "wgrad16", "wgrad16z", "wgrad16zs", "scalar")
NONE, WINO3, WINO2W12, WINO, SMALLC, MFMA, WGRAD16, WGRAD16Z, WGRAD16ZS, SCALAR = range(10)
REDUCE_NAMES = ("none", "f4", "f16", "wino", "wino2", "wino3", "d")
BIAS_NAMES = ("none", "colsum", "generic", "convt", "smallc", "wino3", "wino2w12", "slot28", "zmarch")
DIRECT = (SMALLC, MFMA, WGRAD16, WGRAD16Z, WGRAD16ZS, SCALAR)   # kernels that multiply the operands themselves

# pure A/B switches read at process start: not part of the matrix; a run that sets one (or MVD_WINO=0) skips the modules
ABLATION_ENV = ("MVD_WGRAD16_BIG", "MVD_WGRAD16_TRI", "MVD_WGRAD_DB", "MVD_WGRAD16Z", "MVD_WGRAD16ZS", "MVD_WGRAD_WINO3",
                "MVD_WGRAD_WINO3_MIN", "MVD_WGRAD_BIAS_FOLD", "MVD_WGRAD_REDUCE_G16", "MVD_CONV_DBG")


def skip_reason():
    """why this process cannot judge the default dispatch (None: it can)"""
    for k in ABLATION_ENV:
        if k in os.environ:
            return f"{k} is set for this run"
    if os.environ.get("MVD_WINO", "2") != "2":
        return "MVD_WINO is set for this run"
    return None


# setters of a case: name -> (entry point, value that restores the default)
SETTERS = {"wino3_min": ("mvd_set_wgrad_wino3_min_items", -1), "bias_fold": ("mvd_set_wgrad_bias_fold", -1),
           "bf16_kernel": ("mvd_set_bf16_wgrad_kernel", 1), "engine": ("mvd_set_conv_engine", 0)}

Case = collections.namedtuple("Case", "kind dt N C1 C2 K sp ks st bias setters env kernel why")


def C(kind, dt, N, C1, C2, K, sp, ks, st, kernel, why=(), bias=True, env=None, **setters):
    assert kind in ("conv", "convT") and dt in ("fp32", "bf16") and set(setters) <= set(SETTERS)
    return Case(kind, dt, N, C1, C2, K, tuple(sp), tuple(ks), tuple(st), bias, tuple(sorted(setters.items())),
                tuple(sorted((env or {}).items())), kernel, tuple(why))


def case_id(c):
    s = f"{c.kind}-{c.dt}-N{c.N}-{c.C1}+{c.C2}to{c.K}-{'x'.join(map(str, c.sp))}-k{''.join(map(str, c.ks))}-s{''.join(map(str, c.st))}"
    s += "" if c.bias else "-nobias"
    s += "".join(f"-{k}{v}" for k, v in c.setters) + "".join(f"-{k}{v}" for k, v in c.env)
    return s


class applied:
    """the setters of a case for the duration of a `with` block"""

    def __init__(self, c):
        self.c = c

    def __enter__(self):
        for k, v in self.c.setters:
            _lib.call(SETTERS[k][0], v)

    def __exit__(self, *exc):
        for k, _ in self.c.setters:
            _lib.call(SETTERS[k][0], SETTERS[k][1])


def out_sp(c):
    if c.kind == "convT":
        return tuple(s * t for s, t in zip(c.sp, c.st))
    return tuple((s + 2 * ((k - 1) // 2) - k) // t + 1 for s, k, t in zip(c.sp, c.ks, c.st))


def ntaps(c):
    return c.st[0] * c.st[1] * c.st[2] if c.kind == "convT" else c.ks[0] * c.ks[1] * c.ks[2]


def workspace_bytes(c):
    if c.kind == "convT":
        return _lib.query("mvd_convT3d_wgrad_workspace_bytes", c.C1, c.K, ntaps(c), c.N, *c.sp)
    return _lib.query("mvd_conv3d_wgrad_workspace_bytes", c.C1 + c.C2, c.K, ntaps(c), c.N, *out_sp(c))


def raw_plan(transposed, bf16, N, sp, C1, C2, K, ks, st, ws_bytes=0, want_bias=1, prologue=0):
    """the library's plan, or None where it refuses (status 2 with a message)"""
    lib = _lib.load()
    buf = (ctypes.c_long * PLAN_LEN)()
    rc = lib.mvd_conv_wgrad_plan(int(transposed), int(bf16), N, *sp, C1, C2, K, _lib.i3(ks), _lib.i3(st), ws_bytes, int(want_bias),
                                 int(prologue), buf)
    assert rc in (0, 2) and (rc == 0 or len(lib.mvd_last_error()) > 10), rc
    return Plan(*buf) if rc == 0 else None


def plan_of(c, ws_bytes=0):
    with applied(c):
        return raw_plan(c.kind == "convT", c.dt == "bf16", c.N, c.sp, c.C1, c.C2, c.K, c.ks, c.st, ws_bytes, c.bias)


def _axis(name, extent, tile):
    return f"{name}:small" if extent < tile else f"{name}:whole" if extent % tile == 0 else f"{name}:ragged"


def classes(p, c):
    """the geometry classes a case sits in, from the library's plan of it"""
    # the iteration grid: the output voxels of a conv, the input voxels of a transposed conv
    grid = c.sp if c.kind == "convT" else out_sp(c)
    cl = {_axis("D", grid[0], p.TD), _axis("H", grid[1], p.TH), _axis("W", grid[2], p.TW)} if p.kernel != SCALAR else set()
    if p.ntiles == p.nsplit:
        cl.add("split:clipped")        # fewer tiles than the split count of the shape: one tile per split
    elif p.ntiles % p.nsplit:
        cl.add("split:remainder")      # some splits walk one tile more
    else:
        cl.add("split:even")
    cl.add(f"N={c.N}" if c.N <= 3 else "N>3")
    if p.kernel != SCALAR:
        cl |= {"ncb=1" if p.ncb == 1 else "ncb>1", "nkb=1" if p.nkb == 1 else "nkb>1"}
    if (c.C1 + c.C2) % 32:
        cl.add("C%32")
    if c.K % 32:
        cl.add("K%32")
    if c.C2:
        cl.add("C2>0")
    t = ntaps(c)
    shape = "".join(map(str, c.st if c.kind == "convT" else c.ks))
    cl.add(f"taps={t}" if t in (1, 27, 8, 4, 2) else f"taps={t}:{shape}")
    if p.kernel in (MFMA, WGRAD16):
        cl |= {f"TPW={p.TPW}", f"cfg:{p.NA}.{p.NB}.{p.SH}"}     # the template that runs: k_wgrad_mfma<TPW, NA, NB, SH>
    if p.kernel == WGRAD16:
        cl.add("tri" if p.TRI else "notri")
    if p.kernel == SCALAR:                                       # what kept the MFMA kernels from the shape
        why = {"why:C1%4": c.C1 % 4, "why:C2%4": c.C2 % 4, "why:K%4": c.K % 4, "why:C2>0,C1%32": c.C2 > 0 and c.C1 % 32}
        cl |= {k for k, v in why.items() if v} or ({"why:engine"} if p.engine_mode else set())
    if c.kind == "conv":
        cl.add("stride1" if c.st == (1, 1, 1) else "stride2" if c.st == (2, 2, 2) else "stride_mixed")
    cl.add("bias:" + BIAS_NAMES[p.bias] if c.bias else "nobias")
    cl.add("reduce:" + REDUCE_NAMES[p.reduce])
    return cl


K3, K1, S1, S2 = (3, 3, 3), (1, 1, 1), (1, 1, 1), (2, 2, 2)
# The smallest shapes that reach each cell (chosen by a greedy cover of MATRIX over a few thousand candidate shapes, cheapest
# fp64 reference first), plus a few multi-tile shapes of the layers the networks run.  The comment of a line names the cells it
# was chosen for; `why` pins those that only this line supplies.
_W2 = [  # plain 3x3x3 stride 1, 32-multiple channels: k_wgrad_wino2w12 by default, k_wgrad_wino3 with the item minimum at 1,
         # k_wgrad_wino under MVD_WINO=1 -- the same shapes for all three (tile 2x8x8)
    (1, 32, 0, 32, (2, 3, 5), True),     # D:whole H:small W:small N=1 ncb=1 nkb=1 split:clipped
    (1, 32, 32, 32, (1, 9, 8), False),   # C2>0 D:small H:ragged W:whole ncb>1 nobias
    (2, 32, 0, 64, (2, 3, 5), True),     # N=2 nkb>1
    (3, 32, 0, 32, (3, 5, 4), True),     # D:ragged N=3
    (1, 32, 0, 32, (2, 8, 8), True),     # H:whole
    (1, 32, 0, 32, (5, 4, 9), True),     # W:ragged
    (3, 128, 0, 128, (5, 4, 9), True),   # split:remainder (18 tiles over 16 splits)
    (2, 256, 0, 256, (8, 4, 4), True),   # split:even (8 tiles over 4 splits)
    (2, 32, 32, 64, (9, 10, 17), True),  # a decoder layer: 60 tiles, ragged on every axis, two inputs
]
CASES = [C("conv", "fp32", N, C1, C2, K, sp, K3, S1, WINO3, bias=b, wino3_min=1) for N, C1, C2, K, sp, b in _W2]
CASES += [C("conv", "fp32", N, C1, C2, K, sp, K3, S1, WINO2W12, bias=b) for N, C1, C2, K, sp, b in _W2]
CASES += [C("conv", "fp32", N, C1, C2, K, sp, K3, S1, WINO, bias=b, env={"MVD_WINO": "1"}) for N, C1, C2, K, sp, b in _W2]
CASES += [
    # ---- k_wgrad_smallc: fp32, one input of 4 or 8 channels, at most 128 (tap, channel) rows
    C("conv", "fp32", 1, 4, 0, 8, (2, 4, 4), K1, S2, SMALLC),                      # D/H/W:small K%32 nkb=1 stride2 taps=1
    C("conv", "fp32", 2, 4, 0, 36, (2, 8, 8), (3, 1, 1), (1, 2, 2), SMALLC, ("bias:colsum",), bias_fold=0),  # whole tiles N=2 nkb>1
    C("conv", "fp32", 3, 4, 0, 8, (9, 10, 17), (1, 1, 3), S1, SMALLC, ("reduce:f16",)),  # ragged on every axis, N=3
    C("conv", "fp32", 1, 4, 0, 8, (2, 3, 5), (1, 3, 1), S1, SMALLC, bias=False),   # nobias taps=3:131
    C("conv", "fp32", 1, 4, 0, 8, (2, 4, 4), (1, 3, 3), S2, SMALLC),               # taps=9:133
    C("conv", "fp32", 1, 4, 0, 8, (2, 4, 4), (3, 1, 3), S2, SMALLC),               # taps=9:313
    C("conv", "fp32", 1, 4, 0, 8, (2, 4, 4), (3, 3, 1), S2, SMALLC),               # taps=9:331
    C("conv", "fp32", 1, 4, 0, 8, (2, 4, 4), K3, S2, SMALLC),                      # taps=27
    C("conv", "fp32", 2, 4, 0, 36, (17, 33, 65), K3, S2, SMALLC, ("split:remainder",)),
    C("conv", "fp32", 2, 4, 0, 36, (16, 32, 64), (1, 3, 3), S1, SMALLC, ("split:even",)),
    C("conv", "fp32", 2, 4, 0, 32, (9, 10, 17), K3, S1, SMALLC, ("bias:smallc",)),   # the input layer of the networks
    C("conv", "fp32", 1, 8, 0, 32, (5, 6, 7), (1, 3, 3), S1, SMALLC),              # 8 channels: 72 rows
    # ---- k_wgrad_mfma, convs: everything else with channels in fours
    C("conv", "fp32", 1, 8, 0, 16, (2, 4, 4), K1, S2, MFMA),                       # small tiles, partial blocks, TPW=1
    C("conv", "fp32", 2, 32, 32, 32, (2, 8, 8), (3, 1, 1), (1, 2, 2), MFMA, ("C2>0", "stride_mixed")),
    C("conv", "fp32", 1, 8, 0, 16, (5, 4, 9), (3, 1, 3), S1, MFMA, ("TPW=4",), bias=False),
    C("conv", "fp32", 3, 8, 0, 64, (1, 9, 8), (1, 1, 3), S2, MFMA),                # H:ragged N=3 nkb>1 taps=3:113
    C("conv", "fp32", 1, 8, 0, 16, (2, 4, 4), K3, S2, MFMA, ("TPW=7",)),
    C("conv", "fp32", 3, 8, 0, 16, (9, 10, 17), (1, 3, 1), S2, MFMA, ("reduce:f16",)),
    C("conv", "fp32", 1, 8, 0, 16, (2, 4, 4), (3, 3, 1), S2, MFMA),                # taps=9:331
    C("conv", "fp32", 1, 8, 0, 16, (2, 4, 4), (1, 3, 3), (1, 2, 2), MFMA),         # taps=9:133
    C("conv", "fp32", 3, 256, 0, 256, (4, 4, 4), K1, (1, 2, 2), MFMA, ("split:remainder",)),
    C("conv", "fp32", 2, 256, 0, 256, (8, 4, 4), K1, (1, 2, 2), MFMA, ("split:even",)),
    C("conv", "fp32", 2, 32, 0, 64, (10, 12, 18), K3, S2, MFMA, ("bias:generic",)),  # the first conv of an encoder stage
    C("conv", "fp32", 2, 24, 0, 48, (5, 6, 7), K3, S1, MFMA, ("C%32", "K%32")),    # 27 taps stride 1, partial blocks
    C("conv", "fp32", 1, 48, 0, 24, (5, 6, 7), (1, 3, 3), S1, MFMA),               # two c-blocks, the second partial
    # ---- k_wgrad_mfma, transposed convs (kernel == stride)
    C("convT", "fp32", 1, 8, 0, 16, (2, 3, 5), K1, (1, 1, 2), MFMA, ("cfg:7.2.0", "bias:colsum")),   # two taps: SH 0
    C("convT", "fp32", 2, 8, 0, 16, (1, 9, 8), K1, S2, MFMA, ("cfg:1.8.2", "bias:convt", "TPW=2")),
    C("convT", "fp32", 3, 24, 0, 48, (3, 5, 4), K1, S1, MFMA, ("bias:generic",)),  # one tap: SH 1
    C("convT", "fp32", 1, 8, 0, 16, (5, 4, 9), K1, (1, 2, 2), MFMA, ("taps=4",), bias=False),
    C("convT", "fp32", 1, 64, 0, 32, (2, 3, 5), K1, S1, MFMA),                     # ncb>1
    C("convT", "fp32", 3, 8, 0, 16, (6, 8, 9), K1, (1, 1, 2), MFMA, ("reduce:f16",)),
    C("convT", "fp32", 3, 320, 0, 320, (2, 3, 5), K1, S1, MFMA, ("split:remainder",)),
    C("convT", "fp32", 1, 320, 0, 320, (3, 5, 4), K1, (1, 1, 2), MFMA, ("split:even",)),
    C("convT", "fp32", 2, 64, 0, 32, (5, 6, 9), K1, S2, MFMA, ("bias:convt",)),    # a decoder's transposed conv, ragged
    C("convT", "fp32", 1, 64, 0, 32, (4, 6, 5), K1, (1, 2, 2), MFMA, ("bias:convt",)),
    C("convT", "fp32", 1, 64, 0, 32, (4, 6, 5), K1, (2, 1, 1), MFMA, bias_fold=0),
    # ---- k_wgrad16: bf16 tiled
    C("conv", "bf16", 1, 32, 32, 32, (2, 4, 4), K1, S2, WGRAD16, ("C2>0",)),
    C("conv", "bf16", 1, 32, 0, 32, (2, 8, 8), (3, 1, 3), (1, 2, 2), WGRAD16, ("TPW=4", "stride_mixed"), bias=False),
    C("conv", "bf16", 2, 32, 0, 64, (5, 4, 9), (3, 1, 1), S2, WGRAD16),            # D:ragged N=2 W:ragged nkb>1 taps=3:311
    C("conv", "bf16", 1, 32, 0, 32, (2, 3, 5), K3, S1, WGRAD16, ("tri", "bias:slot28")),
    C("conv", "bf16", 3, 32, 0, 32, (1, 9, 8), (1, 1, 3), (1, 2, 2), WGRAD16),     # H:ragged N=3 taps=3:113
    C("conv", "bf16", 1, 32, 0, 32, (2, 4, 4), (1, 3, 1), S2, WGRAD16),            # taps=3:131
    C("conv", "bf16", 1, 32, 0, 32, (2, 4, 4), (1, 3, 3), S2, WGRAD16),            # taps=9:133
    C("conv", "bf16", 1, 32, 0, 32, (2, 4, 4), (3, 3, 1), S2, WGRAD16),            # taps=9:331
    C("conv", "bf16", 3, 32, 0, 32, (9, 9, 33), K1, (1, 2, 2), WGRAD16, ("reduce:f16",)),
    C("conv", "bf16", 3, 256, 0, 256, (8, 4, 4), K1, (1, 2, 2), WGRAD16, ("split:remainder",)),
    C("conv", "bf16", 2, 256, 0, 256, (9, 10, 17), K1, S2, WGRAD16, ("split:even",)),
    C("conv", "bf16", 1, 32, 0, 32, (38, 36, 28), K3, S1, WGRAD16, ("cfg:10.4.1", "tri")),   # the 256-voxel tile: Wo < 32
    C("conv", "bf16", 2, 32, 32, 32, (9, 10, 17), K3, S1, WGRAD16, ("cfg:7.2.1", "tri")),    # 60 tiles, two inputs
    C("conv", "bf16", 2, 32, 0, 64, (9, 10, 17), K3, S2, WGRAD16, ("notri", "bias:slot28")),  # stride 2 below k_wgrad16zs
    C("conv", "bf16", 1, 32, 0, 32, (9, 10, 33), K3, S1, WGRAD16, ("tri",), bf16_kernel=0),   # k_wgrad16z's shape, kernel off
    C("convT", "bf16", 1, 32, 0, 32, (2, 3, 5), K1, S1, WGRAD16),
    C("convT", "bf16", 1, 64, 0, 32, (1, 9, 8), K1, (1, 1, 2), WGRAD16, ("cfg:7.2.0",), bias=False),
    C("convT", "bf16", 1, 32, 0, 64, (2, 4, 4), K1, S2, WGRAD16, ("cfg:1.8.2", "TPW=2")),
    C("convT", "bf16", 2, 32, 0, 32, (5, 4, 9), K1, S1, WGRAD16),
    C("convT", "bf16", 3, 32, 0, 32, (2, 3, 5), K1, (1, 2, 2), WGRAD16, ("taps=4",)),
    C("convT", "bf16", 3, 320, 0, 320, (3, 5, 4), K1, S1, WGRAD16, ("split:remainder",)),
    C("convT", "bf16", 2, 256, 0, 256, (6, 8, 9), K1, (1, 1, 2), WGRAD16, ("split:even",)),
    C("convT", "bf16", 2, 64, 0, 32, (5, 6, 9), K1, S2, WGRAD16),
    # ---- k_wgrad16z: bf16 plain 3x3x3 stride 1, Wo >= 32, Ho >= 8, Do >= 8 (column tile 8 x 32, chunks of zc planes)
    C("conv", "bf16", 1, 32, 0, 32, (8, 8, 32), K3, S1, WGRAD16Z, ("bias:zmarch",)),
    C("conv", "bf16", 1, 32, 0, 32, (9, 9, 33), K3, S1, WGRAD16Z, bias=False),
    C("conv", "bf16", 1, 32, 32, 32, (8, 8, 32), K3, S1, WGRAD16Z, ("C2>0",)),
    C("conv", "bf16", 2, 32, 0, 64, (8, 8, 32), K3, S1, WGRAD16Z),
    C("conv", "bf16", 1, 32, 0, 32, (17, 9, 33), K3, S1, WGRAD16Z, ("D:ragged",)),
    C("conv", "bf16", 3, 32, 0, 32, (8, 8, 32), K3, S1, WGRAD16Z),
    C("conv", "bf16", 3, 128, 0, 256, (9, 9, 33), K3, S1, WGRAD16Z, ("split:even",)),
    C("conv", "bf16", 3, 128, 0, 256, (8, 24, 32), K3, S1, WGRAD16Z, ("split:remainder",)),
    # ---- k_wgrad16zs: bf16 plain 3x3x3 stride 2, K % 64, Wo >= 32, at least 128 (unit, block) pairs
    C("conv", "bf16", 3, 64, 0, 128, (15, 17, 65), K3, S2, WGRAD16ZS, ("split:clipped", "bias:colsum")),
    C("conv", "bf16", 2, 64, 0, 64, (15, 63, 65), K3, S2, WGRAD16ZS, ("nkb=1",), bias=False),
    C("conv", "bf16", 1, 128, 0, 128, (17, 33, 67), K3, S2, WGRAD16ZS, ("D:ragged",)),
    C("conv", "bf16", 2, 32, 0, 128, (15, 63, 65), K3, S2, WGRAD16ZS, ("ncb=1",)),
    C("conv", "bf16", 2, 256, 0, 256, (10, 12, 64), K3, S2, WGRAD16ZS, ("W:whole",)),
    C("conv", "bf16", 3, 64, 0, 256, (7, 31, 129), K3, S2, WGRAD16ZS, ("split:even",)),
    C("conv", "bf16", 2, 128, 0, 256, (15, 33, 65), K3, S2, WGRAD16ZS, ("split:remainder",)),
    # ---- k_wgrad_scalar: what the MFMA kernels do not take
    C("conv", "fp32", 1, 5, 0, 32, (2, 4, 4), K1, S2, SCALAR, ("why:C1%4",)),
    C("conv", "fp32", 3, 32, 0, 30, (9, 10, 17), K1, S2, SCALAR, ("why:K%4", "split:remainder")),
    C("conv", "fp32", 2, 24, 8, 32, (2, 4, 4), K1, S2, SCALAR, ("why:C2>0,C1%32",)),
    C("conv", "fp32", 1, 32, 6, 32, (2, 3, 5), K1, S1, SCALAR, ("why:C2%4",), bias=False),
    C("conv", "fp32", 1, 32, 0, 32, (2, 4, 4), K3, S2, SCALAR, ("why:engine",), engine=1),
    C("conv", "fp32", 2, 3, 0, 7, (5, 6, 7), K3, S1, SCALAR),                      # 27 taps over several chunks
    C("convT", "fp32", 1, 5, 0, 32, (2, 3, 5), K1, S1, SCALAR),
    C("convT", "fp32", 1, 32, 0, 30, (2, 3, 5), K1, S1, SCALAR, bias=False),
    C("convT", "fp32", 2, 5, 0, 32, (9, 17, 8), K1, S1, SCALAR, ("split:remainder",)),
    C("convT", "fp32", 1, 6, 0, 10, (3, 5, 4), K1, S2, SCALAR),                    # eight taps
]
