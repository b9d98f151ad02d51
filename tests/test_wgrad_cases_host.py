"""CPU tests of the weight-gradient case table (tests/wgrad_ref.py).  The library's host-only plan (mvd_conv_wgrad_plan: the
function the launch code itself consumes, no device call) says which kernel, reduce kernel and bias-gradient source a
weight-gradient entry point runs for a shape.  Every case must run the kernel it declares; every cell of MATRIX (kernel x
geometry class it can meet x operation and type) must have a case, so that a later change of a threshold turns this module red
instead of silently un-testing a path; cells marked unreachable carry a reason and no shape of the scan grid may reach them;
and over a grid with a value on each side of every threshold of the dispatch the plan keeps the invariants listed at
test_plan_invariants_over_the_scan_grid.  Cases under MVD_WINO=1 (k_wgrad_wino, a documented mode read at process start) are
planned in one fresh child process."""
import itertools
import json
import os
import re
import subprocess
import sys

import pytest

import wgrad_ref as R
from conftest import ROOT
from multimodal_mvd_seg_amd import _lib

pytestmark = [pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libmvdseg_hip.so not built"),
              pytest.mark.skipif(R.skip_reason() is not None, reason=str(R.skip_reason()))]

CONV32, CONVT32, CONV16, CONVT16 = ("conv", "fp32"), ("convT", "fp32"), ("conv", "bf16"), ("convT", "bf16")
AXES = tuple(f"{a}:{k}" for a in "DHW" for k in ("whole", "ragged", "small"))
AXES_Z = tuple(f"{a}:{k}" for a in "DHW" for k in ("whole", "ragged"))       # the z-marching kernels: Wo >= 32, Ho, Do >= 8 / 4
SPLITS = ("split:clipped", "split:remainder", "split:even")
NS = ("N=1", "N=2", "N=3")
BLOCKS = ("ncb=1", "ncb>1", "nkb=1", "nkb>1")
WINO = AXES + SPLITS + NS + BLOCKS + ("C2>0", "nobias")
TAPS9 = ("taps=9:133", "taps=9:331", "taps=9:313")
TAPS3 = ("taps=3:311", "taps=3:131", "taps=3:113")
STRIDES = ("stride1", "stride2", "stride_mixed")
# kernel -> [(operation and type, the classes the kernel can meet there)]
MATRIX = {
    "wino3": [(CONV32, WINO + ("bias:wino3", "reduce:wino3"))],
    "wino2w12": [(CONV32, WINO + ("bias:wino2w12", "reduce:wino2"))],
    "wino": [(CONV32, WINO + ("bias:colsum", "reduce:wino"))],
    "smallc": [(CONV32, AXES + SPLITS + NS + ("nkb=1", "nkb>1", "K%32", "taps=27", "taps=1") + TAPS9 + TAPS3 + STRIDES +
                ("bias:smallc", "bias:colsum", "nobias", "reduce:f4", "reduce:f16"))],
    "mfma": [(CONV32, AXES + SPLITS + NS + BLOCKS + ("C%32", "K%32", "C2>0", "taps=27", "taps=1") + TAPS9 + TAPS3 + STRIDES +
              ("TPW=1", "TPW=4", "TPW=7", "cfg:7.2.1", "bias:generic", "nobias", "reduce:f4", "reduce:f16")),
             (CONVT32, AXES + SPLITS + NS + BLOCKS + ("C%32", "K%32", "taps=1", "taps=2", "taps=4", "taps=8", "TPW=1", "TPW=2",
                                                      "cfg:7.2.1", "cfg:7.2.0", "cfg:1.8.2", "bias:generic", "bias:colsum",
                                                      "bias:convt", "nobias", "reduce:f4", "reduce:f16"))],
    "wgrad16": [(CONV16, AXES + SPLITS + NS + BLOCKS + ("C2>0", "taps=27", "taps=1") + TAPS9 + TAPS3 + STRIDES +
                 ("TPW=1", "TPW=4", "TPW=7", "cfg:10.4.1", "cfg:7.2.1", "tri", "notri", "bias:slot28", "bias:colsum", "nobias",
                  "reduce:f4", "reduce:f16")),
                (CONVT16, AXES + SPLITS + NS + BLOCKS + ("taps=1", "taps=2", "taps=4", "taps=8", "TPW=1", "TPW=2", "cfg:7.2.1",
                                                         "cfg:7.2.0", "cfg:1.8.2", "bias:colsum", "nobias", "reduce:f4"))],
    "wgrad16z": [(CONV16, AXES_Z + SPLITS + NS + BLOCKS + ("C2>0", "bias:zmarch", "nobias", "reduce:f4"))],
    "wgrad16zs": [(CONV16, AXES_Z + SPLITS + NS + ("ncb=1", "ncb>1", "nkb=1", "nkb>1", "bias:colsum", "nobias", "reduce:f4"))],
    "scalar": [(CONV32, ("split:remainder", "split:even") + NS + ("why:C1%4", "why:C2%4", "why:K%4", "why:C2>0,C1%32",
                                                                  "why:engine", "bias:colsum", "nobias", "reduce:d")),
               (CONVT32, ("split:remainder", "split:even", "N=1", "N=2", "why:C1%4", "why:K%4", "bias:colsum", "nobias",
                          "reduce:d"))],
}
# cells no entry point can reach, each with the reason; test_unreachable_cells_stay_unreached scans for them
UNREACHABLE = {
    ("mfma", "cfg:1.8.0"): "k_wgrad_mfma<TPW, 1, 8, 0>: the (1, 8) tile configuration is chosen only when the dy halo of a "
                           "transposed conv does not fit (7, 2), and every tap of a transposed conv reads the same x slot (SH 2)",
    ("wgrad16", "cfg:1.8.0"): "k_wgrad16<TPW, 1, 8, 0>: as for k_wgrad_mfma",
    ("mfma", "cfg:1.8.1"): "no such instantiation: SH 1 belongs to the (7, 2) configuration",
    ("wino", "TW=4"): "k_wgrad_wino<13, 4, 2> (tiles 4 wide): a plain 3x3x3 stride-1 problem always fits the first fp32 tile "
                      "candidate, 2x8x8 (400 halo slots of 416), so the Winograd branch never sees another tile",
    ("wino2w12", "fallback:wino"): "k_wgrad_wino under MVD_WINO=2 (the workspace fallback of k_wgrad_wino2w12): the entry "
                                   "points refuse a workspace below the query, and the query holds the 48-position partials",
    ("wino3", "fallback:wino2w12"): "k_wgrad_wino2w12 for a shape k_wgrad_wino3 selected (its workspace fallback): the query "
                                    "holds the 64-position partials at the fp32 split count",
    ("wgrad16z", "fallback:wgrad16"): "k_wgrad16 for a shape of k_wgrad16z with the kernel on (its workspace fallback): the "
                                      "query holds nsplit <= 256 / blocks partials and one bias row each",
    ("wgrad16", "nobiasrows"): "k_wgrad16 with 27 taps and dbias asked for but no room for the bias rows: the query holds them",
    ("mfma", "nobiasrows"): "k_wgrad_mfma / k_wgrad_smallc without their bias rows for want of room: the query holds them",
    ("any", "error:workspace"): "the two 'workspace too small' errors of the plan: the query holds two partials per split",
}


def wanted():
    return {(k, cl, *t) for k, rows in MATRIX.items() for t, cls in rows for cl in cls}


def cells_of(p, c):
    return {(R.KERNEL_NAMES[p.kernel], cl, c.kind, c.dt) for cl in R.classes(p, c)}


_child_cache = {}


def env_plans(cases):
    """plans of the cases that need a process-start switch, from ONE fresh child process per environment"""
    out = {}
    for env in sorted({c.env for c in cases if c.env}):
        todo = [c for c in cases if c.env == env]
        key = (env, tuple(todo))
        if key not in _child_cache:
            code = ("import sys, json; sys.path.insert(0, 'tests'); import wgrad_ref as R; from multimodal_mvd_seg_amd import _lib; "
                    "_lib.load(); todo = [c for c in R.CASES if c.env == tuple(map(tuple, json.loads(sys.argv[1])))]; "
                    "print(json.dumps([list(R.plan_of(c) or ()) for c in todo]))")
            e = dict(os.environ, PYTHONPATH=ROOT, **dict(env))
            r = subprocess.run([sys.executable, "-c", code, json.dumps(env)], env=e, cwd=ROOT, capture_output=True, text=True,
                               timeout=300)
            assert r.returncode == 0, r.stderr
            plans = json.loads(r.stdout.strip().splitlines()[-1])
            full = [c for c in R.CASES if c.env == env]
            _child_cache[key] = {c: (R.Plan(*p) if p else None) for c, p in zip(full, plans)}
        out.update({c: _child_cache[key][c] for c in todo})
    return out


def plans(cases):
    got = {c: R.plan_of(c) for c in cases if not c.env}
    got.update(env_plans(cases))
    return got


@pytest.fixture(scope="module")
def case_plans():
    return plans(R.CASES)


def test_matrix_names_every_kernel_of_the_header():
    assert set(MATRIX) == set(R.KERNEL_NAMES[1:])
    src = open(os.path.join(ROOT, "include", "mvdseg_hip.h")).read()
    ids = dict(re.findall(r"#define MVD_WG_(\w+) (\d+)", src))
    assert int(ids.pop("PLAN_LEN")) == R.PLAN_LEN
    assert {n.lower(): int(v) for n, v in ids.items()} == {n: i for i, n in enumerate(R.KERNEL_NAMES)}
    assert {n.lower(): int(v) for n, v in re.findall(r"#define MVD_WGR_(\w+) (\d+)", src)} == \
        {n: i for i, n in enumerate(R.REDUCE_NAMES) if i}
    assert {n.lower(): int(v) for n, v in re.findall(r"#define MVD_WGB_(\w+) (\d+)", src)} == {n: i for i, n in enumerate(R.BIAS_NAMES)}


def test_every_cell_of_the_matrix_has_a_case(case_plans):
    got = set().union(*(cells_of(p, c) for c, p in case_plans.items() if p))
    missing = wanted() - got
    assert not missing, sorted(missing)


def test_coverage_test_notices_an_emptied_cell(case_plans):
    """the check above is not vacuous: without the cases that sit in a cell, that cell is missing"""
    per_case = {c: cells_of(p, c) for c, p in case_plans.items() if p}
    for cell in sorted(wanted()):
        kept = [c for c in per_case if cell not in per_case[c]]
        assert len(kept) < len(per_case), cell
        assert cell not in set().union(*(per_case[c] for c in kept)), cell


@pytest.mark.parametrize("c", [c for c in R.CASES if not c.env], ids=R.case_id)
def test_case_runs_the_kernel_and_sits_in_the_classes_it_declares(c):
    _check_case(c, R.plan_of(c))


def test_cases_under_a_process_start_switch(case_plans):
    todo = [c for c in R.CASES if c.env]
    assert todo and {c.env for c in todo} == {(("MVD_WINO", "1"),)}
    for c in todo:
        _check_case(c, case_plans[c])
        assert case_plans[c].wino_mode == 1


def _check_case(c, p):
    assert p is not None, f"{R.case_id(c)}: refused"
    assert p.kernel == c.kernel, f"{R.case_id(c)}: runs {R.KERNEL_NAMES[p.kernel]}, the case declares {R.KERNEL_NAMES[c.kernel]}"
    names = R.classes(p, c)
    assert set(c.why) <= names, f"{R.case_id(c)}: declared {set(c.why) - names}, the plan gives {sorted(names)}"
    x = c.N * c.sp[0] * c.sp[1] * c.sp[2] * (c.C1 + c.C2)
    assert x <= 1 << 23 and p.ws_bytes <= 600 << 20, "operands of a case: at most 8 M elements"
    assert 1 <= p.nsplit <= p.ntiles and p.needed_ws <= p.ws_bytes == R.workspace_bytes(c)


def test_table_is_well_formed():
    assert len({R.case_id(c) for c in R.CASES}) == len(R.CASES)
    for k in range(1, len(R.KERNEL_NAMES)):
        assert any(c.kernel == k and not c.bias for c in R.CASES), f"no dbias == NULL case for {R.KERNEL_NAMES[k]}"
    assert {c.N for c in R.CASES} >= {1, 2, 3}


# ------------------------------------------------------------------------------------------------ the scan grid
KS = list(itertools.product((1, 3), repeat=3))
ST = list(itertools.product((1, 2), repeat=3))
# extents with a value on each side of Wo 32, Ho / Do 8 and 4 (after stride 2 as well), tile edges, N Do Ho Wo 2^15
SHAPES = [(1, 1, 1), (3, 3, 3), (4, 4, 32), (3, 4, 31), (7, 7, 31), (7, 8, 32), (8, 7, 32), (8, 8, 31), (8, 8, 32), (8, 8, 33),
          (9, 10, 17), (5, 6, 7), (16, 16, 16), (7, 15, 63), (8, 16, 64), (7, 8, 64), (8, 7, 64), (15, 15, 65), (16, 16, 66),
          (32, 32, 31), (32, 32, 32), (32, 33, 31), (38, 36, 28), (34, 44, 52), (64, 64, 64), (128, 128, 128)]
CHANNELS = [(4, 0, 4), (4, 0, 32), (8, 0, 32), (8, 0, 36), (12, 0, 32), (16, 0, 16), (24, 0, 48), (32, 0, 32), (32, 0, 64),
            (32, 0, 96), (64, 0, 32), (64, 0, 128), (32, 32, 32), (64, 32, 64), (256, 0, 256), (320, 0, 320), (512, 512, 512),
            (3, 0, 32), (5, 0, 32), (32, 0, 3), (32, 0, 30), (32, 5, 32), (24, 8, 32), (2, 0, 2), (1, 0, 1), (32, 16, 32),
            (36, 0, 32)]
SETTINGS = [{}, {"wino3_min": 1}, {"wino3_min": 1 << 40}, {"bias_fold": 0}, {"bf16_kernel": 0}, {"engine": 1}]


def grid():
    for (C1, C2, K), sp, N in itertools.product(CHANNELS, SHAPES, (1, 2, 3)):
        big = sp[0] * sp[1] * sp[2] >= 1 << 17
        for kind in ("conv", "convT"):
            if kind == "convT" and C2:
                continue
            for dt in ("fp32", "bf16"):
                for ks, st in (itertools.product(KS, ST) if kind == "conv" else (((1, 1, 1), s) for s in ST)):
                    if big and (ks not in ((3, 3, 3), (1, 1, 1)) or st not in ((1, 1, 1), (2, 2, 2))):
                        continue   # the two largest volumes: the flagship's layers only
                    yield kind, dt, N, C1, C2, K, sp, ks, st


def plan_at(kind, dt, N, C1, C2, K, sp, ks, st, ws_bytes=0, bias=1):
    return R.raw_plan(kind == "convT", dt == "bf16", N, sp, C1, C2, K, ks, st, ws_bytes, bias)


def _scan(settings):
    """[(point, bias, plan at the queried workspace, plan at an unlimited one)] under one set of setter values"""
    c = R.C("conv", "fp32", 1, 4, 0, 4, (1, 1, 1), (1, 1, 1), (1, 1, 1), 0, **settings)
    out = []
    with R.applied(c):
        for pt in grid():
            if settings and (pt[6][0] >= 64 or pt[7] not in ((3, 3, 3), (1, 1, 1))):
                continue   # the setters move the 27-tap and the bias decisions only; they skip the largest volumes
            for bias in (1, 0):
                out.append((pt, bias, plan_at(*pt, 0, bias), plan_at(*pt, 1 << 62, bias)))
    return out


@pytest.fixture(scope="module")
def scans():
    return {json.dumps(s): _scan(s) for s in SETTINGS}


def _decisions(p):
    return p[:21] if p else None   # everything up to the workspace the plan was made for


def test_plan_invariants_over_the_scan_grid(scans):
    """  * the plan at the queried workspace equals the plan at an unlimited one: the query never costs a shape its preferred
         kernel or its in-kernel bias rows;
       * k_wgrad_scalar only for C1 % 4, C2 % 4, K % 4, C < 4, K < 4, C2 > 0 with C1 % 32, or the scalar engine mode;
       * bf16 never refuses a shape with C1, C2, K multiples of 32 (and refuses every other);
       * 1 <= nsplit <= ntiles, needed_ws <= ws_bytes."""
    n = 0
    for key, rows in scans.items():
        engine = json.loads(key).get("engine", 0)
        for pt, bias, p, pinf in rows:
            kind, dt, N, C1, C2, K, sp, ks, st = pt
            assert _decisions(p) == _decisions(pinf), (key, pt, bias, p, pinf)
            if dt == "bf16":
                assert (p is not None) == (C1 % 32 == 0 and C2 % 32 == 0 and K % 32 == 0), (key, pt)
                if p is None:
                    continue
            assert p is not None and p.kernel != R.NONE, (key, pt)
            if p.kernel == R.SCALAR:
                assert C1 % 4 or C2 % 4 or K % 4 or C1 + C2 < 4 or K < 4 or (C2 > 0 and C1 % 32) or engine, (key, pt, p)
            else:
                assert not (dt == "fp32" and engine), (key, pt, p)
            assert 1 <= p.nsplit <= p.ntiles and p.needed_ws <= p.ws_bytes, (key, pt, p)
            assert (p.bias == 0) == (bias == 0) and (p.bias_rows > 0) == (p.bias >= 2), (key, pt, p)
            n += 1
    assert n > 100000


def test_unreachable_cells_stay_unreached(scans):
    """no shape of the grid reaches a cell marked unreachable; each has a reason"""
    assert all(len(r) > 40 for r in UNREACHABLE.values())
    for key, rows in scans.items():
        s = json.loads(key)
        for pt, bias, p, pinf in rows:
            if p is None:
                continue
            kind, dt, N, C1, C2, K, sp, ks, st = pt
            if p.kernel in (R.MFMA, R.WGRAD16):
                assert (p.NA, p.NB, p.SH) in ((7, 2, 1), (7, 2, 0), (1, 8, 2), (10, 4, 1)), (pt, p)    # cfg:1.8.0, cfg:1.8.1
            if p.kernel in (R.WINO, R.WINO2W12):
                assert (p.TD, p.TH, p.TW) == (2, 8, 8), (pt, p)                                        # TW=4
            plain = kind == "conv" and ks == (3, 3, 3) and st == (1, 1, 1)
            c32 = C1 % 32 == 0 and C2 % 32 == 0 and K % 32 == 0
            if dt == "fp32" and plain and c32 and not s.get("engine"):                              # the workspace fallbacks
                assert p.kernel in (R.WINO3, R.WINO2W12) and p.bias in (0, 5, 6), (pt, p)
                if s.get("wino3_min") == 1 and p.kernel != R.WINO3:
                    assert 16 * sp[1] * sp[2] * max(C1, C2, K // 2) >= 1 << 31, (pt, p)   # only its 31-bit buffer range refuses
            if dt == "bf16" and plain and sp[2] >= 32 and sp[1] >= 8 and sp[0] >= 8 and s.get("bf16_kernel", 1):
                assert p.kernel == R.WGRAD16Z and (p.bias == 8 or not bias), (pt, p)
            if bias and p.kernel == R.WGRAD16 and R.ntaps(R.C(kind, dt, N, C1, C2, K, sp, ks, st, 0)) == 27:
                assert p.bias == 7, (pt, p)                                                            # nobiasrows
            if bias and p.kernel == R.SMALLC and s.get("bias_fold", 1):
                assert p.bias == 4, (pt, p)
            if bias and p.kernel == R.MFMA and p.SH == 1:
                assert p.bias == 2, (pt, p)
            if bias and p.kernel == R.MFMA and p.SH == 2 and s.get("bias_fold", 1) and R.ntaps(R.C(kind, dt, N, C1, C2, K, sp, ks, st, 0)) in (4, 8):
                assert p.bias == 3, (pt, p)


def test_thresholds_sit_where_the_table_assumes():
    P = plan_at
    k3, k1, s1, s2 = (3, 3, 3), (1, 1, 1), (1, 1, 1), (2, 2, 2)
    # bf16 z-marching: Wo >= 32, Ho >= 8, Do >= 8; its stride-2 twin: Wo >= 32, Ho, Do >= 4, K % 64, units x blocks >= 128
    assert [P("conv", "bf16", 1, 32, 0, 32, sp, k3, s1).kernel for sp in ((8, 8, 32), (8, 8, 31), (8, 7, 32), (7, 8, 32))] == \
        [R.WGRAD16Z, R.WGRAD16, R.WGRAD16, R.WGRAD16]
    assert P("conv", "bf16", 3, 64, 0, 128, (15, 17, 65), k3, s2).kernel == R.WGRAD16ZS
    assert P("conv", "bf16", 3, 64, 0, 128, (15, 17, 63), k3, s2).kernel == R.WGRAD16
    assert P("conv", "bf16", 3, 64, 0, 96, (15, 17, 65), k3, s2).kernel == R.WGRAD16
    assert P("conv", "bf16", 2, 64, 0, 128, (15, 17, 65), k3, s2).kernel == R.WGRAD16      # 24 units x 4 blocks < 128
    # bf16 256-voxel tile: N Do Ho Wo >= 2^15
    assert P("conv", "bf16", 1, 32, 0, 32, (32, 33, 31), k3, s1)[3:11] == (7, 7, 2, 1, 1, 2, 8, 8)     # 32 736 voxels
    assert P("conv", "bf16", 1, 32, 0, 32, (32, 34, 31), k3, s1)[3:11] == (7, 10, 4, 1, 1, 4, 8, 8)    # 33 728
    # fp32: the narrow-input kernel up to 8 channels and 128 (tap, channel) rows
    assert [P("conv", "fp32", 1, C, 0, 32, (5, 6, 7), ks, s1).kernel for C, ks in ((4, k3), (8, k3), (8, (1, 3, 3)), (12, k1))] == \
        [R.SMALLC, R.MFMA, R.SMALLC, R.MFMA]
    # the wino3 item minimum, through its setter (items per sample: 4 x 1 x 1 x 1 x 1 at 8^3, 32 -> 32)
    for m, k in ((4, R.WINO3), (5, R.WINO2W12)):
        with R.applied(R.C("conv", "fp32", 1, 32, 0, 32, (8, 8, 8), k3, s1, 0, wino3_min=m)):
            assert P("conv", "fp32", 1, 32, 0, 32, (8, 8, 8), k3, s1).kernel == k


def test_plan_refuses_what_the_entry_points_refuse():
    k3, s1 = (3, 3, 3), (1, 1, 1)
    for bad in (dict(N=0), dict(sp=(0, 8, 8)), dict(K=0), dict(C1=0), dict(C2=-1), dict(ks=(2, 3, 3)), dict(st=(3, 1, 1)),
                dict(ks=(5, 3, 3)), dict(ws=1), dict(tr=1, C2=32), dict(tr=1, st=(3, 1, 1)), dict(pro=1), dict(pro=1, bf=1, C2=32),
                dict(pro=1, bf=1, sp=(8, 8, 16)), dict(bf=1, C1=24)):
        a = dict(tr=0, bf=0, N=1, sp=(8, 8, 32), C1=32, C2=0, K=32, ks=k3, st=s1, ws=0, pro=0)
        a.update(bad)
        assert R.raw_plan(a["tr"], a["bf"], a["N"], a["sp"], a["C1"], a["C2"], a["K"], a["ks"], a["st"], a["ws"], 1, a["pro"]) is None, bad
    p = R.raw_plan(0, 1, 1, (8, 8, 32), 32, 0, 32, k3, s1, 0, 1, 1)
    assert p.kernel == R.WGRAD16Z and p.bias == 8
    lib = _lib.load()
    assert lib.mvd_conv_wgrad_plan(0, 0, 1, 8, 8, 8, 32, 0, 32, _lib.i3(k3), _lib.i3(s1), 0, 1, 0, None) == 2
    assert lib.mvd_conv_wgrad_last_kernel() in range(len(R.KERNEL_NAMES))
