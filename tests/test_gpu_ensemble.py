"""GPU tests of model ensembling (csrc/export.hip: k_export_ensemble, k_ensemble_mean_argmax; csrc/infer.hip:
k_sw_normalize_add; ensembling.py; SlidingWindowPredictor.predict_logits_from_preprocessed_data).

Inputs.  Logits are export_ref.smooth_logits(K, shape, seed, std=2.0) -- not the std 8 of test_gpu_export.py: saturated,
independent members put the MEAN's near-ties between the members' favourite classes (at M = 3, K = 5 and std 8, 2.0e-2 of
the voxels lie under a 1e-4 margin); with std 2 at most 2.7e-4 lie under 4e-5 for M in {2, 3} and K in {2, 5, 8}.

Tolerances, derived as in test_gpu_export.py.  A member's fp32 probability is within 1e-5 of the fp64 oracle (three fp32
lerps, softmax derivative <= 1/4, its own rounding below 1e-6).  The mean of M of them keeps that bound, and the M adds and
the division add at most (M + 1) 2^-24 (values <= M, then <= 1): 1.1e-5 covers M <= 8.  Two channels off by 1.1e-5 each
cannot swap when the oracle's top-2 margin of the mean is at least 4e-5, so labels must be EQUAL there; the share of voxels
under the margin is asserted to be at most 1e-3.  Everything that compares two device routes, or the device with an fp32
numpy restatement in the same order, is bit-exact.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ensemble_ref as EREF
import export_ref as REF
from conftest import load_npz
from multimodal_mvd_seg_amd import ensembling as ENS
from multimodal_mvd_seg_amd import export as EX

DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu

MEAN_TOL = 1.1e-5
MARGIN = 4e-5
MAX_EXCLUDED = 1e-3

# member shape, separate-z axis; M = 8 cycles through them with new seeds
MEMBERS = [((37, 45, 52), None), ((25, 61, 33), 0), ((40, 27, 23), None)]
TARGET = (41, 53, 47)                                   # 102131 voxels: odd, the tail of the four-voxel walk runs
PLACEMENTS = {"pasted": ((46, 55, 57), (3, 1, 7), (2, 0, 1)), "identity": (TARGET, (0, 0, 0), (0, 1, 2))}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from multimodal_mvd_seg_amd import _lib
    _lib.load()


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def members(M, K):
    xs = [REF.smooth_logits(K, MEMBERS[m % 3][0], seed=100 + 10 * K + m, std=2.0) for m in range(M)]
    return xs, [MEMBERS[m % 3][1] for m in range(M)]


@functools.lru_cache(maxsize=None)
def oracle(M, K, place):
    xs, axes = members(M, K)
    full, lo, tb = PLACEMENTS[place]
    return EREF.ensemble(xs, TARGET, full, lo, tb, axes)


@functools.lru_cache(maxsize=None)
def fused(M, K, place):
    xs, axes = members(M, K)
    full, lo, tb = PLACEMENTS[place]
    return ENS.ensemble_logits_to_segmentation([G(x) for x in xs], TARGET, full, lo, tb, axes, return_probabilities=True)


def check(seg, mean, seg_ref, mean_ref, mar, inside, what):
    err = float(np.abs(mean.astype(np.float64) - mean_ref).max())
    low = mar < MARGIN
    share = float(low.mean())
    mism = int(((seg != seg_ref) & ~low).sum())
    print(f"{what}: voxels {seg.size}, max |mean - oracle| {err:.3e}, under the margin {share:.2e}, mismatches above it "
          f"{mism}, mismatches in all {int((seg != seg_ref).sum())}")
    assert np.isfinite(mean).all() and err <= MEAN_TOL, err
    assert share <= MAX_EXCLUDED, share
    assert mism == 0, mism
    assert not seg[~inside].any() and (mean[0][~inside] == 1).all() and not mean[1:][:, ~inside].any()


# ------------------------------------------------------------------------------------------------ 1: fused vs fp64
@pytest.mark.parametrize("place", ["pasted", "identity"])
@pytest.mark.parametrize("K", [2, 5, 8])
@pytest.mark.parametrize("M", [1, 2, 3, 8])
def test_fused_ensemble_matches_the_fp64_oracle(M, K, place):
    seg_ref, mean_ref, mar, inside = oracle(M, K, place)
    seg, mean = fused(M, K, place)
    assert seg.dtype == torch.uint8 and tuple(seg.shape) == seg_ref.shape and tuple(mean.shape) == mean_ref.shape
    assert seg.is_contiguous() and mean.dtype == torch.float32
    check(seg.cpu().numpy(), mean.cpu().numpy(), seg_ref, mean_ref, mar, inside, f"M {M} K {K} {place}")
    assert len(np.unique(seg_ref)) == K, "every class must win somewhere"
    only = ENS.ensemble_logits_to_segmentation([G(x) for x in members(M, K)[0]], TARGET, *PLACEMENTS[place],
                                               members(M, K)[1])
    assert torch.equal(only, seg)                      # the labels-only instantiation


# ------------------------------------------------------------------------------------------------ 2: fused vs chain
def chain(xs, axes, new, full, lo, tb):
    probs = [EX.resize_logits_to_segmentation(x, new, full, lo, tb, ax, return_probabilities=True)[1]
             for x, ax in zip(xs, axes)]
    mean = ENS.average_probabilities(probs)
    seg, mean2 = ENS.merge_probabilities(probs, None, save_probabilities=True)
    assert torch.equal(bits(mean), bits(mean2))
    return seg, mean


@pytest.mark.parametrize("place", ["pasted", "identity"])
@pytest.mark.parametrize("K", [2, 5, 8])
@pytest.mark.parametrize("M", [1, 2, 3, 8])
def test_fused_ensemble_is_bit_identical_to_the_unfused_device_chain(M, K, place):
    xs, axes = members(M, K)
    full, lo, tb = PLACEMENTS[place]
    seg_c, mean_c = chain([G(x) for x in xs], axes, TARGET, full, lo, tb)
    seg, mean = fused(M, K, place)
    assert torch.equal(seg, seg_c)
    assert torch.equal(bits(mean), bits(mean_c))


def test_fused_ensemble_is_bit_identical_to_the_chain_at_full_size():
    K, shape, new = 8, (192, 256, 256), (288, 384, 384)
    g = torch.Generator(device=DEV).manual_seed(5)
    xs = [torch.randn((K, *shape), generator=g, device=DEV) * 2 for _ in range(2)]
    seg_c, mean_c = chain(xs, [None, 0], new, new, (0, 0, 0), (0, 1, 2))
    seg, mean = ENS.ensemble_logits_to_segmentation(xs, new, new, (0, 0, 0), (0, 1, 2), [None, 0],
                                                    return_probabilities=True)
    assert tuple(seg.shape) == new and int(seg.max()) == K - 1
    assert torch.equal(seg, seg_c)
    assert torch.equal(bits(mean), bits(mean_c))
    del mean_c, seg_c
    assert torch.equal(ENS.ensemble_logits_to_segmentation(xs, new, new, (0, 0, 0), (0, 1, 2), [None, 0]), seg)


# ------------------------------------------------------------------------------------------------ 3: stored probabilities
def _probs(M, K, n, seed):
    rng = np.random.default_rng(seed)
    return [torch.softmax(torch.from_numpy((rng.standard_normal((K, n)) * 2).astype(np.float32)), 0).numpy()
            for _ in range(M)]


@pytest.mark.parametrize("n", [1, 3, 4, 1021, 4096])
@pytest.mark.parametrize("K", [2, 8])
@pytest.mark.parametrize("M", [1, 2, 8])
def test_mean_argmax_is_bit_equal_to_numpy_in_the_same_order(M, K, n):
    ps = _probs(M, K, n, 7 * M + K + n)
    seg_ref, mean_ref = EREF.merge(ps)
    dev = [G(p) for p in ps]
    seg, mean = ENS.merge_probabilities(dev, None, save_probabilities=True)
    assert seg.dtype == torch.uint8 and tuple(seg.shape) == (n,) and tuple(mean.shape) == (K, n)
    assert np.array_equal(mean.cpu().numpy().view(np.uint32), mean_ref.view(np.uint32))
    assert np.array_equal(seg.cpu().numpy(), seg_ref)
    assert torch.equal(ENS.merge_probabilities(dev, None), seg)
    assert torch.equal(bits(ENS.average_probabilities(dev)), bits(mean))
    # every base one element off a 16-byte boundary: the scalar route, the same result
    off = []
    for p in ps:
        buf = torch.empty(K * n + 1, dtype=torch.float32, device=DEV)
        buf[1:] = G(p).reshape(-1)
        off.append(buf[1:].view(K, n))
        assert off[-1].data_ptr() % 16 == 4 and off[-1].is_contiguous()
    seg2, mean2 = ENS.merge_probabilities(off, None, save_probabilities=True)
    assert torch.equal(seg2, seg) and torch.equal(bits(mean2), bits(mean))
    for p, d in zip(ps, dev):
        assert np.array_equal(d.cpu().numpy(), p)      # the inputs are left alone


def test_mean_argmax_exact_ties_go_to_the_lowest_index_and_other_dtypes_are_raised_first():
    n = 1021
    rng = np.random.default_rng(3)
    base = (rng.integers(0, 8, size=(3, n)) / 32.0).astype(np.float32)       # multiples of 1/32: every sum is exact
    a = np.stack([base[0], base[1], base[1], base[2], base[1]])              # channels 1, 2 and 4 tie everywhere
    b = np.stack([base[2], base[0], base[0], base[1], base[0]])
    seg_ref, mean_ref = EREF.merge([a, b])
    assert not np.isin(seg_ref, (2, 4)).any() and (seg_ref == 1).any()
    seg, mean = ENS.merge_probabilities([G(a), G(b)], None, save_probabilities=True)
    assert np.array_equal(seg.cpu().numpy(), seg_ref) and np.array_equal(mean.cpu().numpy(), mean_ref)
    assert not ENS.merge_probabilities([torch.zeros((4, 6, 5, 7), device=DEV)] * 3, None).any()
    # volumes keep their shape; fp16 / fp64 members are raised to fp32 first (ensemble.py:24-25)
    ps = _probs(3, 4, 6 * 5 * 7, 9)
    ref_seg, ref_mean = EREF.merge([ps[0].astype(np.float16).astype(np.float32), ps[1], ps[2]])
    seg, mean = ENS.merge_probabilities([G(ps[0]).half().view(4, 6, 5, 7), G(ps[1]).view(4, 6, 5, 7),
                                         G(ps[2]).double().view(4, 6, 5, 7)], None, save_probabilities=True)
    assert tuple(seg.shape) == (6, 5, 7) and mean.dtype == torch.float32
    assert np.array_equal(mean.cpu().numpy().reshape(4, -1), ref_mean) and np.array_equal(seg.cpu().numpy().ravel(), ref_seg)


def test_stored_probabilities_route_reproduces_the_reference_fixture():
    from multimodal_mvd_seg_amd import trainer
    z = load_npz("ensemble.npz")
    lm = trainer.LabelManager({"background": 0, "a": 1, "b": 2})
    probs = [G(p) for p in z["probabilities"]]
    seg, mean = ENS.merge_probabilities(probs, lm, save_probabilities=True)
    assert np.array_equal(mean.cpu().numpy().view(np.uint32), z["mean"].view(np.uint32))
    assert np.array_equal(seg.cpu().numpy(), z["segmentation"])
    seg, mean = ENS.merge_probabilities([G(z["first_f16"])] + probs[1:], lm, save_probabilities=True)
    assert np.array_equal(mean.cpu().numpy().view(np.uint32), z["mean_f16first"].view(np.uint32))
    assert np.array_equal(seg.cpu().numpy(), z["segmentation_f16first"])
    # ensemble_crossvalidations: two models, the second one split over folds, cases in a different order
    a, b = {"c0": probs[0], "c1": probs[1]}, [{"c1": probs[2]}, {"c0": probs[1]}]
    out = ENS.ensemble_crossvalidations([a, b], lm, save_probabilities=True)
    assert list(out) == ["c0", "c1"]
    for case, ms in (("c0", [probs[0], probs[1]]), ("c1", [probs[1], probs[2]])):
        s, m = ENS.merge_probabilities(ms, lm, save_probabilities=True)
        assert torch.equal(out[case][0], s) and torch.equal(bits(out[case][1]), bits(m))
    with pytest.raises(ValueError, match="segmentation heads"):
        ENS.merge_probabilities([torch.zeros((4, 5), device=DEV)], lm)


# ------------------------------------------------------------------------------------------------ 4: the fold loop's tail
@pytest.mark.parametrize("M", [1, 2, 3])
def test_sw_normalize_add_is_bit_equal_to_normalize_plus_torch_add_and_divide(M):
    from multimodal_mvd_seg_amd._lib import call
    K, V = 3, 40 * 45 * 36 + 1
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device=DEV).manual_seed(M)
    accs = [torch.randn((K, V), generator=g, device=DEV) * 1000 for _ in range(M)]
    npreds = [torch.rand((V,), generator=g, device=DEV) * 3000 + 1 for _ in range(M)]
    ref = None
    for acc, npred in zip(accs, npreds):
        one = acc.clone()
        call("mvd_sw_normalize", P(one), P(npred), K, V, s)
        if ref is None:
            ref = one
        else:
            ref += one
    if M > 1:
        ref /= M
    total = None
    for i, (acc, npred) in enumerate(zip(accs, npreds)):
        mine = acc.clone()
        if total is None:
            total = mine                                # the first fold in place, as the predictor does
        call("mvd_sw_normalize_add", P(total), P(mine), P(npred), K, V, int(i == 0), int(i == M - 1), M, s)
    assert torch.equal(bits(total), bits(ref))
    # a separate sum buffer gives the same
    out = torch.full((K, V), float('nan'), device=DEV)
    for i, (acc, npred) in enumerate(zip(accs, npreds)):
        call("mvd_sw_normalize_add", P(out), P(acc), P(npred), K, V, int(i == 0), int(i == M - 1), M, s)
    assert torch.equal(bits(out), bits(ref))


# ------------------------------------------------------------------------------------------------ 5: fold prediction
DS = {"channel_names": {"0": "a", "1": "b"}, "labels": {"background": 0, "a": 1, "b": 2}}


def _net(dim, seed):
    from multimodal_mvd_seg_amd import trainer
    strides = [[1] * dim, [2] * dim, [2] * dim]
    base = 8 if dim == 3 else 32
    plans = trainer.make_plans((32,) * dim, strides, base_features=base, max_features=4 * base,
                               configuration='3d_fullres' if dim == 3 else '2d')
    pm = trainer.PlansManager(plans)
    torch.manual_seed(seed)
    net = trainer.get_network_from_plans(pm, DS, pm.get_configuration('3d_fullres' if dim == 3 else '2d'), 2,
                                         deep_supervision=True)
    return net.to(DEV)


@pytest.mark.parametrize("dim", [3, 2])
def test_fold_prediction_equals_separately_built_networks_summed_in_fold_order(dim):
    from multimodal_mvd_seg_amd.inference import SlidingWindowPredictor
    patch = (32,) * dim
    kw = dict(tile_step_size=0.5, use_gaussian=True, use_mirroring=True, allowed_mirroring_axes=(1,), device=DEV)
    rng = np.random.default_rng(dim)
    img = torch.from_numpy(rng.standard_normal((2, 40, 45, 36)).astype(np.float32) if dim == 3 else
                           rng.standard_normal((2, 5, 45, 36)).astype(np.float32))
    nets = [_net(dim, 11 + i) for i in range(3)]
    sds = [{k: v.detach().clone() for k, v in n.state_dict().items()} for n in nets]
    assert sum(not torch.equal(sds[0][k], sds[1][k]) for k in sds[0]) > 10, "the folds must differ"
    singles = [SlidingWindowPredictor(n, patch, 3, **kw).predict_sliding_window_return_logits(img) for n in nets]
    assert not torch.equal(singles[0], singles[1]) and not torch.equal(singles[1], singles[2])
    want = singles[0].clone()
    want += singles[1]
    want += singles[2]
    want /= 3
    net = _net(dim, 99)
    pred = SlidingWindowPredictor(net, patch, 3, list_of_parameters=sds, **kw)
    got = pred.predict_logits_from_preprocessed_data(img)
    assert tuple(got.shape) == (3, *img.shape[1:])
    assert torch.equal(bits(got), bits(want))
    assert net.training and net.decoder.deep_supervision is True          # restored
    for k, v in net.state_dict().items():                                   # the last fold stays loaded
        assert torch.equal(v, sds[2][k]), k
    # a second pass through the list: fold 0 is loaded over fold 2 -- stale packed weights would show here
    assert torch.equal(bits(pred.predict_logits_from_preprocessed_data(img)), bits(want))
    # one fold, and no list: the single-model prediction itself
    one = SlidingWindowPredictor(net, patch, 3, list_of_parameters=[sds[1]], **kw)
    assert torch.equal(bits(one.predict_logits_from_preprocessed_data(img)), bits(singles[1]))
    none = SlidingWindowPredictor(nets[0], patch, 3, **kw)
    assert torch.equal(bits(none.predict_logits_from_preprocessed_data(img)), bits(singles[0]))
    assert torch.equal(bits(none.predict_sliding_window_return_logits(img)), bits(singles[0]))


# ------------------------------------------------------------------------------------------------ 6: plans and properties
def test_ensemble_predictions_reads_plans_and_properties_like_the_single_model_export():
    from multimodal_mvd_seg_amd import trainer
    tb = [1, 2, 0]
    plans = trainer.make_plans((32, 32, 32), [[1, 1, 1], [2, 2, 2]], spacing=(3.2, 1.0, 1.0))
    plans['configurations']['2d'] = trainer.make_plans((32, 32), [[1, 1], [2, 2]], configuration='2d',
                                                       spacing=(0.9, 0.9))['configurations']['2d']
    plans['transpose_forward'], plans['transpose_backward'] = [2, 0, 1], tb
    pm = trainer.PlansManager(plans)
    lm = pm.get_label_manager({"labels": {"background": 0, "a": 1, "b": 2, "c": 3}})
    c3, c2 = pm.get_configuration('3d_fullres'), pm.get_configuration('2d')
    props = {'shape_before_cropping': (50, 70, 61), 'bbox_used_for_cropping': [[3, 48], [0, 63], [5, 61]],
             'shape_after_cropping_and_before_resampling': (45, 63, 56), 'spacing': [2.5, 0.9, 0.9]}
    x3 = REF.smooth_logits(4, (36, 44, 40), seed=21, std=2.0)     # 3d_fullres: spacing (3.2, 1, 1), axis 0 on its own
    x2 = REF.smooth_logits(4, (45, 57, 50), seed=22, std=2.0)     # 2d: (2.5, 0.9, 0.9) by the case's z spacing, no such axis
    seg, mean = ENS.ensemble_predictions([(G(x3), c3), (G(x2), c2)], pm, lm, props, return_probabilities=True)
    lo = [b[0] for b in props['bbox_used_for_cropping']]
    seg_ref, mean_ref, mar, inside = EREF.ensemble([x3, x2], props['shape_after_cropping_and_before_resampling'],
                                                   props['shape_before_cropping'], lo, tb, [0, None])
    assert tuple(seg.shape) == seg_ref.shape == (70, 61, 50)
    check(seg.cpu().numpy(), mean.cpu().numpy(), seg_ref, mean_ref, mar, inside, "ensemble_predictions 3d + 2d")
    # the same members through the single-model export and the stored-probabilities route
    probs = [EX.convert_predicted_logits_to_segmentation_with_correct_shape(G(x), pm, c, lm, props,
                                                                            return_probabilities=True)[1]
             for x, c in ((x3, c3), (x2, c2))]
    seg_c, mean_c = ENS.merge_probabilities(probs, lm, save_probabilities=True)
    assert torch.equal(seg, seg_c) and torch.equal(bits(mean), bits(mean_c))
    assert torch.equal(ENS.ensemble_predictions([(G(x3), c3), (G(x2), c2)], pm, lm, props), seg)
    # a non-contiguous view, as the predictor returns for an image smaller than the patch
    big = torch.zeros((4, 40, 48, 44), device=DEV)
    big[:, 2:38, 1:45, 3:43] = G(x3)
    assert torch.equal(ENS.ensemble_predictions([(big[:, 2:38, 1:45, 3:43], c3), (G(x2), c2)], pm, lm, props), seg)


# ------------------------------------------------------------------------------------------------ 7: launches and the ABI
def test_repeated_launches_agree_and_bad_arguments_are_refused_through_the_abi():
    from multimodal_mvd_seg_amd import _lib
    from multimodal_mvd_seg_amd._lib import i3
    lib = _lib.load()
    xs = [G(REF.smooth_logits(3, s, seed=30 + i, std=2.0)) for i, s in enumerate([(12, 9, 14), (7, 11, 10)])]
    new = (19, 14, 23)
    a = ENS.ensemble_logits_to_segmentation(xs, new, new, (0, 0, 0), return_probabilities=True)
    b = ENS.ensemble_logits_to_segmentation(xs, new, new, (0, 0, 0), return_probabilities=True)
    assert torch.equal(a[0], b[0]) and torch.equal(bits(a[1]), bits(b[1]))
    # on another stream
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        c = ENS.ensemble_logits_to_segmentation(xs, new, new, (0, 0, 0), return_probabilities=True)
    st.synchronize()
    assert torch.equal(a[0], c[0]) and torch.equal(bits(a[1]), bits(c[1]))
    with pytest.raises(ValueError):
        ENS.ensemble_logits_to_segmentation(xs, new, new, (1, 0, 0))
    with pytest.raises(ValueError):
        ENS.ensemble_logits_to_segmentation(xs, new, new, (0, 0, 0), (0, 1, 1))

    tables = [EX._device_tables(x.shape[1:], new, [1, 1, 1], DEV) for x in xs]
    arr = ctypes.c_void_p * 2
    lg, t0 = arr(*[x.data_ptr() for x in xs]), arr(*[t[0].data_ptr() for t in tables])
    t1, tw = arr(*[t[1].data_ptr() for t in tables]), arr(*[t[2].data_ptr() for t in tables])
    dims = (ctypes.c_int * 6)(12, 9, 14, 7, 11, 10)
    out = torch.zeros(new, dtype=torch.uint8, device=DEV)
    o = ctypes.c_void_p(out.data_ptr())
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    geom = (*new, i3(new), i3((0, 0, 0)), i3((0, 1, 2)))

    def refused(rc, word):
        msg = lib.mvd_last_error().decode()
        assert rc != 0 and word in msg and len(msg) > 10, (rc, msg)

    assert lib.mvd_export_ensemble_argmax_u8(lg, t0, t1, tw, dims, 2, 3, *geom, o, None, s) == 0
    assert torch.equal(out, a[0])
    refused(lib.mvd_export_ensemble_argmax_u8(lg, t0, t1, tw, dims, 0, 3, *geom, o, None, s), "members")
    refused(lib.mvd_export_ensemble_argmax_u8(lg, t0, t1, tw, dims, 9, 3, *geom, o, None, s), "members")
    refused(lib.mvd_export_ensemble_argmax_u8(lg, t0, t1, tw, dims, 2, 9, *geom, o, None, s), "heads")
    refused(lib.mvd_export_ensemble_argmax_u8(lg, t0, t1, tw, dims, 2, 1, *geom, o, None, s), "heads")
    refused(lib.mvd_export_ensemble_argmax_u8(None, t0, t1, tw, dims, 2, 3, *geom, o, None, s), "null")
    refused(lib.mvd_export_ensemble_argmax_u8(lg, t0, t1, tw, dims, 2, 3, *geom, None, None, s), "null")
    refused(lib.mvd_export_ensemble_argmax_u8(arr(xs[0].data_ptr(), None), t0, t1, tw, dims, 2, 3, *geom, o, None, s),
            "member 1")
    refused(lib.mvd_export_ensemble_argmax_u8(lg, t0, t1, tw, dims, 2, 3, *new, i3(new), i3((1, 0, 0)), i3((0, 1, 2)), o,
                                              None, s), "bbox")
    assert torch.equal(out, a[0])                      # a refused call writes nothing

    ps = [torch.rand((3, 8), device=DEV) for _ in range(2)]
    pp = arr(*[p.data_ptr() for p in ps])
    seg = torch.zeros(8, dtype=torch.uint8, device=DEV)
    sp = ctypes.c_void_p(seg.data_ptr())
    assert lib.mvd_ensemble_mean_argmax(pp, 2, 3, 8, sp, None, s) == 0
    refused(lib.mvd_ensemble_mean_argmax(pp, 0, 3, 8, sp, None, s), "members")
    refused(lib.mvd_ensemble_mean_argmax(pp, 9, 3, 8, sp, None, s), "members")
    refused(lib.mvd_ensemble_mean_argmax(pp, 2, 9, 8, sp, None, s), "channels")
    refused(lib.mvd_ensemble_mean_argmax(None, 2, 3, 8, sp, None, s), "null")
    refused(lib.mvd_ensemble_mean_argmax(pp, 2, 3, 8, None, None, s), "null")
    refused(lib.mvd_ensemble_mean_argmax(pp, 2, 3, 0, sp, None, s), "voxel count")
    refused(lib.mvd_sw_normalize_add(None, None, None, 3, 8, 1, 1, 1, s), "bad arguments")
    refused(lib.mvd_sw_normalize_add(sp, sp, sp, 3, 8, 1, 1, 0, s), "folds")
    torch.cuda.synchronize()
