"""The graphed train step inside the sequences a real run consists of: training interleaved with validation, checkpoint
loads, re-captures and inference -- tests/test_gpu_graph.py pins N train steps followed by one validation step only.

The captured forward reads PERSISTENT packed-weight buffers, and only Python-side stamps say whether they are current.
The invariant these tests pin: every pack a replay reads is either rewritten by the replay itself or
refreshed before it, and an eager forward that meets a stale pack in graph mode packs IN PLACE into the persistent buffer.

Every test runs twin trainers from the same weights on the same batches: E with use_hip_graph=False (the reference: the
eager step is pinned to the oracle by the rest of the suite) and G with use_hip_graph=True.  The graph holds the same
kernels in the same order, so everything is compared BIT FOR BIT: the loss of every train step, every field of every
validation_step result, every parameter and the momentum buffer at the end.  Each sequence asserts that a capture exists
(or does not exist yet) where it relies on that.  A "loaded" state comes from a trainer built under another seed, and the
test asserts that at least half of the input conv's weight elements differ, so a stale pack cannot hide in bit-identity.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
STRIDES = [[1, 1, 1], [2, 2, 2], [2, 2, 2]]
DS = {"channel_names": {str(i): f"m{i}" for i in range(4)}, "labels": {"background": 0, "a": 1, "b": 2, "c": 3, "d": 4}}
SINGLE, DUAL = "nnUNetTrainerMI355", "ContrastiveTrainerMI355"
CASES = [(SINGLE, "fp32"), (SINGLE, "bf16"), (DUAL, "bf16")]
CASE_IDS = ["single-fp32", "single-bf16", "dual-bf16-topo"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from multimodal_mvd_seg_amd import _lib
    _lib.load()


def _make(cls_name, precision, graph, seed=0):
    """the set-up of tests/test_gpu_graph.py: patch 32^3, three stages, 4 modalities, batch 2"""
    from multimodal_mvd_seg_amd import trainer
    plans = trainer.make_plans((32, 32, 32), STRIDES, batch_size=2)
    tr = getattr(trainer, cls_name)(plans, "3d_fullres", 0, DS, device=DEV)
    tr.precision = precision
    tr.use_hip_graph = graph
    if cls_name == DUAL:
        tr.use_topo = True
    torch.manual_seed(seed)
    tr.initialize()
    return tr


def _batches(tr, n):
    return [tr.make_dummy_batch(seed=100 + i) for i in range(n)]


def _first_sample(b):
    return {"data": b["data"][:1].contiguous(), "target": [t[:1].contiguous() for t in b["target"]]}


def _other_state(cls_name, precision, seed=7):
    """network.state_dict() of a trainer built under another seed: every conv weight differs"""
    o = _make(cls_name, precision, False, seed=seed)
    return {k: v.detach().clone() for k, v in o.network.state_dict().items()}


def _input_convs(net):
    got = [(n, p) for n, p in net.named_parameters() if p.dim() == 5 and p.shape[1] == 4]
    assert got, "no 4-modality input conv found"
    return got


def _assert_state_differs(tr, other):
    for n, p in _input_convs(tr.network):
        frac = float((p.detach() != other[n]).float().mean())
        assert frac >= 0.5, f"{n}: only {frac:.2f} of the loaded input-conv weight differs from the current one"


def _graph(tr):
    return tr._step_graph["graph"] if tr._step_graph is not None else None


class _Twins:
    """E (eager, the reference) and G (graph) driven through the same sequence, compared after every operation."""

    def __init__(self, cls_name, precision, E=None, G=None):
        self.E = E if E is not None else _make(cls_name, precision, False)
        self.G = G if G is not None else _make(cls_name, precision, True)
        for (n, p), (_, q) in zip(self.E.network.named_parameters(), self.G.network.named_parameters()):
            assert torch.equal(p.detach(), q.detach()), f"twins start from different weights: {n}"
        self.log, self.losses = [], []

    def both(self, fn):
        fn(self.E)
        fn(self.G)

    def train(self, batch, what="train"):
        self.log.append(what)
        a, b = self.E.train_step(batch)["loss"], self.G.train_step(batch)["loss"]
        a, b = np.asarray(a).copy(), np.asarray(b).copy()
        self.losses.append(a)
        assert np.array_equal(a, b), f"loss of op {len(self.log)} {self.log}: eager {a} graph {b}"
        assert self.E._step_graph is None

    def validate(self, batch, what="validate"):
        self.log.append(what)
        a, b = self.E.validation_step(batch), self.G.validation_step(batch)
        assert set(a) == set(b) == {"loss", "tp_hard", "fp_hard", "fn_hard"}
        for k in a:
            assert np.array_equal(a[k], b[k]), f"validation {k} at op {len(self.log)} {self.log}: eager {a[k]} graph {b[k]}"

    def end(self, ref=None):
        torch.cuda.synchronize()
        ref = ref if ref is not None else self.E
        for tr in ([self.G] if ref is self.E else [self.E, self.G]):
            for (n, p), (_, q) in zip(ref.network.named_parameters(), tr.network.named_parameters()):
                assert torch.equal(p.detach(), q.detach()), f"parameter {n} after {self.log}"
            assert torch.equal(ref.optimizer.momentum_buffer, tr.optimizer.momentum_buffer), f"momentum after {self.log}"
            assert ref.optimizer._steps == tr.optimizer._steps


def _check_packs(tr, graph_mode, precision):
    """The direct invariant: every cached pack equals a fresh pack of the CURRENT master weight, bit for bit (the padded
    entry: of the zero-padded master); in graph mode the bf16 entries are views of the persistent buffer the captured
    forward reads.  Catches a stale pack even where that weight happens not to move the loss."""
    from multimodal_mvd_seg_amd import ops
    fp = tr.optimizer.fp
    lo = hi = None
    if graph_mode and precision == "bf16":
        assert fp._pack16_buf is not None, "graph mode without a persistent bf16 pack buffer"
        buf = fp._pack16_buf[1]
        lo, hi = buf.data_ptr(), buf.data_ptr() + buf.numel() * buf.element_size()
    seen = {"_mvd_pack16": 0, "_mvd_pack16pad": 0, "_mvd_pack": 0}
    for n, w in tr.network.named_parameters():
        e = getattr(w, "_mvd_pack16", None)
        if e is not None:
            seen["_mvd_pack16"] += 1
            wf, wb = ops.pack_weight_bf16(w, e[0][1])
            assert torch.equal(e[1], wf) and torch.equal(e[2], wb), f"{n}: cached bf16 pack is not the current weight"
            if lo is not None:
                assert all(lo <= t.data_ptr() < hi for t in e[1:3]), f"{n}: bf16 pack outside the persistent buffer"
        e = getattr(w, "_mvd_pack16pad", None)
        if e is not None:
            seen["_mvd_pack16pad"] += 1
            d = w.detach()
            wp = torch.zeros((d.shape[0], e[0][1], *d.shape[2:]), dtype=torch.float32, device=d.device)
            wp[:, :d.shape[1]] = d
            wf, wb = ops.pack_weight_bf16(wp, False)
            assert torch.equal(e[1], wf) and torch.equal(e[2], wb), f"{n}: cached padded bf16 pack is not the current weight"
            if lo is not None:
                assert all(lo <= t.data_ptr() < hi for t in e[1:3]), f"{n}: padded bf16 pack outside the persistent buffer"
        e = getattr(w, "_mvd_pack", None)
        if e is not None:
            seen["_mvd_pack"] += 1
            wf, wb = ops.pack_weight(w, e.transposed)
            assert torch.equal(e.wf, wf) and torch.equal(e.wb, wb), f"{n}: cached fp32 pack is not the current weight"
    if precision == "bf16":
        assert seen["_mvd_pack16"] > 0 and seen["_mvd_pack16pad"] == len(_input_convs(tr.network)), seen
    else:
        assert seen["_mvd_pack"] > 0, seen


def _load_state_dict(other):
    def fn(tr):
        tr.network.load_state_dict(other)     # torch-visible (version counters): no invalidate_packs() needed
    return fn


def _raw_copy(other):
    def fn(tr):
        for n, p in tr.network.named_parameters():
            p.data.copy_(other[n])            # behind torch's back: the documented case for invalidate_packs()
        tr.optimizer.fp.invalidate_packs()
    return fn


@pytest.mark.parametrize("how", ["load_state_dict", "data_copy_and_invalidate"])
@pytest.mark.parametrize("cls_name,precision", CASES, ids=CASE_IDS)
def test_s1_weights_loaded_after_the_capture_reach_validation_and_the_replays(cls_name, precision, how):
    """S1: capture, replays, then new weights (load_state_dict without invalidate_packs(), or p.data.copy_() with it),
    validation, two replays, validation.  The eager validation right after the load meets stale packs: it must refresh the
    buffers the replay reads, not pack aside of them."""
    t = _Twins(cls_name, precision)
    bs = _batches(t.E, 8)
    for b in bs[:3]:
        t.train(b, "warm")
    assert _graph(t.G) is None and t.G._step_graph["warm"] == 3
    t.train(bs[3], "capture")
    g0 = _graph(t.G)
    assert g0 is not None
    t.train(bs[4], "replay")
    t.train(bs[5], "replay")
    other = _other_state(cls_name, precision)
    _assert_state_differs(t.G, other)
    t.both((_load_state_dict if how == "load_state_dict" else _raw_copy)(other))
    t.log.append(how)
    t.validate(bs[0])
    t.train(bs[6], "replay")
    t.train(bs[7], "replay")
    assert _graph(t.G) is g0, "the sequence must go through the graph captured BEFORE the load"
    t.validate(bs[1])
    t.end()
    _check_packs(t.G, True, precision)
    _check_packs(t.E, False, precision)


@pytest.mark.parametrize("cls_name,precision", CASES, ids=CASE_IDS)
def test_s2_validation_between_warm_up_and_capture_and_across_a_geometry_change(cls_name, precision):
    """S2: an eager forward between the last warm-up step and the capture (and again inside the re-warm after a geometry
    change) leaves every pack cache entry current at capture time: no pack kernel is captured by accident, so whatever the
    replays read must be rewritten by the captured repack."""
    t = _Twins(cls_name, precision)
    bs = _batches(t.E, 12)
    one = [_first_sample(b) for b in bs]
    for b in bs[:3]:
        t.train(b, "warm")
    assert _graph(t.G) is None and t.G._step_graph["warm"] == 3
    t.validate(bs[0], "validate-in-window")
    assert _graph(t.G) is None
    t.train(bs[3], "capture")
    g0 = _graph(t.G)
    assert g0 is not None
    for b in bs[4:7]:
        t.train(b, "replay")
    assert _graph(t.G) is g0
    t.validate(bs[1])
    t.train(one[7], "geometry-change")
    assert _graph(t.G) is None and t.G._step_graph["warm"] == 1, "the old capture must not serve another geometry"
    t.validate(bs[2], "validate-in-rewarm")
    t.train(one[8], "rewarm")
    t.validate(one[0], "validate-in-rewarm")
    t.train(one[9], "rewarm")
    assert _graph(t.G) is None and t.G._step_graph["warm"] == 3
    t.validate(bs[3], "validate-in-window")
    t.train(one[10], "recapture")
    g1 = _graph(t.G)
    assert g1 is not None and g1 is not g0
    t.train(one[11], "replay")
    t.train(one[0], "replay")
    assert _graph(t.G) is g1
    t.validate(one[1])
    t.end()
    _check_packs(t.G, True, precision)
    _check_packs(t.E, False, precision)


@pytest.mark.parametrize("cls_name,precision", CASES, ids=CASE_IDS)
def test_s7_weights_loaded_right_before_an_eager_step_of_a_graph_trainer(cls_name, precision):
    """S7: new weights with NO validation before the next train step, where that step is eager although the trainer is in
    graph mode: between warm-up steps, in the re-warm after a geometry change, and in the eager fallback a failed capture
    leaves behind (use_hip_graph off, the persistent pack buffer still owned).  The packs then live in the persistent
    buffer and are stale while autograd records: refreshing them must not invalidate what earlier layers of the same
    forward saved for their backward (no 'weights were updated between forward and backward'), and the step must equal the
    eager twin's bit for bit."""
    t = _Twins(cls_name, precision)
    bs = _batches(t.E, 12)
    one = [_first_sample(b) for b in bs]
    t.train(bs[0], "warm")
    assert _graph(t.G) is None and t.G._step_graph["warm"] == 1
    other = _other_state(cls_name, precision)
    _assert_state_differs(t.G, other)
    t.both(_load_state_dict(other))
    t.log.append("load_state_dict")
    t.train(bs[1], "warm")
    t.train(bs[2], "warm")
    assert _graph(t.G) is None
    t.train(bs[3], "capture")
    g0 = _graph(t.G)
    assert g0 is not None
    t.train(bs[4], "replay")
    t.train(one[5], "geometry-change")
    assert _graph(t.G) is None and t.G._step_graph["warm"] == 1
    other2 = _other_state(cls_name, precision, seed=11)
    _assert_state_differs(t.G, other2)
    t.both(_raw_copy(other2))
    t.log.append("data_copy_and_invalidate")
    t.train(one[6], "rewarm")
    t.train(one[7], "rewarm")
    assert _graph(t.G) is None and t.G._step_graph["warm"] == 3
    t.train(one[8], "recapture")
    assert _graph(t.G) is not None and _graph(t.G) is not g0
    t.train(one[9], "replay")
    # what a failed capture leaves behind (trainer._graphed_step): eager steps from here on, in-place packs still owned
    t.G.use_hip_graph = False
    assert t.G.optimizer.fp.pack16_inplace
    _assert_state_differs(t.G, other)
    t.both(_load_state_dict(other))
    t.log.append("load_state_dict")
    t.train(one[10], "fallback-eager")
    t.train(bs[11], "fallback-eager")
    t.validate(bs[0])
    t.end()
    _check_packs(t.G, True, precision)
    _check_packs(t.E, False, precision)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_s3_training_alternating_with_validation_while_the_schedule_moves(precision):
    """S3: the epoch pattern -- after the capture six rounds of train / validate, the learning rate changing in the middle."""
    t = _Twins(SINGLE, precision)
    bs = _batches(t.E, 10)
    for b in bs[:3]:
        t.train(b, "warm")
    assert _graph(t.G) is None
    t.train(bs[3], "capture")
    g0 = _graph(t.G)
    assert g0 is not None
    for r in range(6):
        if r == 3:
            t.both(lambda tr: tr.lr_scheduler.step(60))
            t.log.append("lr")
        t.train(bs[4 + r], "replay")
        t.validate(bs[r])
    assert _graph(t.G) is g0
    assert t.E.optimizer.param_groups[0]["lr"] == t.G.optimizer.param_groups[0]["lr"] != t.E.initial_lr
    t.end()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_s4_checkpoint_round_trip_resumes_bit_identically_eager_and_graphed(precision):
    """S4: 7 uninterrupted eager steps against 3 steps + save + load into FRESH trainers (other initial weights) + 4 steps.
    network.load_state_dict() is torch-visible and optimizer.load_state_dict() touches no weight, so no invalidate_packs()
    is due.  The resumed graph trainer crosses warm-up -> capture with _steps > 0: the first-step flag travels through the
    device hyper-parameters."""
    full = _make(SINGLE, precision, False)
    bs = _batches(full, 7)
    want = [np.asarray(full.train_step(b)["loss"]).copy() for b in bs]
    first = _make(SINGLE, precision, False)
    for i, b in enumerate(bs[:3]):
        assert np.array_equal(np.asarray(first.train_step(b)["loss"]), want[i])
    net_sd = {k: v.detach().clone() for k, v in first.network.state_dict().items()}
    opt_sd = first.optimizer.state_dict()
    opt_sd["momentum_buffer"] = opt_sd["momentum_buffer"].clone()
    E2, G2 = _make(SINGLE, precision, False, seed=5), _make(SINGLE, precision, True, seed=5)
    _assert_state_differs(G2, net_sd)
    for tr in (E2, G2):
        tr.network.load_state_dict(net_sd)
        tr.optimizer.load_state_dict(opt_sd)
        assert tr.optimizer._steps == 3
    t = _Twins(SINGLE, precision, E=E2, G=G2)
    for b in bs[3:6]:
        t.train(b, "warm")
    assert _graph(G2) is None and G2._step_graph["warm"] == 3
    t.train(bs[6], "capture")
    assert _graph(G2) is not None
    for i in range(4):
        assert np.array_equal(t.losses[i], want[3 + i]), f"loss of step {4 + i}: resumed {t.losses[i]} uninterrupted {want[3 + i]}"
    t.end(ref=full)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_s5_inference_between_replays_sees_the_trained_weights_and_does_not_disturb_the_graph(precision):
    """S5: deep supervision off + eval() + a no_grad forward between replays, then training goes on through the SAME
    capture.  The graph key holds both flags: under the inference flags the key differs from the captured one, so that
    capture could not be replayed for them."""
    t = _Twins(SINGLE, precision)
    bs = _batches(t.E, 9)
    for b in bs[:3]:
        t.train(b, "warm")
    t.train(bs[3], "capture")
    g0 = _graph(t.G)
    assert g0 is not None
    t.train(bs[4], "replay")
    t.train(bs[5], "replay")
    key0 = t.G._step_graph["key"]
    outs = []
    for tr in (t.E, t.G):
        tr.set_deep_supervision_enabled(False)
        tr.network.eval()
        with torch.no_grad():
            o = tr.network(bs[0]["data"])
        assert torch.is_tensor(o), "deep supervision off: one logits tensor"
        outs.append(o.float().clone())
    assert torch.equal(outs[0], outs[1]), "inference logits between replays: eager vs graph trainer"
    assert t.G._graph_key(bs[0]["data"], bs[0]["target"]) != key0, "train-mode capture would serve the inference flags"
    assert _graph(t.G) is g0
    for tr in (t.E, t.G):
        tr.network.train()
        tr.set_deep_supervision_enabled(True)
    assert t.G._graph_key(bs[0]["data"], bs[0]["target"]) == key0
    for b in bs[6:9]:
        t.train(b, "replay")
    assert _graph(t.G) is g0 and t.G._step_graph["key"] == key0
    t.end()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_s6_device_losses_collected_over_an_epoch_are_one_value_per_step(precision):
    """S6: train_step(return_device_loss=True) collected without reading: the list equals the eager one element by
    element (the graph's loss is ONE static tensor; handing it out would give N aliases of the last value)."""
    E, G = _make(SINGLE, precision, False), _make(SINGLE, precision, True)
    bs = _batches(E, 6)
    le = [E.train_step(b, return_device_loss=True)["loss"] for b in bs]
    lg = [G.train_step(b, return_device_loss=True)["loss"] for b in bs]
    assert _graph(G) is not None
    torch.cuda.synchronize()
    assert lg[-1].data_ptr() != lg[-2].data_ptr()
    assert len({x.data_ptr() for x in lg}) == len(lg)
    for i, (a, b) in enumerate(zip(le, lg)):
        assert a.is_cuda and b.is_cuda and torch.equal(a, b), f"device loss of step {i}: eager {float(a)} graph {float(b)}"
    assert len({float(x) for x in lg}) > 1


def test_s6_last_topology_of_a_replayed_step_is_overwritten_by_the_next_step_and_survives_a_validation():
    """ContrastiveTrainerMI355.last_topology in graph mode is documented as the graph's static tensors, OVERWRITTEN by the
    next train step (clone what has to outlive it).  Asserted here: after every replay it holds that step's counts (equal
    to the eager trainer's, whose tensors are fresh per step), at the same addresses; a clone taken before the next step
    keeps the earlier counts; and a validation_step in between -- an eager forward that re-points the attribute at its own
    tensors -- does not detach it from the graph for the train steps that follow."""
    t = _Twins(DUAL, "bf16")
    bs = _batches(t.E, 7)
    keys = ("cc_pred", "cc_true", "betti0_error")

    def same():
        for k in keys:
            assert torch.equal(t.E.last_topology[k], t.G.last_topology[k]), (k, t.log)

    for b in bs[:4]:
        t.train(b)
        same()
    assert _graph(t.G) is not None
    t.train(bs[4], "replay")
    same()
    kept = {k: v.clone() for k, v in t.G.last_topology.items()}
    kept_e = {k: v for k, v in t.E.last_topology.items()}
    ptrs = {k: v.data_ptr() for k, v in t.G.last_topology.items()}
    t.train(bs[5], "replay")
    same()
    assert {k: v.data_ptr() for k, v in t.G.last_topology.items()} == ptrs, "static tensors: overwritten in place"
    for k in keys:
        assert torch.equal(kept[k], kept_e[k])
    t.validate(bs[0])
    same()
    t.train(bs[6], "replay")
    same()
    assert {k: v.data_ptr() for k, v in t.G.last_topology.items()} == ptrs
    t.end()
