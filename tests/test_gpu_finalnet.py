"""MI355FinalNetv2 and FinalNetTrainerMI355 on a tiny plan: 2 input channels, patch 8 x 16 x 16, features 8/16/32/64, so
N = 16 bottleneck tokens of C = 64 features (8 heads of 8).

The whole-network comparison uses the bar of the project's other whole-network test (tests/test_gpu_parity.py: 1e-4
max(1, max|ref|) per tensor): its error is the conv stack's; the fusion block alone is held to the tighter bar of
tests/test_gpu_attention.py.
"""
import numpy as np
import pytest
import torch
from torch import nn

import attention_ref as R
from multimodal_mvd_seg_amd import network, ops, trainer
from oracle import unet_oracle as UO

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PATCH, STRIDES = (8, 16, 16), [(1, 1, 1), (1, 2, 2), (1, 2, 2), (2, 2, 2)]
FEATURES, BOTTLENECK = [8, 16, 32, 64], (4, 2, 2)
DJ = {"channel_names": {"0": "a", "1": "b"}, "labels": {"background": 0, "organ": 1, "vessel": 2}}
K = 3


class FinalNetTrainerAdamW(trainer.FinalNetTrainerMI355):
    configure_optimizers = trainer.nnUNetTrainerAdamMI355.configure_optimizers


def _plans():
    plans = trainer.make_plans(PATCH, STRIDES, batch_size=2, base_features=8, max_features=64)
    plans['configurations']['3d_fullres']['spacing'] = [1.0, 1.0, 1.0]   # (read by the segmentation export)
    return plans


def _net(seed=0, ds=True):
    torch.manual_seed(seed)
    pm = trainer.PlansManager(_plans())
    return network.get_finalnet_from_plans(pm, DJ, pm.get_configuration("3d_fullres"), 2, ds)


def _make(graph, seed=0, cls=trainer.FinalNetTrainerMI355):
    tr = cls(_plans(), "3d_fullres", 0, DJ, device=DEV)
    tr.use_hip_graph = graph
    torch.manual_seed(seed)
    tr.initialize()
    return tr


def _no_dropout(net):
    for m in net.modules():
        if isinstance(m, nn.Dropout):
            m.p = 0.0


def _perturb_fusion(net, seed=5):
    """pos_embed starts at 0, LayerNorm at (1, 0): move every used fusion parameter so that each gradient path is live"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in net.fusion_parameters():
            p.add_(torch.randn(p.shape, generator=g).to(p.device) * 0.1)


# ------------------------------------------------------------------------------------------------ against fp64
def _restatement(sd, dtype):
    """The whole network in torch on the CPU: the oracle's plain encoder / decoder (oracle/unet_oracle.py) around
    attention_ref.fusion_block; UNetDecoder6.forward is the plain decoder with y in the place of skips[-1]."""
    parts = []
    for i in (1, 2):
        enc = UO.PlainConvEncoder(1, 4, FEATURES, [[3, 3, 3]] * 4, STRIDES, 2)
        dec = UO.UNetDecoder(enc, K, 2, True)
        enc.load_state_dict({k[len(f"encoder{i}."):]: v for k, v in sd.items() if k.startswith(f"encoder{i}.")})
        own = set(dec.state_dict())
        dec.load_state_dict({k[len(f"decoder{i}."):]: v for k, v in sd.items()
                             if k.startswith(f"decoder{i}.") and k[len(f"decoder{i}."):] in own})
        parts.append((enc.to(dtype), dec.to(dtype)))
    P = {k: sd[k].to(dtype).requires_grad_(True) for k in R.FUSION_KEYS}

    def forward(x):
        (e1, d1), (e2, d2) = parts
        s1, s2 = e1(x[:, 0:1]), e2(x[:, 1:2])
        B, C = s1[-1].shape[:2]
        tok = lambda t: t.reshape(B, C, -1).permute(0, 2, 1)
        y1, y2 = R.fusion_block(tok(s1[-1]), tok(s2[-1]), P)
        back = lambda y: y.permute(0, 2, 1).reshape(s1[-1].shape)
        return d1(s1[:-1] + [back(y1)], True), d2(s2[:-1] + [back(y2)], True)

    def named():
        out = dict(P)
        for i, (e, d) in enumerate(parts, 1):
            out.update({f"encoder{i}.{n}": p for n, p in e.named_parameters()})
            out.update({f"decoder{i}.{n}": p for n, p in d.named_parameters() if not n.startswith("encoder.")})
        return out
    return forward, named


def test_forward_and_parameter_gradients_against_fp64():
    net = _net()
    _perturb_fusion(net)
    _no_dropout(net)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 2, *PATCH, generator=g)
    fwd, named = _restatement(sd, torch.float64)
    (o1, f1), (o2, f2) = fwd(x.double())
    ws = [torch.randn(o.shape, generator=g) for o in list(o1) + list(o2)]
    loss = sum((o * w.double()).sum() for o, w in zip(list(o1) + list(o2), ws))
    loss.backward()
    ref = {"logits": [o.detach() for o in list(o1) + list(o2)], "feat": [f1.detach(), f2.detach()],
           "grads": {n: p.grad for n, p in named().items()}}
    net.to(DEV).train()
    o1, o2, f1, f2 = net(x.to(DEV))
    assert isinstance(o1, list) and len(o1) == 3 and len(o2) == 3
    loss = sum((o * w.to(DEV)).sum() for o, w in zip(list(o1) + list(o2), ws))
    loss.backward()

    def close(what, got, want):
        want = want.double()
        tol = 1e-4 * max(1.0, float(want.abs().max()))
        err = float((got.detach().cpu().double() - want).abs().max())
        print(f"{what}: err {err:.3e} tol {tol:.3e} max|ref| {float(want.abs().max()):.3e}")
        assert err <= tol, f"{what}: {err:.3e} > {tol:.3e}"
    for i, (o, r) in enumerate(zip(list(o1) + list(o2), ref["logits"])):
        close(f"logits{i}", o, r)
    close("feat1", f1, ref["feat"][0])
    close("feat2", f2, ref["feat"][1])
    params = dict(net.named_parameters())
    unused = set(net.unused_parameter_names())
    checked = 0
    for n, gr in ref["grads"].items():
        assert n in params and n not in unused, n
        assert gr is not None, f"the restatement does not use {n}"
        close("grad " + n, params[n].grad, gr)
        checked += 1
    assert checked == len(params) - len(unused)
    for n in unused:
        assert params[n].grad is None, n


def test_inference_output_is_the_mean_of_the_two_branches():
    net = _net(ds=True).to(DEV).eval()
    _perturb_fusion(net)
    x = torch.randn(1, 2, *PATCH, generator=torch.Generator().manual_seed(4)).to(DEV)
    with torch.no_grad():
        o1, o2, _, _ = net(x)
        net.do_ds = False
        assert net.decoder1.deep_supervision is False and net.decoder2.deep_supervision is False
        avg = net(x)
    assert torch.is_tensor(avg) and avg.shape == (1, K, *PATCH)
    assert torch.equal(avg, (o1[0] + o2[0]) / 2)
    assert int(net.mvd_dropout_state[1]) == 0, "eval forwards must not advance t"


# ------------------------------------------------------------------------------------------------ state_dict
def _reference_keys():
    """Key -> shape, written out from the reference's constructors (selfattnNet.py:883-907, UNetDecoder.py:830-868,
    :1094-1099, :1136-1139, PlainConvEncoder / StackedConvBlocks / ConvDropoutNormReLU of dynamic_network_architectures) for
    this plan, with N in the place of the hard-coded 128."""
    N, C = 16, 64
    keys = {}

    def block(prefix, cin, cout):   # ConvDropoutNormReLU registers conv / norm and the same modules again in all_modules
        for conv, norm in (("conv", "norm"), ("all_modules.0", "all_modules.1")):
            keys[f"{prefix}.{conv}.weight"], keys[f"{prefix}.{conv}.bias"] = (cout, cin, 3, 3, 3), (cout,)
            keys[f"{prefix}.{norm}.weight"], keys[f"{prefix}.{norm}.bias"] = (cout,), (cout,)

    def encoder(prefix):
        cin = 1
        for s, f in enumerate(FEATURES):
            block(f"{prefix}.stages.{s}.0.convs.0", cin, f)
            block(f"{prefix}.stages.{s}.0.convs.1", f, f)
            cin = f

    def attention(prefix, cross):
        if cross:
            for m in ("qkv1", "qkv2"):
                keys[f"{prefix}.{m}.weight"] = (3 * C, C)
            for m in ("proj1", "proj2"):
                keys[f"{prefix}.{m}.weight"], keys[f"{prefix}.{m}.bias"] = (C, C), (C,)
        else:
            keys[f"{prefix}.qkv.weight"] = (3 * C, C)
            keys[f"{prefix}.proj.weight"], keys[f"{prefix}.proj.bias"] = (C, C), (C,)

    def layernorm(prefix):
        keys[f"{prefix}.weight"], keys[f"{prefix}.bias"] = (C,), (C,)
    for i in (1, 2):
        encoder(f"encoder{i}")
        d = f"decoder{i}"
        encoder(f"{d}.encoder")   # the decoder keeps its encoder as a submodule (UNetDecoder.py:821)
        for s in range(3):
            below, skip, st = FEATURES[-(s + 1)], FEATURES[-(s + 2)], STRIDES[-(s + 1)]
            keys[f"{d}.transpconvs.{s}.weight"], keys[f"{d}.transpconvs.{s}.bias"] = (below, skip, *st), (skip,)
            block(f"{d}.stages.{s}.convs.0", 2 * skip, skip)
            block(f"{d}.stages.{s}.convs.1", skip, skip)
            keys[f"{d}.seg_layers.{s}.weight"], keys[f"{d}.seg_layers.{s}.bias"] = (K, skip, 1, 1, 1), (K,)
        for j in (1, 2, 3):
            keys[f"{d}.pos_embed{j}"] = (1, N, C)
        attention(f"{d}.crossattn", True)
        attention(f"{d}.selfattn", False)
        layernorm(f"{d}.norm1")
        layernorm(f"{d}.norm2")
    for j in (1, 2, 3, 4):
        keys[f"pos_embed{j}"] = (1, N, C)
        layernorm(f"norm{j}")
    attention("crossattn", True)
    attention("selfattn1", False)
    attention("selfattn2", False)
    return keys


def test_state_dict_keys_shapes_and_round_trip():
    net = _net(seed=1)
    sd = net.state_dict()
    want = _reference_keys()
    want["mvd_dropout_state"] = (2,)   # the one key the reference does not have: {seed, t} of the dropout generator
    assert set(sd) == set(want), sorted(set(sd) ^ set(want))
    for k, shp in want.items():
        assert tuple(sd[k].shape) == tuple(shp), (k, tuple(sd[k].shape), shp)
    other = _net(seed=2)
    assert int(other.mvd_dropout_state[0]) != int(net.mvd_dropout_state[0]), "the seed comes from torch's CPU generator"
    assert int(_net(seed=1).mvd_dropout_state[0]) == int(net.mvd_dropout_state[0])
    res = other.load_state_dict(sd)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in other.state_dict().items():
        assert torch.equal(v, sd[k]), k
    # a checkpoint of the reference has no dropout state: it loads, and the module keeps its own
    ref_sd = {k: v for k, v in sd.items() if k != "mvd_dropout_state"}
    third = _net(seed=3)
    own = third.mvd_dropout_state.clone()
    third.load_state_dict(ref_sd)
    assert torch.equal(third.mvd_dropout_state, own)


# ------------------------------------------------------------------------------------------------ trainer
@pytest.mark.parametrize("cls", [trainer.FinalNetTrainerMI355, FinalNetTrainerAdamW], ids=["sgd", "adamw"])
def test_unused_parameters_never_move_and_used_fusion_parameters_do(cls):
    tr = _make(False, cls=cls)
    net = tr.network
    unused = net.unused_parameter_names()
    params = dict(net.named_parameters())
    before = {n: p.detach().clone() for n, p in params.items()}
    flat = tr.optimizer.fp.flat
    lo, hi = flat.data_ptr(), flat.data_ptr() + flat.numel() * 4
    for n in unused:
        assert not (lo <= params[n].data_ptr() < hi), f"{n} lies inside the flat buffer"
    used_fusion = {id(p) for p in net.fusion_parameters()}
    assert all(lo <= p.data_ptr() < hi for p in net.fusion_parameters())
    assert {id(p) for p in tr.optimizer.fp.params} == {id(p) for n, p in params.items() if n not in unused}
    for i in range(3):
        tr.train_step(tr.make_dummy_batch(seed=100 + i))
    torch.cuda.synchronize()
    for n in unused:
        assert torch.equal(params[n].detach(), before[n]), f"{n} moved"
    for n, p in params.items():
        if id(p) in used_fusion:
            assert not torch.equal(p.detach(), before[n]), f"{n} did not move in 3 steps"
    assert int(net.mvd_dropout_state[1]) == 3


def test_three_graphed_steps_equal_three_eager_steps_with_dropout_on():
    """Two trainers with the same seed: E always eager, G eager for its warm-up steps, then one capture and three replays."""
    E, G = _make(False), _make(True)
    assert torch.equal(E.network.mvd_dropout_state, G.network.mvd_dropout_state)
    assert E.network.crossattn.attn_drop1.p == 0.1 and E.network.training
    for (n, p), (_, q) in zip(E.network.named_parameters(), G.network.named_parameters()):
        assert torch.equal(p.detach(), q.detach()), n
    steps = G.hip_graph_warmup + 1 + 3
    seed = int(E.network.mvd_dropout_state[0])
    replays = 0
    for i in range(steps):
        b = E.make_dummy_batch(seed=200 + i)
        had_graph = G._step_graph is not None and G._step_graph["graph"] is not None
        a, c = E.train_step(b)["loss"], G.train_step(b)["loss"]
        replays += int(had_graph)
        assert np.array_equal(np.asarray(a), np.asarray(c)), f"loss of step {i + 1}: eager {a} graph {c}"
        # the device step counter moved by one per step, replayed or not: every replay draws fresh masks
        assert E.network.mvd_dropout_state.cpu().tolist() == G.network.mvd_dropout_state.cpu().tolist() == [seed, i + 1]
    assert replays == 3 and E._step_graph is None and G.use_hip_graph, "the capture fell back to the eager step"
    torch.cuda.synchronize()
    for (n, p), (_, q) in zip(E.network.named_parameters(), G.network.named_parameters()):
        assert torch.equal(p.detach(), q.detach()), f"parameter {n} after {steps} steps"
    assert torch.equal(E.optimizer.momentum_buffer, G.optimizer.momentum_buffer)
    # the masks of consecutive steps differ
    n = 2 * 8 * 16 * 16
    m = [ops.dropout_mask(seed, t, 0, 0.1, n, DEV).cpu().numpy() for t in (steps - 2, steps - 1, steps)]
    assert not np.array_equal(m[0], m[1]) and not np.array_equal(m[1], m[2])


def _case(seed):
    g = torch.Generator().manual_seed(seed)
    shape = (12, 24, 20)
    return {"data": torch.randn(2, *shape, generator=g),
            "seg": torch.randint(0, K, shape, generator=g).numpy().astype(np.uint8)[None],
            "properties": {"shape_before_cropping": shape, "bbox_used_for_cropping": [[0, s] for s in shape],
                           "shape_after_cropping_and_before_resampling": shape, "spacing": [1.0, 1.0, 1.0]}}


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_validation_leaves_the_following_train_steps_bit_identical(graph):
    """The recipe of tests/test_gpu_graph_sequences.py: V validates between its train steps, P never does; both end with
    the same parameters.  Eval forwards draw nothing and do not advance t."""
    V, P = _make(graph), _make(graph)
    bs = [V.make_dummy_batch(seed=300 + i) for i in range(5)]
    for b in bs[:2]:
        V.train_step(b)
        P.train_step(b)
    t0 = int(V.network.mvd_dropout_state[1])
    out = V.validation_step(bs[0])
    assert set(out) == {"loss", "tp_hard", "fp_hard", "fn_hard"} and np.isfinite(out["loss"]).all()
    metrics = V.perform_actual_validation([_case(1), _case(2)])
    assert len(metrics["metric_per_case"]) == 2
    assert int(V.network.mvd_dropout_state[1]) == t0 and V.network.training and V.network.do_ds
    for b in bs[2:]:
        a, c = V.train_step(b)["loss"], P.train_step(b)["loss"]
        assert np.array_equal(np.asarray(a), np.asarray(c))
    torch.cuda.synchronize()
    for (n, p), (_, q) in zip(V.network.named_parameters(), P.network.named_parameters()):
        assert torch.equal(p.detach(), q.detach()), f"parameter {n}"
    assert V.network.mvd_dropout_state.cpu().tolist() == P.network.mvd_dropout_state.cpu().tolist()
