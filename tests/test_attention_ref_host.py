"""Host-side checks of the FinalNetv2 work: the fp64 restatement (tests/attention_ref.py) against the fixture the reference's
own Cross_Attention / Self_Attention wrote, the dropout generator's host form against numpy.random.Philox, and the
refusals, which are raised at construction and so need no GPU."""
import os

import numpy as np
import pytest
import torch
from torch import nn

import attention_ref as R
from multimodal_mvd_seg_amd import network, trainer

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cross_attention.npz")


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLD, allow_pickle=False)
    return {k: (torch.from_numpy(z[k]) if z[k].dtype == np.float64 else z[k]) for k in z.files}


def test_restatement_reproduces_the_reference_cross_attention(gold):
    assert gold["x1"].shape == (2, 16, 32) and int(gold["heads"]) == 8 and str(gold["source"]).startswith("reference")
    o1, o2 = R.cross_attention(gold["x1"], gold["x2"], gold["ca/qkv1.weight"], gold["ca/qkv2.weight"],
                               gold["ca/proj1.weight"], gold["ca/proj1.bias"], gold["ca/proj2.weight"],
                               gold["ca/proj2.bias"], int(gold["heads"]))
    assert float((o1 - gold["ca_out1"]).abs().max()) <= 1e-12
    assert float((o2 - gold["ca_out2"]).abs().max()) <= 1e-12
    # which stream queries which: swapping the inputs does not give the swapped outputs
    s1, _ = R.cross_attention(gold["x2"], gold["x1"], gold["ca/qkv1.weight"], gold["ca/qkv2.weight"],
                              gold["ca/proj1.weight"], gold["ca/proj1.bias"], gold["ca/proj2.weight"],
                              gold["ca/proj2.bias"], int(gold["heads"]))
    assert float((s1 - gold["ca_out2"]).abs().max()) > 1e-3


def test_restatement_reproduces_the_reference_self_attention_and_its_quirk(gold):
    so = R.self_attention(gold["x1"], gold["sa/qkv.weight"], int(gold["heads"]))
    assert float((so - gold["sa_out"]).abs().max()) <= 1e-12
    # the fixture's second run had another proj: the reference's output did not move, so proj is not part of the function
    assert not np.array_equal(gold["sa/proj.weight"].numpy(), gold["sa/proj2.weight"].numpy())
    assert torch.equal(gold["sa_out"], gold["sa_out_other_proj"])


def test_fusion_block_restatement_is_built_from_the_pinned_helpers(gold):
    """With pos = 0, norm = identity-affine the block is cross_attention / self_attention of layer-normed tokens."""
    C, N, H = 32, 16, int(gold["heads"])
    P = {"pos_embed1": torch.zeros(1, N, C, dtype=torch.float64), "pos_embed2": torch.zeros(1, N, C, dtype=torch.float64)}
    for i in range(1, 5):
        P[f"norm{i}.weight"], P[f"norm{i}.bias"] = torch.ones(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    for k in ("qkv1.weight", "qkv2.weight", "proj1.weight", "proj1.bias", "proj2.weight", "proj2.bias"):
        P["crossattn." + k] = gold["ca/" + k]
    P["selfattn1.qkv.weight"] = P["selfattn2.qkv.weight"] = gold["sa/qkv.weight"]
    x1, x2 = gold["x1"], gold["x2"]
    y1, y2 = R.fusion_block(x1, x2, P, H)
    ln = lambda t: torch.nn.functional.layer_norm(t, (C,), eps=1e-5)
    a1, a2 = R.cross_attention(ln(x2), ln(x1), *[gold["ca/" + k] for k in ("qkv1.weight", "qkv2.weight", "proj1.weight",
                                                                            "proj1.bias", "proj2.weight", "proj2.bias")], H)
    e1 = x1 + R.self_attention(ln(a1 + x2), gold["sa/qkv.weight"], H)
    e2 = x2 + R.self_attention(ln(a2 + x1), gold["sa/qkv.weight"], H)
    assert float((y1 - e1).abs().max()) <= 1e-12 and float((y2 - e2).abs().max()) <= 1e-12


def test_mask_generator_matches_numpy_philox():
    seed, t, site, n = 0x0123_4567_89AB_CDEF, 41, 3, 1003
    ref = np.random.Philox(key=[seed, site], counter=[0, t, 0, 0]).random_raw(n)
    assert np.array_equal(R.dropout_words(seed, t, site, n), ref)
    u = (ref >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)
    assert np.array_equal(R.dropout_mask(seed, t, site, 0.1, n), (u >= np.float32(0.1)).astype(np.uint8))
    assert R.dropout_mask(seed, t, site, 0.0, n).all()


# ------------------------------------------------------------------------------------------------ refusals
DJ = {'channel_names': {'0': 'a', '1': 'b'}, 'labels': {'background': 0, 'organ': 1, 'vessel': 2}}
STRIDES = [(1, 1, 1), (1, 2, 2), (1, 2, 2), (2, 2, 2)]


def _build(patch=(8, 16, 16), strides=STRIDES, base=8, max_features=64, channels=2, configuration='3d_fullres'):
    plans = trainer.make_plans(patch, strides, base_features=base, max_features=max_features, configuration=configuration)
    pm = trainer.PlansManager(plans)
    return network.get_finalnet_from_plans(pm, DJ, pm.get_configuration(configuration), channels, True)


def test_tiny_plan_builds_on_the_host():
    net = _build()
    assert (net.num_tokens, net.hidden_size) == (16, 64)
    assert _build((32, 64, 64), [(1, 1, 1)] + [(2, 2, 2)] * 2 + [(1, 2, 2)] * 2, base=4, max_features=32).num_tokens == 128


@pytest.mark.parametrize("channels", [1, 3, 4])
def test_refuses_other_input_channel_counts(channels):
    with pytest.raises(NotImplementedError, match="exactly 2 input channels"):
        _build(channels=channels)


def test_refuses_feature_counts_the_heads_do_not_divide():
    with pytest.raises(NotImplementedError, match=r"C % 8 != 0"):
        _build(base=8, max_features=60)


@pytest.mark.parametrize("features,dh", [(16, 2), (48, 6), (640, 80)])
def test_refuses_head_dimensions_outside_the_kernel(features, dh):
    with pytest.raises(NotImplementedError, match=f"head dimension {dh}"):
        network.BottleneckFusion(features, 16)


def test_refuses_more_tokens_than_the_kernel_holds():
    with pytest.raises(NotImplementedError, match="at most 256"):
        _build(patch=(32, 64, 64))   # 16 * 8 * 8 = 1024 tokens


def test_refuses_2d_plans():
    with pytest.raises(NotImplementedError, match="2-D plans"):
        _build(patch=(16, 16), strides=[(1, 1), (2, 2), (2, 2), (2, 2)], configuration='2d')
    with pytest.raises(NotImplementedError, match="2-D plans"):
        network.MI355FinalNetv2(True, nn.InstanceNorm2d, None, None, None, nn.LeakyReLU, None, [8, 16, 32, 64], 3,
                                [1, 2, 2, 2], 2, 2, n_stages=4, conv_op=nn.Conv2d, num_tokens=16)


def test_refuses_bf16():
    net = _build()
    with pytest.raises(NotImplementedError, match="fp32 only"):
        network.set_precision(net, 'bf16')
    assert network.set_precision(net, 'fp32') is net


def test_unused_members_are_frozen_and_outside_the_execution_order():
    net = _build()
    unused = set(net.unused_parameter_names())
    expect = {f"selfattn{i}.proj.{w}" for i in (1, 2) for w in ("weight", "bias")} | {"pos_embed3", "pos_embed4"}
    for d in ("decoder1", "decoder2"):
        expect |= {f"{d}.pos_embed{i}" for i in (1, 2, 3)} | {f"{d}.norm{i}.{w}" for i in (1, 2) for w in ("weight", "bias")}
        expect |= {f"{d}.crossattn.{m}.weight" for m in ("qkv1", "qkv2", "proj1", "proj2")}
        expect |= {f"{d}.crossattn.{m}.bias" for m in ("proj1", "proj2")}
        expect |= {f"{d}.selfattn.qkv.weight", f"{d}.selfattn.proj.weight", f"{d}.selfattn.proj.bias"}
    assert unused == expect
    order = net.parameters_in_execution_order()
    ids = {id(p) for p in order}
    by_name = dict(net.named_parameters())
    assert len(ids) == len(order) and all(id(by_name[n]) not in ids for n in unused)
    assert ids == {id(p) for n, p in by_name.items() if n not in unused}
    # encoder1, encoder2, fusion, decoder1, decoder2
    name_of = {id(p): n for n, p in by_name.items()}
    groups = [name_of[id(p)].split(".")[0] for p in order]
    firsts = [g for i, g in enumerate(groups) if i == 0 or groups[i - 1] != g]
    assert firsts[:2] == ["encoder1", "encoder2"] and firsts[-2:] == ["decoder1", "decoder2"]
    assert firsts[2:4] == ["pos_embed1", "pos_embed2"] and "selfattn2" == firsts[-3]
