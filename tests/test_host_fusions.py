"""CPU tests of the fusion functions on the fused engines: the float64 restatement (tests/fusion_ref.py) against the fixture
written from the reference's modules/fusion.py (tests/golden/fusions.npz), the engine's parameter layout against the task
modules' state_dict for every fusion, and the refusals."""
import os

import numpy as np
import pytest
import torch

import fusion_ref as R
import gen_util as G
from m2_mixer_amd import engine as E
from m2_mixer_amd import models as MD

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fusions.npz")


def test_restatement_matches_the_reference_fixture():
    z = np.load(GOLDEN)
    a, b, dy = (torch.from_numpy(z[k]).requires_grad_(True) for k in ("a", "b", "dy"))
    for name in ("SumFusion", "MeanFusion", "MaxFusion"):
        a.grad = b.grad = None
        y = R.fuse(name, a, b)
        y.backward(dy)
        assert np.array_equal(y.detach().numpy(), z[f"{name}.y"]), name
        assert np.array_equal(a.grad.numpy(), z[f"{name}.da"]) and np.array_equal(b.grad.numpy(), z[f"{name}.db"]), name
    a.grad = b.grad = None
    p = {k[len("gate."):]: torch.from_numpy(z[k]).requires_grad_(True) for k in z.files if k.startswith("gate.fusion_function.")}
    y = R.gate(a, b, p)
    y.backward(dy)
    assert np.allclose(y.detach().numpy(), z["gate.y"], rtol=0, atol=1e-12)
    assert np.allclose(a.grad.numpy(), z["gate.da"], rtol=0, atol=1e-12)
    assert np.allclose(b.grad.numpy(), z["gate.db"], rtol=0, atol=1e-12)
    for k, v in p.items():
        assert np.allclose(v.grad.numpy(), z[f"grad.{k}"], rtol=0, atol=1e-12), k


def _module_cfg(task, c):
    a, b = ("image", "audio") if task == "avmnist" else ("image", "text")
    mods = {a: dict(c[a], block_type="MLPMixer"), b: dict(c[b], block_type="MLPMixer")}
    mods["multimodal"] = dict(c["multimodal"], block_type="FusionMixer")
    mods["classification"] = dict(classifier="StandardClassifier", num_classes=c["num_classes"],
                                  input_shape=[16, 49, c["multimodal"]["hidden_dim"]])
    cfg = {"dropout": c["dropout"], "modalities": mods}
    if task == "mmimdb":
        cfg["pos_weight"] = c["pos_weight"]
    return cfg


SHAPES = [("avmnist", "S"), ("avmnist", "M"), ("avmnist", "B"), ("avmnist", "gated_4loss"), ("mmimdb", "mmimdb")]


@pytest.mark.parametrize("fusion", R.FUSIONS)
@pytest.mark.parametrize("task,shapes", SHAPES)
def test_engine_param_shapes_match_the_module(task, shapes, fusion):
    base = {"S": G.AVMNIST["S"], "M": G.AVMNIST["M"], "B": G.AVMNIST["B"], "gated_4loss": R.GATED_4LOSS, "mmimdb": G.MMIMDB}[shapes]
    c = R.with_fusion(base, fusion)
    cls = MD.AVMnistMixerMultiLoss if task == "avmnist" else MD.MMIMDBMixerMultiLoss
    net = cls(_module_cfg(task, c), {"lr": 1e-3})
    sd = [(k, tuple(v.shape)) for k, v in net.state_dict().items() if not k.endswith("criterion.pos_weight")]
    mods = ("image", "audio") if task == "avmnist" else ("image", "text")
    eng = list(E.two_tower_param_shapes(net._engine_cfg(), mods).items())
    assert eng == sd
    assert eng == list(R.two_tower_shapes(task, c).items())
    if fusion == "BiModalGatedUnit":
        keys = [k for k, _ in eng]
        i = keys.index("fusion_function.mod1_hidden.weight")
        assert keys[i:i + 6] == [f"fusion_function.{m}.{t}" for m in R.GATE_KEYS for t in ("weight", "bias")]
        assert keys[i + 6].startswith("fusion_mixer.") and keys[i - 1].startswith(mods[1] + "_mixer.")


def test_missing_fusion_function_is_concat():
    c = G.AVMNIST["B"]
    assert "fusion_function" not in c["multimodal"]
    assert list(E.two_tower_param_shapes(c, ("image", "audio")).items()) == list(G.avmnist_shapes(c).items())
    assert E.fusion_tokens(c["multimodal"], 4, 4) == 8
    assert E.fusion_tokens(dict(c["multimodal"], fusion_function="ConcatFusion"), 4, 49) == 53


@pytest.mark.parametrize("name", ["ConcatDynaFusion", "ExtraConcatFusion", "MultiModalGatedUnit"])
def test_unbuilt_fusions_are_refused(name):
    c = R.with_fusion(G.AVMNIST["S"], "SumFusion")
    c["multimodal"]["fusion_function"] = name
    with pytest.raises(RuntimeError, match="fusion_function"):
        E.two_tower_param_shapes(c, ("image", "audio"))


@pytest.mark.parametrize("fusion", ["SumFusion", "MeanFusion", "MaxFusion"])
def test_unequal_token_counts_are_refused_as_the_reference_does(fusion):
    with pytest.raises(ValueError, match="Input shapes must be equal"):
        E.fusion_tokens({"fusion_function": fusion}, 4, 49)


def test_gate_with_unequal_token_counts_is_refused():
    with pytest.raises(RuntimeError, match="fusion_function"):
        E.fusion_tokens({"fusion_function": "BiModalGatedUnit"}, 4, 49)


def test_gate_sizes_other_than_the_hidden_dim_are_refused():
    """The engine needs the gate's out_size to be the towers' hidden_dim (one D for the heads): refused before any GPU work."""
    c = R.with_fusion(G.AVMNIST["S"], "BiModalGatedUnit")
    c["multimodal"]["out_size"] = 64
    eng = object.__new__(E.AVMnistEngine)
    eng.cfg = c
    with pytest.raises(RuntimeError, match="out_size"):
        E._TwoTowerEngine._build(eng)
