"""CPU-side checks of the evidential (EDL) model: tests/edl_ref.py against the reference's own EDLMSELoss (tests/golden/edl.npz,
written by tests/golden/make_golden_edl.py) and against its closed-form gradient, the gate form, the case table's seeds, and the
plumbing of the entry point (header, binding, library), the module and the engine's refusal."""
import os
import re

import numpy as np
import pytest
import torch

import edl_ref as E
import leaf_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "edl.npz"))
FIXTURE_CASES = ((1, 2), (5, 10), (9, 32))
EPOCHS = (0, 3, 50)


def _fixture(B, K):
    tag = f"B{B}K{K}"
    return tag, torch.from_numpy(GOLD[f"{tag}.logits"]), torch.from_numpy(GOLD[f"{tag}.labels"])


@pytest.mark.parametrize("B,K", FIXTURE_CASES)
def test_edl_ref_reproduces_the_reference_loss_and_gradient(B, K):
    """Value and d loss / d logits of the reference's EDLMSELoss: 1e-6 in float32, 1e-12 in float64, at every stored epoch."""
    tag, logits, labels = _fixture(B, K)
    assert logits.dtype == torch.float64 and tuple(logits.shape) == (B, K)
    for dtype, name, tol in ((torch.float32, "f32", 1e-6), (torch.float64, "f64", 1e-12)):
        z = logits.to(dtype).clone().requires_grad_(True)
        loss = E.edl_loss(z, labels)
        loss.backward()
        for epoch in EPOCHS:
            want_l, want_g = GOLD[f"{tag}.e{epoch}.{name}.loss"], GOLD[f"{tag}.e{epoch}.{name}.dlogits"]
            assert abs(float(loss.detach()) - float(want_l)) < tol, (name, epoch)
            assert float((z.grad.double() - torch.from_numpy(want_g).double()).abs().max()) < tol, (name, epoch)


@pytest.mark.parametrize("B,K", FIXTURE_CASES)
def test_the_epoch_has_no_effect_in_the_reference(B, K):
    """The KL term is times annealing_coef * 0 (modules/losses.py:20): the stored results of epochs 0, 3 and 50 are bit-equal."""
    tag = f"B{B}K{K}"
    for name in ("f32", "f64"):
        for what in ("loss", "dlogits"):
            first = GOLD[f"{tag}.e{EPOCHS[0]}.{name}.{what}"]
            for epoch in EPOCHS[1:]:
                assert np.array_equal(first, GOLD[f"{tag}.e{epoch}.{name}.{what}"]), (name, what, epoch)


@pytest.mark.parametrize("B,K", FIXTURE_CASES + ((81, 23),))
def test_gate_form_equals_relu_form_under_relus_own_gate_and_the_closed_form_gradient_equals_autograd(B, K):
    gen = torch.Generator().manual_seed(7 * B + K)
    z0 = 2.0 * torch.randn(B, K, generator=gen, dtype=torch.float64)
    z0[0, 0] = 0.0
    labels = torch.randint(0, K, (B,), generator=gen)
    grads = []
    for gate in (None, z0 > 0):
        z = z0.clone().requires_grad_(True)
        loss = E.edl_loss(z, labels, gate)
        loss.backward()
        grads.append((float(loss.detach()), z.grad.clone()))
        assert float((E.edl_grad(z0, labels, gate) - z.grad).abs().max()) < 1e-15
    assert grads[0][0] == grads[1][0] and torch.equal(grads[0][1], grads[1][1])
    assert torch.equal(E.uncertainty(z0), E.uncertainty(z0, z0 > 0))
    # a gate on the other side of a small logit moves the gradient by the whole term: what the kernel's own gate is passed for
    flipped = (z0 > 0).clone()
    flipped[0, 1] = ~flipped[0, 1]
    assert float((E.edl_grad(z0, labels, flipped) - grads[0][1]).abs().max()) > 1e-4 * float(grads[0][1].abs().max())


def test_predictions_uncertainty_and_the_combination_rule():
    """argmax relu(z) takes the first index on ties and 0 when no logit is positive; u = K / S is exactly 1 without evidence; the
    combined prediction is that of the strictly least uncertain head, 0 on a tie for the minimum (models/avmnist.py:517-537)."""
    z = torch.tensor([[[-1.0, -2.0, -0.5], [0.0, 3.0, 3.0], [1.0, 0.5, -4.0]],          # head 0: none, tie of 1 / 2, class 0
                      [[-1.0, 2.0, -0.5], [0.0, 3.0, 3.0], [-1.0, -0.5, -4.0]],         # head 1: class 1, the same tie, none
                      [[-3.0, -2.0, 0.25], [0.0, 0.0, 9.0], [-1.0, -0.5, -4.0]]], dtype=torch.float64)
    ref = E.heads([torch.zeros(3, 4)] * 3, [torch.zeros(3, 4)] * 3, [torch.zeros(3)] * 3, [1.0] * 3, torch.tensor([0, 1, 2]))
    assert float(ref["uncertainty"].min()) == 1.0 and int(ref["preds"].abs().max()) == 0 and int(ref["combined"].abs().max()) == 0
    preds, u = torch.relu(z).argmax(dim=2), E.uncertainty(z)
    assert preds.tolist() == [[0, 1, 0], [1, 1, 0], [2, 2, 0]]
    assert u[0, 0] == 1.0 and u[1, 2] == 1.0 and u[0, 1] == u[1, 1]
    # sample 0: head 1 (u = 3 / 5) is strictly least -> 1; sample 1: head 2 (3 / 12) -> 2; sample 2: head 0 (3 / 4.5) -> 0
    assert E.combine(preds, u).tolist() == [1, 2, 0]
    # two heads bit-equal at the minimum: 0, whatever they predict
    assert E.combine(preds[:2, 1:2], u[:2, 1:2]).tolist() == [0]
    # the reference's own expression (three heads) on random logits
    gen = torch.Generator().manual_seed(3)
    z = torch.randn(3, 50, 5, generator=gen, dtype=torch.float64)
    p, un = torch.relu(z).argmax(dim=2), E.uncertainty(z)
    want = (p[2] * ((un[2] < un[0]) & (un[2] < un[1])).long() + p[0] * ((un[0] < un[2]) & (un[0] < un[1])).long()
            + p[1] * ((un[1] < un[2]) & (un[1] < un[0])).long())
    assert torch.equal(E.combine(p, un), want)


def test_every_case_seed_stays_under_the_exclusion_cap():
    """A property of the inputs alone: at the seed the table resolves to, fewer than 1 % of the head decisions and of the combined
    decisions lie inside the margins; B, D, K, heads, token counts, slots, weights and aliasing cover what the issue lists."""
    for case in E.EDL_CASES:
        inp = E.edl_inputs(case)
        ref = E.heads(inp["xs"], inp["ws"], inp["bs"], case["coef"], inp["labels"])
        assert float((~ref["head_decided"]).float().mean()) < LR.PRED_EXCLUDED_MAX, case["name"]
        assert float((~ref["combined_decided"]).float().mean()) < LR.PRED_EXCLUDED_MAX, case["name"]
        assert 0.5 < float(ref["logits"].abs().max()) < 8.0                                  # logits ~ N(0, 1)
        if ref["logits"].numel() >= 100:
            assert 0.3 < float((ref["logits"] > 0).float().mean()) < 0.7                     # both sides of the gate
        if case["gpart"]:
            assert case["K"] * case["D"] + case["K"] + 2 <= 1472
    cover = lambda f: {f(c) for c in E.EDL_CASES}
    assert cover(lambda c: c["D"]) == {32, 64, 128, 256}
    assert cover(lambda c: c["B"]) == {1, 3, 4, 5, 64, 65, 81}
    assert cover(lambda c: c["K"]) == {2, 3, 10, 23, 32}
    assert cover(lambda c: len(c["forms"])) == {1, 2, 3, 4}
    assert {f[1] for c in E.EDL_CASES for f in c["forms"] if f != "p"} == {1, 7, 9, 25}
    for key in ("gpart", "dev_weights", "alias"):
        assert cover(lambda c: c[key]) == {False, True}, key


def test_header_binding_and_library_carry_the_entry_point():
    from m2_mixer_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "m2mixer.h")).read()
    decl = re.search(r"int m2m_heads_edl\(([^;]*)\);", header)
    assert decl is not None
    args = [a.strip() for a in decl.group(1).replace("\n", " ").split(",")]
    assert len(args) == 14 and args[9].endswith("uncertainty") and args[10].endswith("combined") and args[-1] == "void* stream"
    res, argtypes = L.SIGNATURES["m2m_heads_edl"]
    assert len(argtypes) == 14
    assert "#define M2M_ABI_VERSION 18" in header and L.ABI_VERSION == 18                     # an addition within ABI 18
    for line in ("models/avmnist.py:447-572", "modules/losses.py:5-31"):
        assert line in header and line in open(os.path.join(ROOT, "m2_mixer_amd", "csrc", "edl.hip")).read()
    assert "edl.hip" in open(os.path.join(ROOT, "m2_mixer_amd", "csrc", "Makefile")).read()
    assert hasattr(L.lib(), "m2m_heads_edl")
    from m2_mixer_amd import runtime
    assert callable(runtime.heads_edl)


def _model_cfg(**extra):
    import gen_util as G
    c = G.AVMNIST["S"]
    mods = {"image": dict(c["image"], block_type="MLPMixer"), "audio": dict(c["audio"], block_type="MLPMixer"),
            "multimodal": dict(c["multimodal"], block_type="FusionMixer", fusion_function="ConcatFusion"),
            "classification": dict(classifier="StandardClassifier", num_classes=c["num_classes"],
                                   input_shape=[16, 49, c["multimodal"]["hidden_dim"]])}
    return {"dropout": 0.0, "modalities": mods, **extra}


def test_module_keeps_the_state_dict_keys_and_its_schedule_stays_off_the_engine():
    from m2_mixer_amd import models as MD
    base = MD.AVMnistMixerMultiLoss(_model_cfg(), {"lr": 1e-2})
    uq = MD.AVMnistMixerMultiLossUQ(_model_cfg(fusion_loss_change=0.25), {"lr": 1e-2})
    assert list(uq.state_dict()) == list(base.state_dict())
    assert [tuple(v.shape) for v in uq.state_dict().values()] == [tuple(v.shape) for v in base.state_dict().values()]
    assert uq.TEST_PRED_KEYS == base.TEST_PRED_KEYS and uq.num_classes == 10

    class Refusing:                                    # an engine whose loss has no fusion_loss_weight
        def set_fusion_loss_weight(self, w):
            raise AssertionError("the schedule reached the engine")

    uq._engine = Refusing()
    w0 = uq.fusion_loss_weight
    uq.validation_epoch_end([])
    assert uq.fusion_loss_weight == pytest.approx(w0 + 0.25)          # the attribute moves, as in the reference (its loss ignores it)
    # the torch loss of the unbound shared_step is the restated one
    _, logits, labels = _fixture(5, 10)
    assert float(MD.edl_mse_loss(logits, labels)) == pytest.approx(float(E.edl_loss(logits, labels)), abs=1e-15)


def test_engine_refuses_rank_scores_before_allocating_anything(monkeypatch):
    from m2_mixer_amd import engine as EN
    import gen_util as G

    def no_alloc(*a, **k):
        raise AssertionError("allocated before the refusal")

    monkeypatch.setattr(EN._FlatEngine, "__init__", no_alloc)
    with pytest.raises(RuntimeError, match="rank_scores"):
        EN.AVMnistUQEngine(dict(G.AVMNIST["S"]), 8, rank_scores=True)
    assert issubclass(EN.AVMnistUQEngine, EN.AVMnistEngine)
    assert EN.AVMnistUQEngine._heads_are_ce(object()) is False and EN.AVMnistUQEngine._heads_write_slots(object()) is True
    # the slot hook returns what the gate it replaces returned for every existing engine
    for cls in (EN.AVMnistEngine, EN.MMIMDBEngine):
        assert cls._heads_write_slots(cls.__new__(cls)) is cls._heads_are_ce(cls.__new__(cls))
