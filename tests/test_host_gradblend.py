"""Gradient-Blending, host side (no GPU): the weight arithmetic against the reference's recorded sums and weights
(tests/golden/gradblend.npz, written by tests/golden/make_golden_gradblend.py from modules/gradblend.py), the float64
restatement tests/blend_ref.py against the same fixture, the flat ranges of the modalities-only stage on every configuration of
tests/engine_cases.py, and the task modules' cfg handling."""
import os

import numpy as np
import pytest
import torch

import blend_cases as BC
import blend_ref as BR
import engine_ref as R
import gen_util as G
import stage_ref as S
from engine_cases import CASES, Case

HERE = os.path.dirname(os.path.abspath(__file__))
CASE = Case("gradblend_avmnist_S", "avmnist", BC.CFG, BC.B, 0.0, {})


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(HERE, "golden", "gradblend.npz")))


@pytest.fixture(scope="module")
def restated(golden):
    """blend_ref.get_weights on the fixture's schedule, once per train size."""
    seed = int(golden["seed"])
    out = {}
    for n in BC.TRAIN_SIZES:
        sums, ws = BR.get_weights(CASE, BC.params(seed), BC.data(seed, n), BC.NVAL, BC.B, BC.orders(seed, n))
        out[n] = (sums.numpy(), ws.numpy())
    return out


@pytest.mark.parametrize("n", BC.TRAIN_SIZES)
def test_weight_arithmetic_reproduces_the_reference(golden, n):
    from m2_mixer_amd.gradblend import blend_weight, normalise
    sums, want = golden[f"n{n}.f64.sums"], golden[f"n{n}.f64.weights"]
    assert sums.shape == (3, 4) and sums.dtype == np.float64
    got = normalise([blend_weight(*row) for row in sums])
    assert all(isinstance(w, float) for w in got)
    assert np.abs(np.asarray(got) / want - 1).max() < 1e-12
    assert abs(sum(got) - 1) < 1e-12


def test_fixture_is_well_conditioned(golden):
    for n in BC.TRAIN_SIZES:
        sums, ws = golden[f"n{n}.f64.sums"], golden[f"n{n}.f64.weights"]
        for n_tr, n_va, nn_tr, nn_va in sums:
            assert abs(nn_va - n_va) >= 1e-2 * n_va and abs((nn_va - nn_tr) - (n_va - n_tr)) >= 5e-2 * n_va
        assert min(abs(ws[i] - ws[j]) for i in range(3) for j in range(i)) >= 0.1


@pytest.mark.parametrize("n", BC.TRAIN_SIZES)
def test_float64_restatement_reproduces_the_reference(golden, restated, n):
    sums, ws = restated[n]
    s64, s32 = golden[f"n{n}.f64.sums"], golden[f"n{n}.f32.sums"]
    assert np.abs(sums / s64 - 1).max() < 1e-9
    bar32 = 10 * np.abs(s32 / s64 - 1).max()             # ten times the reference's own fp32 - float64 deviation
    assert np.abs(sums / s32 - 1).max() < bar32
    assert np.abs(ws / golden[f"n{n}.f64.weights"] - 1).max() < 1e-6       # (w divides by G^2: the sums' 1e-9, amplified)
    assert list(np.argsort(ws)) == list(np.argsort(golden[f"n{n}.f64.weights"]))


def test_modality_step_trains_the_modality_keys_only():
    case = CASE._replace(B=5)
    params = G.make_params(R.case_shapes(case), 5)
    one = R.Step(case, params, 2e-3)
    one.step(R.case_batch(case, 1))
    both = BR.ModalityStep(one)
    img, aud = BR.ModalityStep(one, (0,)), BR.ModalityStep(one, (1,))
    batch = R.case_batch(case, 2)
    out = both.step(batch)
    img.step(batch)
    aud.step(batch)
    assert float(out["losses"][2]) == 0.0 and float(out["losses"][3]) == float(out["losses"][0] + out["losses"][1])
    for k in one.p:
        modal = BR.is_modal(case, k)
        assert modal == S.is_frozen(case, k), "the stage trains exactly what stage two freezes"
        if not modal:
            assert torch.equal(both.p[k], one.p[k]) and torch.equal(both.m[k], one.m[k]) and torch.equal(both.v[k], one.v[k]), k
        elif not k.endswith(R.NOISE_KEYS):
            assert not torch.equal(both.p[k], one.p[k]), k
        # the two unimodal models share no parameter and Adam is element-wise: trained at once == trained separately
        src = img if BR.is_modal(case, k, (0,)) else (aud if BR.is_modal(case, k, (1,)) else one)
        assert torch.equal(both.p[k], src.p[k]), k
    assert both.t == 2


def engine_shapes(case):
    from m2_mixer_amd import engine as E
    if case.engine == "mimic":
        return E.mimic_param_shapes(case.cfg)
    return E.two_tower_param_shapes(case.cfg, S.MODS[case.engine])


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_modality_stage_ranges_complement_stage_two(case):
    from m2_mixer_amd import engine as E
    shapes = engine_shapes(case)
    prefixes = E.frozen_key_prefixes(S.MODS[case.engine])
    two = E.trainable_flat_ranges(shapes, prefixes)
    modal = E.trainable_flat_ranges(shapes, prefixes, invert=True)
    n_params = sum(int(torch.Size(s).numel()) for s in shapes.values())
    cover = np.zeros(n_params, dtype=np.int8)
    for lo, hi in two + modal:
        assert lo < hi
        cover[lo:hi] += 1
    assert (cover == 1).all(), "the two stages' ranges are disjoint and tile [0, n_params)"
    assert all(a[1] < b[0] for a, b in zip(modal, modal[1:])), "sorted and merged"
    keys = {k for k in shapes if BR.is_modal(case, k)}
    assert keys == {k for k in shapes if S.is_frozen(case, k)}
    for lo, hi in S.flat_ranges(shapes, keys):
        assert any(a <= lo and hi <= b for a, b in modal)
    assert len(modal) == 2, "the two towers (adjacent segments), then the two modality heads"


def module_cfg(task, **extra):
    c = BC.CFG if task == "avmnist" else G.MIMIC_H
    fusion = dict(c["multimodal"], block_type="FusionMixer", fusion_function="ConcatFusion")
    if task == "mimic":
        mods = {"static": dict(c["static"], block_type="MLP"), "time": dict(c["time"], block_type="MLPMixerNoPatching")}
    else:
        mods = {"image": dict(c["image"], block_type="MLPMixer"), "audio": dict(c["audio"], block_type="MLPMixer")}
    mods["multimodal"] = fusion
    mods["classification"] = dict(classifier="StandardClassifier", num_classes=c["num_classes"], input_shape=[16, 49, c["multimodal"]["hidden_dim"]])
    return dict({"dropout": 0.0, "modalities": mods}, **extra)


def test_task_modules_accept_gradblend_and_refuse_softadapt():
    from m2_mixer_amd import models as MD
    for task, cls, order in (("avmnist", MD.AVMnistMixerMultiLoss, ("audio", "image", "fusion")),
                             ("mimic", MD.MimicMixerMultiLoss, ("static", "time", "fusion"))):
        plain = cls(module_cfg(task), {"lr": 1e-2})
        assert not plain.use_gradblend and plain.gb_weights is None and plain.on_train_epoch_start() is None
        for key in ("gradblend", "use_gradblend"):
            net = cls(module_cfg(task, **{key: True}), {"lr": 1e-2})
            assert net.use_gradblend and net.gb_update_freq == 20 and net.gb_epochs == 20 and net.gb_weights is None
            assert net.GB_ORDER == order
        net = cls(module_cfg(task, gradblend=True, gb_update_freq=3, gb_epochs=2), {"lr": 1e-2})
        assert (net.gb_update_freq, net.gb_epochs) == (3, 2)
        with pytest.raises(RuntimeError, match="bind_engine"):
            net.on_train_epoch_start(data=object())          # epoch 0 is due; an unbound module cannot run it
        net.current_epoch = 1
        assert net.on_train_epoch_start(data=object()) is None, "nothing is due between refreshes"
        with pytest.raises(NotImplementedError):
            cls(module_cfg(task, gradblend=True, use_softadapt=True), {"lr": 1e-2})
        # the total in the reference's list order (models/avmnist.py:283-288 -- no x3; models/mimic.py:116-124)
        a, b = cls.MODS
        losses = {a: torch.tensor(2.0), b: torch.tensor(3.0), "fusion": torch.tensor(5.0)}
        assert net._gb_loss(losses) is None
        net.gb_weights = [0.2, 0.3, 0.5]
        w = dict(zip(order, net.gb_weights))
        assert float(net._gb_loss(losses)) == pytest.approx(w[a] * 2.0 + w[b] * 3.0 + 0.5 * 5.0, rel=1e-6)
    for cls in (MD.AVMnistMixerMultiLossUQ,):
        with pytest.raises(NotImplementedError, match="Gradient-Blending"):
            cls(module_cfg("avmnist", gradblend=True), {"lr": 1e-2})


def test_gradblend_host_arithmetic_by_hand():
    from m2_mixer_amd.gradblend import blend_weight, normalise
    # N_train 4, N_val 5 -> overfitting 1; Nn_train 2, Nn_val 4.5 -> 2.5: O = 1.5, G = -0.5, w = 6
    assert blend_weight(4.0, 5.0, 2.0, 4.5) == 6.0
    assert normalise([6.0, 3.0, 1.0]) == [0.6, 0.3, 0.1]
    with pytest.raises(ZeroDivisionError):
        blend_weight(1.0, 2.0, 0.5, 2.0)                  # G == 0: the reference divides by zero as well (a tensor inf there)
