"""Gradient-Blending on the fused engines (-m gpu): engine.clone, engine.probe, gradblend.GradBlend end to end on the schedule of
tests/golden/blend_cases.py against the float64 restatement tests/blend_ref.py (which tests/test_host_gradblend.py holds against
the reference's recorded run), and the bound task module's on_train_epoch_start.

Bars.  Every loss sum is a sum of `nb` batch-mean losses: nb x the project's per-batch loss bar (fp32 1e-3, bf16 2e-2, absolute:
tests/test_gpu_two_stage.py).  The weights divide by G^2 and nobody has measured how far the fp32 kernels drift over 30 Adam
steps: their deviation from blend_ref is recorded (observe), not barred; what is asserted is that they are exactly
normalise(blend_weight(...)) of the engine's own sums, finite, in [0, 1], sum to 1 and come in the fixture's order (its pairwise
gaps are >= 0.1).  In bf16 the reference defines no trajectory: the sums before training are barred, the rest must be finite.

Observed (MI355X, fp32, 48 / 40 train samples): see DESIGN.md section 15."""
import math
import os

import numpy as np
import pytest
import torch

import blend_cases as BC
import blend_ref as BR
import engine_ref as R
import gen_util as G
from conftest import observe
from engine_cases import CASES, Case
from test_gpu_engine_backed import avmnist_batch, make_net
from test_gpu_two_stage import BARS, LR, PARAM_SEED, build, dev, err  # noqa: F401

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
AV = Case("gradblend_avmnist_S", "avmnist", BC.CFG, BC.B, 0.0, {})
MIMIC8 = next(c for c in CASES if c.name == "mimic_patches_8")
SEED = int(np.load(os.path.join(HERE, "golden", "gradblend.npz"))["seed"])
_REF = {}


def restated(n):
    """blend_ref.get_weights on the fixture's schedule: computed once per train size, shared, left unchanged."""
    if n not in _REF:
        sums, ws = BR.get_weights(AV, BC.params(SEED), BC.data(SEED, n), BC.NVAL, BC.B, BC.orders(SEED, n))
        _REF[n] = (sums.numpy(), ws.numpy())
    return _REF[n]


def state_of(eng):
    return [t.clone() for t in (eng.flat_p, eng.flat_g, eng.flat_m, eng.flat_v, eng.adam_state, eng.drop_step)]


def same_state(eng, snap, upto=6):
    return all(torch.equal(a, b) for a, b in list(zip((eng.flat_p, eng.flat_g, eng.flat_m, eng.flat_v, eng.adam_state, eng.drop_step), snap))[:upto])


@pytest.mark.parametrize("case", [AV, MIMIC8], ids=lambda c: c.name)
def test_clone_is_independent_and_starts_fresh(case, dev):
    params = G.make_params(R.case_shapes(case), PARAM_SEED)
    eng = build(case, "fp32", dev, params)
    batches = [tuple(t.to(dev) for t in R.case_batch(case, 301 + i)) for i in range(3)]
    eng.fused_step(*batches[0])                          # non-zero moments and counters on the original
    torch.cuda.synchronize()
    snap = state_of(eng)
    twin = eng.clone()
    assert type(twin) is type(eng) and twin.B == eng.B and twin.prec == eng.prec and twin.scores is None and twin.rank is None
    assert twin.flat_p.data_ptr() != eng.flat_p.data_ptr() and twin._stage_group is not eng._stage_group
    assert torch.equal(twin.flat_p, eng.flat_p) and torch.equal(twin.loss_weights, eng.loss_weights)
    assert float(twin.flat_m.abs().max()) == 0.0 and float(twin.flat_v.abs().max()) == 0.0
    assert float(twin.adam_state[0]) == 0.0 and int(twin.drop_step[0]) == 0 and float(twin.adam_state[1]) == float(eng.adam_state[1])
    assert eng.clone(5).B == 5
    # the clone's first step is a fresh engine's with the same parameters: same forward, same gradient, same first moments
    fresh = build(case, "fp32", dev, {k: v.clone() for k, v in eng.params.items()})
    for e in (twin, fresh):
        e.forward_backward(*batches[1])
    torch.cuda.synchronize()
    assert err(twin.losses, fresh.losses) < 1e-5 * float(fresh.losses.abs().max())
    gscale = float(fresh.flat_g.abs().max())
    assert err(twin.flat_g, fresh.flat_g) < 1e-5 * gscale, "gradients of the first step (float atomics: order noise only)"
    for e in (twin, fresh):
        e.optimizer_step()
    twin.fused_step(*batches[2])
    torch.cuda.synchronize()
    assert float(twin.adam_state[0]) == 2.0 and int(twin.drop_step[0]) == 2
    assert not torch.equal(twin.flat_p, eng.flat_p)
    assert same_state(eng, snap), "two steps on the clone changed the original"


@pytest.mark.parametrize("case", [AV, MIMIC8], ids=lambda c: c.name)
def test_probe_writes_only_the_step_outputs_and_the_dropout_counter(case, dev):
    assert case.p == 0
    params = G.make_params(R.case_shapes(case), PARAM_SEED)
    eng = build(case, "fp32", dev, params)
    batches = [tuple(t.to(dev) for t in R.case_batch(case, 311 + i)) for i in range(2)]
    eng.fused_step(*batches[0])
    torch.cuda.synchronize()
    snap = state_of(eng)
    out = eng.probe(*batches[1])
    torch.cuda.synchronize()
    assert out is eng.losses
    assert same_state(eng, snap, upto=5), "probe() wrote a parameter, gradient, moment or the Adam count"
    assert int(eng.drop_step[0]) == int(snap[5][0]) + 1, "the dropout counter advances as in a training step"
    probed = dict(losses=eng.losses.clone(), logits=eng.logits.clone(), preds=eng.preds.clone())
    eng.evaluate(*batches[1])
    torch.cuda.synchronize()
    rel = err(probed["losses"], eng.losses) / float(eng.losses.abs().max())
    observe(f"probe vs evaluate at p = 0, {case.engine} losses (rel)", rel, 1e-5)
    assert rel < 1e-5                                     # the capture-vs-eager bar
    assert torch.equal(probed["preds"], eng.preds)
    # in the modalities-only stage the probe is that stage's forward
    eng.train_modalities_only()
    snap = state_of(eng)
    eng.probe(*batches[1])
    torch.cuda.synchronize()
    assert same_state(eng, snap, upto=5)
    assert float(eng.losses[2]) == 0.0 and torch.equal(eng.losses[3], eng.losses[0] + eng.losses[1])
    assert err(eng.losses[:2], probed["losses"][:2]) < 1e-5 * float(probed["losses"][:2].abs().max())


def run_gradblend(prec, n, dev):
    from m2_mixer_amd.data import ResidentTensors
    from m2_mixer_amd.engine import AVMnistEngine
    from m2_mixer_amd.gradblend import GradBlend
    eng = AVMnistEngine(BC.CFG, BC.B, device=dev, precision=prec, lr=1e-2, init=False)
    eng.load_state_dict(BC.params(SEED))
    torch.cuda.synchronize()
    before = state_of(eng)
    data = ResidentTensors({"train": tuple(t.to(dev) for t in BC.data(SEED, n))})
    gb = GradBlend(eng, data, val_fraction=BC.val_fraction(n), epochs=BC.EPOCHS, lr=1e-3, orders=BC.orders(SEED, n))
    ws = gb.get_weights()
    torch.cuda.synchronize()
    assert same_state(eng, before), "GradBlend works on clones: the engine itself is untouched"
    assert list(ws) == list(BC.HEADS) == list(gb.sums)
    sums = np.asarray([[gb.sums[h][k] for k in BC.SUMS] for h in BC.HEADS], dtype=np.float64)
    return gb, sums, np.asarray([ws[h] for h in BC.HEADS])


@pytest.mark.parametrize("n", BC.TRAIN_SIZES)
def test_gradblend_end_to_end_fp32(n, dev):
    from m2_mixer_amd.gradblend import blend_weight, normalise
    gb, sums, ws = run_gradblend("fp32", n, dev)
    want_sums, want_ws = restated(n)
    nb = np.asarray([math.ceil(n / BC.B), math.ceil(BC.NVAL / BC.B)] * 2, dtype=np.float64)      # batches in n_train, n_val, nn_train, nn_val
    bad = []
    for h, head in enumerate(BC.HEADS):
        for k, key in enumerate(BC.SUMS):
            dev_ = abs(sums[h, k] - want_sums[h, k])
            observe(f"gradblend fp32 n{n} {head} {key} (abs)", dev_, nb[k] * BARS["fp32"]["losses"])
            print(f"n{n} {head} {key}: engine {sums[h, k]:.9f} float64 {want_sums[h, k]:.9f} dev {dev_:.3e}")
            if not dev_ < nb[k] * BARS["fp32"]["losses"]:
                bad.append(f"{head} {key}: {dev_:.3e}")
    own = normalise([blend_weight(*row) for row in sums])
    assert list(ws) == own, "the weights are the host arithmetic of the engine's own sums"
    assert all(math.isfinite(w) and 0.0 <= w <= 1.0 for w in ws) and abs(sum(ws) - 1.0) < 1e-6
    for head, w, ww in zip(BC.HEADS, ws, want_ws):
        observe(f"gradblend fp32 n{n} weight {head} (abs, recorded: no bar yet)", abs(w - ww), float("inf"))
        print(f"n{n} weight {head}: engine {w:.6f} float64 {ww:.6f}")
    assert not bad, "; ".join(bad)
    assert list(np.argsort(ws)) == list(np.argsort(want_ws)), (list(ws), list(want_ws))


def test_gradblend_end_to_end_bf16(dev):
    n = BC.TRAIN_SIZES[1]                                 # the split with the ragged tail
    gb, sums, ws = run_gradblend("bf16", n, dev)
    want_sums, _ = restated(n)
    nb = (math.ceil(n / BC.B), math.ceil(BC.NVAL / BC.B))
    for h, head in enumerate(BC.HEADS):
        for k in (0, 1):                                  # the sums before training
            dev_ = abs(sums[h, k] - want_sums[h, k])
            observe(f"gradblend bf16 n{n} {head} {BC.SUMS[k]} (abs)", dev_, nb[k] * BARS["bf16"]["losses"])
            assert dev_ < nb[k] * BARS["bf16"]["losses"], (head, BC.SUMS[k], dev_)
        print(f"bf16 n{n} {head}: sums {sums[h]} weight {ws[h]:.6f}")
    assert np.isfinite(sums).all() and np.isfinite(ws).all() and abs(ws.sum() - 1.0) < 1e-6


def test_gradblend_on_the_mimic_engine_and_refusals(dev):
    from m2_mixer_amd.data import ResidentTensors
    from m2_mixer_amd.engine import AVMnistEngine, AVMnistUQEngine
    from m2_mixer_amd.gradblend import GradBlend, blend_weight, normalise
    case = MIMIC8
    eng = build(case, "fp32", dev, G.make_params(R.case_shapes(case), PARAM_SEED))
    data = ResidentTensors({"train": tuple(t.to(dev) for t in G.mimic_batch(40, 7, case.cfg))})
    gb = GradBlend(eng, data, val_fraction=0.2, epochs=2, seed=3)
    ws = gb.get_weights()
    assert list(ws) == ["static", "time", "fusion"]
    own = normalise([blend_weight(*(gb.sums[h][k] for k in BC.SUMS)) for h in ws])
    assert list(ws.values()) == own and abs(sum(own) - 1) < 1e-6 and all(math.isfinite(w) for w in own)
    for h in ws:                                         # every model was retrained: its sums moved
        s = gb.sums[h]
        assert all(math.isfinite(v) for v in s.values()) and s["nn_train"] != s["n_train"] and s["nn_val"] != s["n_val"], h
    with pytest.raises(ValueError, match="full training batch"):
        GradBlend(eng, data, val_fraction=0.9).get_weights()
    summed = dict(BC.CFG, multimodal=dict(BC.CFG["multimodal"], fusion_function="SumFusion"))      # (4 + 4 tokens: equal counts)
    with pytest.raises(NotImplementedError, match="ConcatFusion"):
        GradBlend(AVMnistEngine(summed, 4, device=dev, precision="fp32"), data)
    with pytest.raises(NotImplementedError, match="evidential"):
        GradBlend(AVMnistUQEngine(BC.CFG, 4, device=dev, precision="fp32"), data)


def test_bound_module_refreshes_its_weights_and_keeps_its_graph(dev):
    from m2_mixer_amd.data import ResidentTensors
    net, _ = make_net("avmnist", BC.CFG, 17, dev, gradblend=True, gb_update_freq=2, gb_epochs=1)
    eng = net.bind_engine(BC.B, precision="fp32")
    data = ResidentTensors({"train": tuple(t.to(dev) for t in BC.data(SEED, 48))})
    batch = avmnist_batch(BC.B, 41, BC.CFG, dev)
    net.training_step(batch)                             # captures the step's graph
    graph = eng._graph
    assert graph is not None
    net.current_epoch = 0
    w = net.on_train_epoch_start(data)
    torch.cuda.synchronize()
    assert net.gb_weights == [w["audio"], w["image"], w["fusion"]], "the reference's list order (models/avmnist.py:283-288)"
    want = torch.tensor([w["image"], w["audio"], w["fusion"]], dtype=torch.float32)
    assert torch.equal(eng.loss_weights.cpu(), want), "the engine's table, in its head order"
    assert abs(sum(net.gb_weights) - 1) < 1e-6 and eng._graph is graph, "the captured graph is kept"
    net.current_epoch = 1
    kept = list(net.gb_weights)
    assert net.on_train_epoch_start(data) is None and net.gb_weights == kept, "epoch 1 recomputes nothing"
    out = net.training_step(batch)
    torch.cuda.synchronize()
    assert eng._graph is graph
    total = w["fusion"] * float(out["loss_fusion"]) + w["image"] * float(out["loss_image"]) + w["audio"] * float(out["loss_audio"])
    assert abs(float(out["loss"]) - total) < BARS["fp32"]["losses"]
    ev = net.validation_step(batch)
    total = w["fusion"] * float(ev["loss_fusion"]) + w["image"] * float(ev["loss_image"]) + w["audio"] * float(ev["loss_audio"])
    assert abs(float(ev["loss"]) - total) < BARS["fp32"]["losses"], "gb_weights hold in every mode"
    # the schedule of validation_epoch_end no longer reaches the engine's table
    net.fusion_loss_change, net.loss_change_epoch = 0.1, 0
    net.validation_epoch_end()
    assert torch.equal(eng.loss_weights.cpu(), want)
