"""The modalities-only stage of the fused engines (-m gpu): every case of tests/engine_cases.py, in fp32 and bf16.

Per case: two ordinary steps, engine.train_modalities_only(), two stage steps (a fused_step, then forward_backward +
optimizer_step), an evaluation -- against the float64 reference (engine_ref.Step twice, then blend_ref.ModalityStep twice, fed
the kernels' own dropout masks where p > 0) at the bars of tests/test_gpu_two_stage.py for the same case and precision (imported:
logits and losses absolute 1e-3 / 2e-2, parameters 2e-3 / 1e-2 with the rounding-level key left out).  The fusion head's logits
are not produced in the stage: the two modality heads' are compared.  The flat ranges of the fusion keys (fusion function, fusion
tower, fusion head) in flat_p, flat_m and flat_v must be torch.equal to their snapshot at the switch after every stage step;
losses[2] == 0 and losses[3] is the fp32 sum losses[0] + losses[1]; the evaluation afterwards is the full model's.

Every call into the library during the stage steps is recorded (as tests/test_gpu_two_stage.py records them): no forward,
backward or weight gradient of the fusion tower, heads launches of two heads, Adam inside the trainable ranges only, no re-pack
of the fusion tower.

One case (AV-MNIST S, B = 13) goes through capture() after the switch, with a training sibling(10) built before it."""
import ctypes as C

import pytest
import torch

import blend_ref as BR
import engine_ref as R
import gen_util as G
import stage_ref as S
from conftest import observe
from engine_cases import CASES
from test_gpu_two_stage import AV_S, BARS, LR, PARAM_SEED, Calls, build, dev, err, masks_equal, snapshot, untouched  # noqa: F401

pytestmark = pytest.mark.gpu

_REFS = {}          # case name -> (masks of the four steps, reference results): computed once, shared by the two precisions


def reference(case, params, batches, masks):
    """Step, Step, ModalityStep, ModalityStep and an evaluation of the first batch with the final parameters."""
    hit = _REFS.get(case.name)
    if hit is not None and all(masks_equal(a, b) for a, b in zip(hit[0], masks)):
        return hit[1]
    one = R.Step(case, params, LR)
    outs = [one.step(batches[0], masks[0]), one.step(batches[1], masks[1])]
    two = BR.ModalityStep(one)
    outs += [two.step(batches[2], masks[2]), two.step(batches[3], masks[3])]
    ref = dict(outs=outs, p4={k: v.clone() for k, v in two.p.items()}, ev=two.forward(batches[0]))
    _REFS[case.name] = (masks, ref)
    return ref


def fusion_ranges(eng, case):
    return S.flat_ranges(eng.shapes, {k for k in eng.shapes if not BR.is_modal(case, k)})


def check_stage_calls(eng, seen, nsteps):
    """The launch list of the modalities-only stage."""
    names = [n for n, _ in seen]
    fus = eng.t_fus.desc
    desc_of = lambda a: getattr(a[0], "_obj", None)
    is_fus = lambda ptr: bool(ptr) and C.addressof(ptr.contents) == C.addressof(fus)
    for gone in ("m2m_fusion_forward", "m2m_gate_forward", "m2m_fusion_backward", "m2m_gate_backward", "m2m_gate_wgrad",
                 "m2m_tower_backward_heads", "m2m_towers_forward_embeds", "m2m_adam_pack_all", "m2m_pack_all"):
        assert gone not in names, gone
    for single in ("m2m_tower_forward", "m2m_tower_backward", "m2m_tower_wgrad", "m2m_pack_tower"):
        assert all(desc_of(a) is not fus for n, a in seen if n == single), f"{single} of the fusion tower"
    for n, a in seen:
        if n in ("m2m_towers_forward", "m2m_towers_backward"):
            assert a[2] == 2 and not any(is_fus(a[0][i]) for i in range(2))
        if n in ("m2m_towers_wgrad", "m2m_towers_wgrad_heads", "m2m_towers_wgrad_tail"):
            assert not any(is_fus(a[0][i]) for i in range(a[2])), "the fusion tower in a weight-gradient launch"
    heads = [a for n, a in seen if n in ("m2m_heads_ce", "m2m_heads_ce_w", "m2m_heads_bce", "m2m_heads_bce_w", "m2m_heads_edl")]
    assert len(heads) == nsteps and all(a[1] == 2 for a in heads), "one heads launch per step, of the two modality heads"
    back = [n for n in names if n in ("m2m_towers_backward", "m2m_tower_backward")]
    assert len(back) in (nsteps, 2 * nsteps), "the two modality towers' backward, as a pair or one by one"
    adam = [(n, a) for n, a in seen if n in ("m2m_adam_step", "m2m_adam_step_ranges", "m2m_adam_step_bf16")]
    assert len(adam) == nsteps * len(eng._trainable)
    base = eng.flat_p.data_ptr()
    for name, a in adam:
        count = a[4] if name == "m2m_adam_step" else a[5]      # (_ranges / _bf16 carry the bf16 gradient pointer before the moments)
        lo = (a[0] - base) // 4
        assert (lo, lo + count) in eng._trainable, (lo, count, eng._trainable)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_modality_stage_against_float64(case, prec, dev):
    params = G.make_params(R.case_shapes(case), PARAM_SEED)
    eng = build(case, prec, dev, params)
    two_tower = case.engine != "mimic"
    masked = case.p > 0
    host = [R.case_batch(case, 101 + i) for i in range(4)]
    gpu = [tuple(t.to(dev) for t in b) for b in host]
    ranges = fusion_ranges(eng, case)
    got, masks, bad = [], [], []

    def record():
        torch.cuda.synchronize()
        masks.append(R.engine_masks(eng, case.B) if masked else None)
        got.append(dict(logits=eng.logits.clone(), losses=eng.losses.clone()))

    for b in gpu[:2]:                                    # ---- ordinary steps
        eng.fused_step(*b)
        record()
    eng.train_modalities_only()
    assert eng._graph is None and eng._modal and not eng._frozen
    with pytest.raises(RuntimeError, match="no way back"):
        eng.freeze_modalities()
    torch.cuda.synchronize()
    snap = snapshot(eng, ranges)
    trainable_before = {k: v.clone() for k, v in eng.params.items() if BR.is_modal(case, k)}
    with Calls() as calls:                               # ---- the stage
        eng.fused_step(*gpu[2])
        record()
        if not untouched(eng, ranges, snap):
            bad.append("a fusion range changed in the fused stage step")
        eng.forward_backward(*gpu[3])
        record()
        eng.optimizer_step()
        torch.cuda.synchronize()
    if not untouched(eng, ranges, snap):
        bad.append("a fusion range changed in forward_backward + optimizer_step")
    check_stage_calls(eng, calls.seen, 2)
    counters = (float(eng.adam_state[0]), int(eng.drop_step[0]))
    p4 = {k: v.clone() for k, v in eng.params.items()}
    eng.evaluate(*gpu[0])
    torch.cuda.synchronize()
    gotev = dict(logits=eng.logits.clone(), losses=eng.losses.clone())

    ref = reference(case, params, host, masks)
    bar, kind = BARS[prec], f"modality stage {case.engine} {prec}"

    def hold(what, value, tol, name):
        observe(f"{kind} {what}", value, tol)
        if not value < tol:
            bad.append(f"{name}: {value:.3e} >= {tol:.0e}")

    for i, (g, w) in enumerate(zip(got, ref["outs"])):
        nh = 3 if i < 2 else 2                           # (the stage computes the two modality heads)
        hold("logits (abs)", err(g["logits"][:nh], w["logits"][:nh]), bar["logits"], f"step {i + 1} logits")
        hold("losses (abs)", err(g["losses"], w["losses"]), bar["losses"], f"step {i + 1} losses")
    for i in (2, 3):
        l = got[i]["losses"]
        if float(l[2]) != 0.0:
            bad.append(f"step {i + 1}: losses[2] = {float(l[2])!r} is not 0")
        if not torch.equal(l[3], l[0] + l[1]):
            bad.append(f"step {i + 1}: losses[3] = {float(l[3])!r} is not the fp32 sum {float(l[0] + l[1])!r}")
    hold("logits (abs)", err(gotev["logits"], ref["ev"]["logits"]), bar["logits"], "eval logits (the full model)")
    hold("losses (abs)", err(gotev["losses"], ref["ev"]["losses"]), bar["losses"], "eval losses (the weighted total)")
    hold("trainable parameters after the stage (abs)",
         max(err(p4[k], v) for k, v in ref["p4"].items() if BR.is_modal(case, k) and not k.endswith(R.NOISE_KEYS)),
         bar["params"], "trainable parameters")
    for k, v in trainable_before.items():
        if not k.endswith(R.NOISE_KEYS) and torch.equal(p4[k], v):
            bad.append(f"trainable {k} did not move in the stage")
    if counters != (4.0, 4):
        bad.append(f"step counters (Adam, dropout) after four steps: {counters}")
    assert not bad, f"{case.name} [{prec}]: " + "; ".join(bad)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_captured_stage_and_a_sibling_built_before_the_switch(prec, dev):
    case = AV_S
    params = G.make_params(R.case_shapes(case), PARAM_SEED)
    eng = build(case, prec, dev, params)
    sib = eng.sibling(10)                                # a training sibling from before the switch
    host = [R.case_batch(case, 201 + i) for i in range(4)]
    gpu = [tuple(t.to(dev) for t in b) for b in host]
    ranges = fusion_ranges(eng, case)
    got, masks = [], []

    def record():
        torch.cuda.synchronize()
        masks.append(R.engine_masks(eng, case.B))
        got.append(dict(logits=eng.logits.clone(), losses=eng.losses.clone()))

    replay = eng.capture(*gpu[0])
    for b in gpu[:2]:
        replay(*b)
        record()
    eng.train_modalities_only()
    assert eng._graph is None, "train_modalities_only drops the captured graph as release_capture does"
    assert sib._modal, "the stage is the family's"
    with pytest.raises(RuntimeError, match="single GPU"):
        eng.train_step(*gpu[2], grad_sync=lambda g: 1.0)
    with pytest.raises(RuntimeError, match="single GPU"):
        eng.capture(*gpu[2], grad_sync=lambda g: 1.0)
    torch.cuda.synchronize()
    snap = snapshot(eng, ranges)
    replay = eng.capture(*gpu[2])
    assert untouched(eng, ranges, snap) and float(eng.adam_state[0]) == 2.0, "capture() does not train"
    for b in gpu[2:]:
        replay(*b)
        record()
        assert float(eng.losses[2]) == 0.0 and torch.equal(eng.losses[3], eng.losses[0] + eng.losses[1])
    assert untouched(eng, ranges, snap)
    p4 = {k: v.clone() for k, v in eng.params.items()}
    ref = reference(case._replace(name=case.name + "_captured"), params, host, masks)
    bar = BARS[prec]
    for i, (g, w) in enumerate(zip(got, ref["outs"])):
        nh = 3 if i < 2 else 2
        assert err(g["logits"][:nh], w["logits"][:nh]) < bar["logits"], f"step {i + 1} logits"
        assert err(g["losses"], w["losses"]) < bar["losses"], f"step {i + 1} losses"
    worst = max(err(p4[k], v) for k, v in ref["p4"].items() if BR.is_modal(case, k) and not k.endswith(R.NOISE_KEYS))
    observe(f"modality stage captured avmnist {prec} trainable parameters (abs)", worst, bar["params"])
    assert worst < bar["params"]
    # the sibling's stage step: its own batch size, the family's ranges
    small = tuple(t[:10].contiguous() for t in gpu[3])
    sib.pack()
    sib.train_step(*small)
    eng.pack()
    torch.cuda.synchronize()
    assert untouched(eng, ranges, snap), "the sibling's step wrote a fusion range"
    assert float(sib.losses[2]) == 0.0 and float(eng.adam_state[0]) == 5.0
    assert not torch.equal(eng.params["classifier_image.weight"], p4["classifier_image.weight"])
    # a sibling built AFTER the switch is in the stage as well
    eng.release_capture()
    late = eng.sibling(case.B - 5)
    assert late._modal and late._trainable == eng._trainable
    late.pack()
    late.train_step(*(t[:case.B - 5].contiguous() for t in gpu[2]))
    torch.cuda.synchronize()
    assert untouched(eng, ranges, snap) and float(late.losses[2]) == 0.0


def test_the_stage_is_refused_where_it_cannot_run(dev):
    case = AV_S
    params = G.make_params(R.case_shapes(case), PARAM_SEED)
    eng = build(case, "bf16", dev, params)
    eng._loss_weight_group["fused_heads"] = True         # what M2M_FUSED_HEADS=1 sets where that launch exists
    with pytest.raises(RuntimeError, match="M2M_FUSED_HEADS"):
        eng.train_modalities_only()
    assert not eng._modal
    scored = R.engine_class(case)(case.cfg, case.B, device=dev, precision="fp32", lr=LR, init=False, scores=True)
    with pytest.raises(RuntimeError, match="scores"):
        scored.train_modalities_only()
    frozen = build(case, "fp32", dev, params)
    frozen.freeze_modalities()
    with pytest.raises(RuntimeError, match="no way back"):
        frozen.train_modalities_only()
