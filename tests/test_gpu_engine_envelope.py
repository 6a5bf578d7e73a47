"""Configuration envelope of the fused training engines (-m gpu): every case of tests/engine_cases.py, in fp32 and bf16.

Per case: the engine is built from the config and the decisions the case is there for (`expect`) are asserted against it
before any launch; then two training steps and an evaluation are compared with the float64 reference (engine_ref.Step: autograd
through the oracle's task forward, fed the kernels' own dropout masks, + oracle.adam_step):

  step 1   forward_backward: the three logits tensors, the four losses, every gradient, preds == argmax / (logit > 0) of the
           engine's own logits; optimizer_step: flat gradient cleared outside the kept ranges, step counter, parameters;
  step 2   forward_backward on a second batch: logits and losses -- wrong after a stale packed operand, a slot that was not
           added, a range that was not cleared or a counter that did not advance (tests/test_host_engine_cases.py checks that
           un-updated parameters would move these logits by >= 10x the bar);
  eval     evaluate() on batch 1 with the updated parameters (dropout off, nothing saved).

Bars (those of test_gpu_fusions.test_engine_step_against_oracle for the same quantities): logits and losses absolute 1e-3
(fp32) / 2e-2 (bf16); gradients 1e-3 / 5e-2 relative to the tensor's max (tighter than max(1, tensor max): these models'
gradients are well below 1); parameters after the update 2e-3 / 1e-2, the rounding-level key left out.

LR = 2e-3.  One Adam step moves a parameter by up to LR whatever its gradient's size, so an element whose bf16 gradient has the
wrong sign ends 2 LR from the reference (the observed bf16 parameter maximum is exactly that), and everything computed from the
updated parameters -- step 2, the evaluation -- carries that noise on top of the kernels' own error, in proportion to LR
(AV-MNIST D = 128 / K = 12, bf16 logits: 3.1e-3 at step 1; at step 2 / eval 9.2e-3 / 1.1e-2 with LR 2e-3, 1.7e-2 / 2.1e-2 with
4e-3).  The gap an un-updated parameter set would leave is proportional to LR as well, and is what bounds LR from below
(tests/test_host_engine_cases.py: >= 10x the bf16 bar needs LR >= 1.7e-3 on the MIMIC cases); 2e-3 is the round value above it.
The step-2 gradients are compared with the reference in fp32 only, where the update agrees to 1e-5; in both precisions they are
compared with those of a fresh engine given the updated parameters (zero gradient buffer, nothing kept from step 1), where a
range that was kept but not overwritten, or cleared but needed, shows at full size.

Observed maxima are recorded per engine / launch path / precision (conftest.observe)."""
import pytest
import torch

import engine_ref as R
import gen_util as G
from conftest import observe
from engine_cases import CASES

pytestmark = pytest.mark.gpu

LR = 2e-3
PARAM_SEED = 31
BARS = {"fp32": dict(logits=1e-3, losses=1e-3, grads=1e-3, params=2e-3), "bf16": dict(logits=2e-2, losses=2e-2, grads=5e-2, params=1e-2)}
CAPTURE_CASES = ("av_token_class_n4_n6_d128_half", "mimic_patches_8")     # two streams; the MLP's flushed ride + a wide fusion tower

_REFS = {}         # case name -> (masks of step 1 and 2, reference results): computed once, shared by the two precisions


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from m2_mixer_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def err(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def build(case, prec, dev, params):
    eng = R.engine_class(case)(case.cfg, case.B, device=dev, precision=prec, lr=LR, init=False)
    eng.load_state_dict(params)
    return eng


def path_of(d):
    if "time_wide" in d:
        return f"mimic time-{'wide' if d['time_wide'] else 'fused'} fusion-{'wide' if d['wide_fus'] else 'fused'}"
    towers = "".join("w" if d[k] else "f" for k in ("wide_a", "wide_b", "wide_fus"))
    return f"{'pair' if d['grouped'] else 'streams'} {towers}"


masks_equal = R.masks_equal


def reference(case, params, b1, b2, masks1, masks2):
    """Two reference steps (kept unchanged once computed; recomputed only if a precision drew other masks)."""
    hit = _REFS.get(case.name)
    if hit is not None and masks_equal(hit[0], masks1) and masks_equal(hit[1], masks2):
        return hit[2]
    ref = R.Step(case, params, LR)
    one = ref.step(b1, masks1)
    p1 = {k: v.clone() for k, v in ref.p.items()}
    two = ref.step(b2, masks2)
    out = dict(one=one, p1=p1, two=two, ev=ref.forward(b1, p1))
    _REFS[case.name] = (masks1, masks2, out)
    return out


def own_preds(case, logits):
    return (logits > 0).int() if case.engine == "mmimdb" else logits.argmax(-1).int()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_engine_case_against_float64(case, prec, dev):
    params = G.make_params(R.case_shapes(case), PARAM_SEED)
    eng = build(case, prec, dev, params)
    assert list(eng.shapes) == list(params)
    took = R.decisions(eng)
    want = R.expected(case, prec)
    wrong = {k: (took.get(k), v) for k, v in want.items() if took.get(k) != v}
    assert not wrong, f"{case.name} [{prec}] is off its arm (decision: (engine, table)): {wrong}"

    b1, b2 = R.case_batch(case, 101), R.case_batch(case, 102)
    g1, g2 = tuple(t.to(dev) for t in b1), tuple(t.to(dev) for t in b2)
    masked = case.p > 0
    # ---- the GPU side, start to end (the reference needs the masks of both steps) ----
    eng.forward_backward(*g1)
    torch.cuda.synchronize()
    masks1 = R.engine_masks(eng, case.B) if masked else None
    got1 = dict(logits=eng.logits.clone(), losses=eng.losses.clone(), preds=eng.preds.clone(), grads={k: v.clone() for k, v in eng.grads.items()})
    eng.optimizer_step()
    torch.cuda.synchronize()
    cleared, adam_t, drop_t = R.grads_cleared(eng), float(eng.adam_state[0]), int(eng.drop_step[0])
    p1 = {k: v.clone() for k, v in eng.params.items()}
    eng.forward_backward(*g2)
    torch.cuda.synchronize()
    masks2 = R.engine_masks(eng, case.B) if masked else None
    got2 = dict(logits=eng.logits.clone(), losses=eng.losses.clone(), grads={k: v.clone() for k, v in eng.grads.items()})
    adam_t2, drop_t2 = float(eng.adam_state[0]), int(eng.drop_step[0])
    # a fresh engine (zero gradient buffer, nothing kept, nothing stale) on the updated parameters, same batch and dropout step
    twin = build(case, prec, dev, eng.state_dict())
    twin.drop_step.fill_(drop_t2 - 1)
    twin.forward_backward(*g2)
    torch.cuda.synchronize()
    twin_grads = {k: v.clone() for k, v in twin.grads.items()}
    del twin
    eng.evaluate(*g1)
    torch.cuda.synchronize()
    gotev = dict(logits=eng.logits.clone(), losses=eng.losses.clone(), preds=eng.preds.clone())

    ref = reference(case, params, b1, b2, masks1, masks2)
    bar, kind = BARS[prec], f"engine {path_of(took)} {prec}"
    bad = []

    def hold(what, value, tol, name):
        observe(f"{kind} {what}", value, tol)
        if not value < tol:
            bad.append(f"{name}: {value:.3e} >= {tol:.0e}")

    for tag, got, want_ in (("step 1", got1, ref["one"]), ("step 2", got2, ref["two"]), ("eval", gotev, ref["ev"])):
        hold("logits (abs)", err(got["logits"], want_["logits"]), bar["logits"], f"{tag} logits")
        hold("losses (abs)", err(got["losses"], want_["losses"]), bar["losses"], f"{tag} losses")
    for tag, got, want_ in (("step 1", got1, ref["one"]), ("step 2", got2, ref["two"])):
        if tag == "step 2" and prec != "fp32":
            continue
        for k, g in want_["grads"].items():
            scale = float(g.abs().max())
            if k.endswith(R.NOISE_KEYS):
                # under a final LayerNorm this bias shifts a whole token row, which every later LayerNorm removes: its true
                # gradient is exactly zero, so it is measured against its weight's gradient scale (tests/test_gpu_shape_envelope.py)
                floor = float(want_["grads"][k[:-4] + "weight"].abs().max())
                scale = scale if scale > 1e-6 * floor else floor
            hold("gradients (rel to max)", err(got["grads"][k], g) / max(scale, 1e-30), bar["grads"], f"{tag} grad {k}")
    # step 2 against the fresh engine: same kernels, parameters and masks, so only the order of fp32 sums may differ (the bar of
    # test_gpu_parity.test_launch_forms_of_a_step_agree) -- in both precisions, free of the first update's sign noise
    for k, g in twin_grads.items():
        if k.endswith(R.NOISE_KEYS):
            continue
        if float(g.abs().max()) == 0.0:
            if float(got2["grads"][k].abs().max()) != 0.0:
                bad.append(f"step 2 grad {k}: not zero as in a fresh engine")
            continue
        hold("step-2 gradients vs a fresh engine (rel to max)", relerr(got2["grads"][k], g), 2e-4, f"step 2 grad {k} vs fresh engine")
    hold("parameters after the update (abs)", max(err(p1[k], v) for k, v in ref["p1"].items() if not k.endswith(R.NOISE_KEYS)),
         bar["params"], "parameters")
    for tag, got in (("step 1", got1), ("eval", gotev)):
        if not torch.equal(got["preds"].cpu(), own_preds(case, got["logits"]).cpu()):
            bad.append(f"{tag} preds are not those of the engine's own logits")
    if not cleared:
        bad.append("the update left gradient elements uncleared outside the kept ranges")
    if (adam_t, drop_t, adam_t2, drop_t2) != (1.0, 1, 2.0, 2):
        bad.append(f"step counters (Adam, dropout) after steps 1 and 2: {(adam_t, drop_t, adam_t2, drop_t2)}")
    assert not bad, f"{case.name} [{prec}]: " + "; ".join(bad)


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max()) / (float(b.abs().max()) + 1e-12)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", CAPTURE_CASES)
def test_captured_step_equals_the_eager_step(name, prec, dev):
    """capture + one replay of the whole step (forked streams and all) against the eager fused_step: same parameters, batch and
    dropout step.  Bars of test_gpu_parity.test_launch_forms_of_a_step_agree: logits 1e-5, gradients 2e-4 of the tensor's max --
    read off Adam's first moment (0.1 x the gradient after step 1; the step itself clears the gradient)."""
    case = next(c for c in CASES if c.name == name)
    params = G.make_params(R.case_shapes(case), PARAM_SEED)
    batch = tuple(t.to(dev) for t in R.case_batch(case, 101))
    eager, graphed = build(case, prec, dev, params), build(case, prec, dev, params)
    eager.fused_step(*batch)
    replay = graphed.capture(*batch)
    replay(*batch)
    torch.cuda.synchronize()
    assert float(graphed.adam_state[0]) == 1.0 and int(graphed.drop_step[0]) == 1
    assert relerr(graphed.logits, eager.logits) < 1e-5 and relerr(graphed.losses, eager.losses) < 1e-5
    assert torch.equal(graphed.preds, eager.preds)
    worst = 0.0
    for k in eager.exp_avg:
        ma, mb = graphed.exp_avg[k], eager.exp_avg[k]
        if float(mb.abs().max()) == 0.0:
            assert float(ma.abs().max()) == 0.0, k
            continue
        worst = max(worst, relerr(ma, mb))
        assert relerr(ma, mb) < 2e-4, (k, relerr(ma, mb))
    observe(f"engine capture vs eager [{name} {prec}] gradients (rel to max)", worst, 2e-4)
    assert R.grads_cleared(graphed) and R.grads_cleared(eager)
