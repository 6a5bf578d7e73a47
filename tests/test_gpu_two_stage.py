"""Stage two of the two-stage training on the fused engines (-m gpu): every case of tests/engine_cases.py, in fp32 and bf16.

Per case: two stage-one steps, engine.freeze_modalities(), two stage-two steps (a fused_step, then forward_backward +
optimizer_step), an evaluation -- against the float64 reference (engine_ref.Step twice, then stage_ref.FrozenStep twice, fed the
kernels' own dropout masks where p > 0) at the bars tests/test_gpu_engine_envelope.py uses for the same case and precision
(logits and losses absolute 1e-3 / 2e-2, parameters 2e-3 / 1e-2 with the rounding-level key left out; its LR and parameter
seed).  The flat ranges of the frozen keys in flat_p, flat_m and flat_v must be torch.equal to their snapshot at the freeze
after every stage-two step; losses[3] == losses[2] in stage two; the evaluation afterwards returns the weighted total loss.

Two-tower cases: every call into the library during the stage-two steps is recorded (the functions of the loaded CDLL are wrapped
as scripts/launch_trace.py wraps them): no backward of a modality tower, no embedding weight gradient, weight-gradient calls of
one tower and no embedding, Adam inside the trainable ranges only, no re-pack but the fusion tower's.

One case (AV-MNIST S, B = 13) goes through capture() after the freeze, with a training sibling(B - 3) built before it.

The fusion functions other than ConcatFusion (AV-MNIST S, dropout 0, B = 6; tests/fusion_ref.py): the fusion's own backward
still runs in stage two and a gated unit's parameters keep training, against the float64 reference at the same bars."""
import pytest
import torch

import engine_ref as R
import fusion_ref as FR
import gen_util as G
import stage_ref as S
from conftest import observe
from engine_cases import CASES, Case

pytestmark = pytest.mark.gpu

LR = 2e-3                                                # tests/test_gpu_engine_envelope.py
PARAM_SEED = 31
BARS = {"fp32": dict(logits=1e-3, losses=1e-3, params=2e-3), "bf16": dict(logits=2e-2, losses=2e-2, params=1e-2)}
AV_S = Case("avmnist_S_b13", "avmnist", dict(G.AVMNIST["S"]), 13, G.AVMNIST["S"]["dropout"], {})

_REFS = {}          # case name -> (masks of the four steps, reference results): computed once, shared by the two precisions


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


masks_equal = R.masks_equal


def reference(case, params, batches, masks):
    """Step, Step, FrozenStep, FrozenStep and an evaluation of the first batch with the final parameters (kept once computed;
    recomputed only if a precision drew other masks)."""
    hit = _REFS.get(case.name)
    if hit is not None and all(masks_equal(a, b) for a, b in zip(hit[0], masks)):
        return hit[1]
    one = R.Step(case, params, LR)
    outs = [one.step(batches[0], masks[0]), one.step(batches[1], masks[1])]
    two = S.FrozenStep(one)
    p2 = {k: v.clone() for k, v in two.p.items()}
    outs += [two.step(batches[2], masks[2]), two.step(batches[3], masks[3])]
    ref = dict(outs=outs, p2=p2, p4={k: v.clone() for k, v in two.p.items()}, ev=two.forward(batches[0]))
    _REFS[case.name] = (masks, ref)
    return ref


def frozen_ranges(eng, case):
    return S.flat_ranges(eng.shapes, {k for k in eng.shapes if S.is_frozen(case, k)})


def snapshot(eng, ranges):
    return [[t[lo:hi].clone() for lo, hi in ranges] for t in (eng.flat_p, eng.flat_m, eng.flat_v)]


def untouched(eng, ranges, snap):
    return all(torch.equal(t[lo:hi], s) for t, row in zip((eng.flat_p, eng.flat_m, eng.flat_v), snap) for (lo, hi), s in zip(ranges, row))


class Calls:
    """Every call into the loaded library while active: (symbol, arguments)."""

    def __init__(self):
        from m2_mixer_amd import _lib as L
        self.lib, self.names, self.seen, self.orig = L.lib(), list(L.SIGNATURES), [], {}

    def __enter__(self):
        for name in self.names:
            fn = self.orig[name] = getattr(self.lib, name)
            setattr(self.lib, name, lambda *a, _n=name, _f=fn: (self.seen.append((_n, a)), _f(*a))[1])
        return self

    def __exit__(self, *exc):
        for name, fn in self.orig.items():
            setattr(self.lib, name, fn)


def check_stage_two_calls(eng, seen, nsteps):
    """The stage-two launch list of a two-tower engine."""
    names = [n for n, _ in seen]
    fus = eng.t_fus.desc
    desc_of = lambda a: getattr(a[0], "_obj", None)
    assert "m2m_towers_backward" not in names and "m2m_tower_backward_heads" not in names
    back = [a for n, a in seen if n == "m2m_tower_backward"]
    assert len(back) == nsteps and all(desc_of(a) is fus for a in back), "one backward per step: the fusion tower's"
    assert "m2m_embed_wgrad" not in names and "m2m_embeds_wgrad" not in names
    single = [a for n, a in seen if n == "m2m_tower_wgrad"]
    grouped = [a for n, a in seen if n in ("m2m_towers_wgrad", "m2m_towers_wgrad_heads", "m2m_towers_wgrad_tail")]
    assert len(single) + len(grouped) == nsteps, "one weight-gradient call per step"
    assert all(desc_of(a) is fus for a in single)
    assert all(a[2] == 1 and a[7] == 0 for a in grouped), "one tower, no embeddings"
    assert "m2m_adam_pack_all" not in names and "m2m_pack_all" not in names and "m2m_pack_embed" not in names
    assert all(desc_of(a) is fus for n, a in seen if n == "m2m_pack_tower")
    adam = [(n, a) for n, a in seen if n in ("m2m_adam_step", "m2m_adam_step_ranges", "m2m_adam_step_bf16")]
    assert len(adam) == nsteps * len(eng._trainable)
    base = eng.flat_p.data_ptr()
    for name, a in adam:
        count = a[4] if name == "m2m_adam_step" else a[5]      # (_ranges / _bf16 carry the bf16 gradient pointer before the moments)
        lo = (a[0] - base) // 4
        assert (lo, lo + count) in eng._trainable, (lo, count, eng._trainable)
    for gone in ("m2m_towers_forward_embeds",):
        assert gone not in names


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_stage_two_against_float64(case, prec, dev):
    params = G.make_params(R.case_shapes(case), PARAM_SEED)
    eng = build(case, prec, dev, params)
    two_tower = case.engine != "mimic"
    masked = case.p > 0
    host = [R.case_batch(case, 101 + i) for i in range(4)]
    gpu = [tuple(t.to(dev) for t in b) for b in host]
    ranges = frozen_ranges(eng, case)
    got, masks, bad = [], [], []

    def record():
        torch.cuda.synchronize()
        masks.append(R.engine_masks(eng, case.B) if masked else None)
        got.append(dict(logits=eng.logits.clone(), losses=eng.losses.clone()))

    for b in gpu[:2]:                                    # ---- stage one
        eng.fused_step(*b)
        record()
    eng.freeze_modalities()
    assert eng._graph is None and eng._frozen
    torch.cuda.synchronize()
    snap = snapshot(eng, ranges)
    trainable_before = {k: v.clone() for k, v in eng.params.items() if not S.is_frozen(case, k)}
    with Calls() as calls:                               # ---- stage two
        eng.fused_step(*gpu[2])
        record()
        if not untouched(eng, ranges, snap):
            bad.append("a frozen range changed in the fused stage-two step")
        eng.forward_backward(*gpu[3])
        record()
        eng.optimizer_step()
        torch.cuda.synchronize()
    if not untouched(eng, ranges, snap):
        bad.append("a frozen range changed in forward_backward + optimizer_step")
    if two_tower:
        check_stage_two_calls(eng, calls.seen, 2)
    counters = (float(eng.adam_state[0]), int(eng.drop_step[0]))
    p4 = {k: v.clone() for k, v in eng.params.items()}
    eng.evaluate(*gpu[0])
    torch.cuda.synchronize()
    gotev = dict(logits=eng.logits.clone(), losses=eng.losses.clone())

    ref = reference(case, params, host, masks)
    bar, kind = BARS[prec], f"stage two {case.engine} {prec}"

    def hold(what, value, tol, name):
        observe(f"{kind} {what}", value, tol)
        if not value < tol:
            bad.append(f"{name}: {value:.3e} >= {tol:.0e}")

    for i, (g, w) in enumerate(zip(got, ref["outs"])):
        hold("logits (abs)", err(g["logits"], w["logits"]), bar["logits"], f"step {i + 1} logits")
        hold("losses (abs)", err(g["losses"], w["losses"]), bar["losses"], f"step {i + 1} losses")
    for i in (2, 3):
        l = got[i]["losses"]
        if float(l[3]) != float(l[2]):
            bad.append(f"step {i + 1}: losses[3] = {float(l[3])!r} is not losses[2] = {float(l[2])!r}")
    hold("logits (abs)", err(gotev["logits"], ref["ev"]["logits"]), bar["logits"], "eval logits")
    hold("losses (abs)", err(gotev["losses"], ref["ev"]["losses"]), bar["losses"], "eval losses (the weighted total)")
    hold("trainable parameters after stage two (abs)",
         max(err(p4[k], v) for k, v in ref["p4"].items() if not S.is_frozen(case, k) and not k.endswith(R.NOISE_KEYS)),
         bar["params"], "trainable parameters")
    for k, v in trainable_before.items():
        if not k.endswith(R.NOISE_KEYS) and torch.equal(p4[k], v):
            bad.append(f"trainable {k} did not move in stage two")
    if counters != (4.0, 4):
        bad.append(f"step counters (Adam, dropout) after four steps: {counters}")
    assert not bad, f"{case.name} [{prec}]: " + "; ".join(bad)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_captured_stage_two_and_a_sibling_built_before_the_freeze(prec, dev):
    case = AV_S
    params = G.make_params(R.case_shapes(case), PARAM_SEED)
    eng = build(case, prec, dev, params)
    sib = eng.sibling(case.B - 3)                        # a training sibling from stage one
    host = [R.case_batch(case, 201 + i) for i in range(4)]
    gpu = [tuple(t.to(dev) for t in b) for b in host]
    ranges = frozen_ranges(eng, case)
    got, masks = [], []

    def record():
        torch.cuda.synchronize()
        masks.append(R.engine_masks(eng, case.B))
        got.append(dict(logits=eng.logits.clone(), losses=eng.losses.clone()))

    replay = eng.capture(*gpu[0])
    for b in gpu[:2]:
        replay(*b)
        record()
    assert eng._graph is not None
    eng.freeze_modalities()
    assert eng._graph is None, "freeze_modalities drops the captured graph as release_capture does"
    assert sib._frozen, "the stage is the family's"
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
        assert float(eng.losses[3]) == float(eng.losses[2])
    assert untouched(eng, ranges, snap)
    p4 = {k: v.clone() for k, v in eng.params.items()}
    ref = reference(case._replace(name=case.name + "_captured"), params, host, masks)
    bar = BARS[prec]
    for i, (g, w) in enumerate(zip(got, ref["outs"])):
        assert err(g["logits"], w["logits"]) < bar["logits"], f"step {i + 1} logits"
        assert err(g["losses"], w["losses"]) < bar["losses"], f"step {i + 1} losses"
    worst = max(err(p4[k], v) for k, v in ref["p4"].items() if not S.is_frozen(case, k) and not k.endswith(R.NOISE_KEYS))
    observe(f"stage two captured avmnist {prec} trainable parameters (abs)", worst, bar["params"])
    assert worst < bar["params"]
    # the sibling's stage-two step: its own batch size, the family's frozen ranges
    small = tuple(t[:case.B - 3].contiguous() for t in gpu[3])
    sib.pack()
    sib.train_step(*small)
    eng.pack()
    torch.cuda.synchronize()
    assert untouched(eng, ranges, snap), "the sibling's step wrote a frozen range"
    assert float(sib.losses[3]) == float(sib.losses[2]) and float(eng.adam_state[0]) == 5.0
    assert not torch.equal(eng.params["classifier_fusion.classifer.weight"], p4["classifier_fusion.classifer.weight"])
    # a sibling built AFTER the freeze is in stage two as well
    eng.release_capture()                                # (sibling()'s rule: build training siblings before capture(), or capture again)
    late = eng.sibling(case.B - 5)
    assert late._frozen and late._trainable == eng._trainable
    late.pack()
    late.train_step(*(t[:case.B - 5].contiguous() for t in gpu[2]))
    torch.cuda.synchronize()
    assert untouched(eng, ranges, snap) and float(late.losses[3]) == float(late.losses[2])


def test_freeze_is_refused_with_the_fused_heads_launch(dev):
    case = AV_S
    eng = build(case, "bf16", dev, G.make_params(R.case_shapes(case), PARAM_SEED))
    eng._loss_weight_group["fused_heads"] = True         # what M2M_FUSED_HEADS=1 sets where that launch exists
    with pytest.raises(RuntimeError, match="M2M_FUSED_HEADS"):
        eng.freeze_modalities()
    assert not eng._frozen


def fusion_stage_two_step(ref, case, xa, xb, y):
    """fusion_ref.Step.step in stage two: the loss is losses[2], only the trainable keys are updated, the step count goes on."""
    leaves = {k: v.clone().requires_grad_(True) for k, v in ref.p.items()}
    out = FR.two_tower_forward(ref.task, xa.double(), xb.double(), y, leaves, ref.c, ref.pw)
    out["losses"][2].backward()
    ref.t += 1
    for k, leaf in leaves.items():
        if S.is_frozen(case, k):
            continue
        g = leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)
        m, v = ref.m.get(k, torch.zeros_like(g)), ref.v.get(k, torch.zeros_like(g))
        ref.p[k], ref.m[k], ref.v[k] = FR.O.adam_step(ref.p[k], g, m, v, ref.t, ref.lr)
    losses = out["losses"].detach().clone()
    losses[3] = losses[2]
    return {"logits": out["logits"].detach(), "losses": losses}


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("fusion", FR.FUSIONS)
def test_stage_two_with_a_fusion_function(fusion, prec, dev):
    from m2_mixer_amd.engine import AVMnistEngine
    c = dict(FR.with_fusion(G.AVMNIST["S"], fusion), dropout=0.0)
    case = Case("avmnist_S_" + fusion, "avmnist", c, 6, 0.0, {})
    params = dict(G.make_params(FR.two_tower_shapes("avmnist", c), 21))
    eng = AVMnistEngine(c, case.B, device=dev, precision=prec, lr=LR, init=False)
    eng.load_state_dict(params)
    assert list(eng.shapes) == list(params)
    ref = FR.Step("avmnist", c, params, LR)
    host = [G.avmnist_batch(case.B, 100 + i, c) for i in range(3)]
    gpu = [tuple(t.to(dev) for t in b) for b in host]
    bar = BARS[prec]
    eng.fused_step(*gpu[0])
    ref.step(*host[0])
    eng.freeze_modalities()
    torch.cuda.synchronize()
    ranges = frozen_ranges(eng, case)
    snap = snapshot(eng, ranges)
    before = {k: v.clone() for k, v in eng.params.items()}
    with Calls() as calls:
        for b, h in zip(gpu[1:], host[1:]):
            eng.fused_step(*b)
            torch.cuda.synchronize()
            want = fusion_stage_two_step(ref, case, *h)
            assert err(eng.logits, want["logits"]) < bar["logits"] and err(eng.losses, want["losses"]) < bar["losses"]
            assert float(eng.losses[3]) == float(eng.losses[2])
    check_stage_two_calls(eng, calls.seen, 2)
    names = [n for n, _ in calls.seen]
    if fusion == "BiModalGatedUnit":
        assert names.count("m2m_gate_backward") == 2 and names.count("m2m_gate_wgrad") == 2
    elif fusion != "SumFusion":
        assert names.count("m2m_fusion_backward") == 2
    assert untouched(eng, ranges, snap)
    worst = max(err(eng.params[k], v) for k, v in ref.p.items() if not S.is_frozen(case, k) and not k.endswith(R.NOISE_KEYS))
    observe(f"stage two fusion {fusion} {prec} trainable parameters (abs)", worst, bar["params"])
    assert worst < bar["params"]
    for k in eng.params:
        if k.startswith("fusion_function."):
            assert not torch.equal(eng.params[k], before[k]), f"{k} (trainable in stage two) did not move"
