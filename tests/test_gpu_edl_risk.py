"""The evidential heads' cross-entropy risk, annealed KL term and epoch means of the uncertainties on the GPU (-m gpu):
m2m_heads_edl_risk through runtime.heads_edl, engine.AVMnistUQEngine with its three cfg keys and set_epoch, the epoch feed's
uncertainty sums and models.AVMnistMixerMultiLossUQ, against the float64 restatement of tests/edl_risk_ref.py.

Bars are the project's: float tensors at leaf_ref.FP32_REL (1e-4) of the tensor's max, losses and kl_out at 1e-4 x max(1, |value|),
the uncertainty at tests/test_gpu_edl.py's 1e-4 absolute; the reference is given the kernel's own gate and predictions are held
where the float64 reference is decided (tests/edl_ref.py's docstring; at most 1 % of a case's decisions excluded: the seeds of
edl_risk_ref.risk_inputs).  Engine bars are those of tests/test_gpu_engine_envelope.py (BARS, LR), unchanged.  Observed maxima are
recorded (conftest.observe)."""
import pytest
import torch

import edl_ref as E
import edl_risk_ref as RR
import engine_cases as EC
import engine_ref as R
import gen_util as G
import leaf_ref as LR
from conftest import observe
from test_gpu_edl import SENT, U_BAR, check_forward, check_grads, err, rel, slot_sums, model_cfg, own_rows, LOSS_KEYS, UQ_KEYS
from test_gpu_engine_envelope import BARS, LR as LRATE, PARAM_SEED
from test_gpu_two_stage import Calls

pytestmark = pytest.mark.gpu

BAR = LR.FP32_REL
LAMBDAS = (None, 1.0, 0.3)            # no KL term at all (kl_coef NULL), lambda = 1, lambda = 0.3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from m2_mixer_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


# ---- the leaf -------------------------------------------------------------------------------------------------------------------
def run_risk(case, inp, dev, risk, lam, training=True, zero_losses=True, gpart=None, coef_by_value=None, kl_fill=SENT, old_entry=False):
    """One call of m2m_heads_edl_risk (old_entry: m2m_heads_edl) on the case; returns the outputs and the gradient buffers."""
    from m2_mixer_amd import _lib as L
    from m2_mixer_amd.runtime import heads_edl
    B, D, K, nh = case["B"], case["D"], case["K"], len(case["forms"])
    use_gpart = case["gpart"] if gpart is None else gpart
    tiles = L.lib().m2m_heads_part_tiles(B)
    slots = torch.full((nh, tiles, L.SPLIT_GPART), SENT, device=dev) if use_gpart else None
    fill = SENT if (use_gpart or not training) else 0.0           # atomics add onto zero; untouched buffers keep the sentinel
    hd = []
    for h, f in enumerate(case["forms"]):
        d = dict(w=inp["ws"][h].to(dev), b=inp["bs"][h].to(dev), g_w=torch.full((K, D), fill, device=dev),
                 g_b=torch.full((K,), fill, device=dev), d_pooled=torch.full((B, D), SENT, device=dev) if training else None,
                 weight=(coef_by_value or case["coef"])[h])
        if f == "p":
            d["pooled"] = inp["xs"][h].to(dev).contiguous()
        else:
            buf = inp["bufs"][h].to(dev).contiguous()
            d["tokens"] = (buf, f[1], buf.shape[1])
        if slots is not None:
            d["g_part"] = slots[h]
        hd.append(d)
    weights = torch.tensor(case["coef"], dtype=torch.float32, device=dev) if case["dev_weights"] else None
    preds = torch.full((nh, B), -7, dtype=torch.int32, device=dev)
    combined = preds[nh - 1] if case["alias"] else torch.full((B,), -7, dtype=torch.int32, device=dev)
    out = (torch.full((nh, B, K), SENT, device=dev), torch.full((nh + 1,), SENT, device=dev), preds, torch.full((nh, B), SENT, device=dev),
           combined)
    kl_coef = None if lam is None else torch.tensor([lam], dtype=torch.float32, device=dev)
    kl_out = None if lam is None else torch.full((nh,), kl_fill, device=dev)
    extra = {} if old_entry else dict(risk=risk, kl_coef=kl_coef, kl_out=kl_out)
    logits, losses, preds, unc, combined = heads_edl(hd, inp["labels"].to(dev), B, D, K, out=out, zero_losses=zero_losses, weights=weights,
                                                     **extra)
    torch.cuda.synchronize()
    return dict(logits=logits, losses=losses, preds=preds, uncertainty=unc, combined=combined, heads=hd, gpart=slots, kl=kl_out)


def reference_for(case, inp, got, risk, lam):
    """The float64 reference under the kernel's own gate, after checking that gate against the reference's own."""
    z = E._logits64(inp)
    gate = got["logits"].cpu() > 0
    clear = z.abs() > 10.0 * BAR * float(z.abs().max())
    assert torch.equal(gate[clear], (z > 0)[clear]), "the kernel's gate differs from the reference's away from 0"
    return RR.heads(inp["xs"], inp["ws"], inp["bs"], case["coef"], inp["labels"], risk=risk, lam=lam, gate=gate)


def check_kl(kind, got, ref, lam):
    if lam is None:
        assert got["kl"] is None
        return
    for h, (g, r) in enumerate(zip(LR.f64(got["kl"]).tolist(), ref["kl"].tolist())):
        assert observe(f"edl {kind} kl_out (abs / max(1, |kl|))", abs(g - r) / max(1.0, abs(r)), BAR) < BAR, (h, g, r)


_INPUTS = {}


def inputs_of(case):
    if case["name"] not in _INPUTS:
        _INPUTS[case["name"]] = RR.risk_inputs(case)
    return _INPUTS[case["name"]]


@pytest.mark.parametrize("lam", LAMBDAS, ids=lambda l: "nokl" if l is None else f"lam{l}")
@pytest.mark.parametrize("risk", RR.RISKS)
@pytest.mark.parametrize("case", RR.RISK_CASES, ids=lambda c: c["name"])
def test_heads_edl_risk_vs_float64(case, risk, lam, dev):
    """Every output of one training call against float64.  Cases with device weights pass a wrong by-value coefficient, which
    must be ignored.  Slot cases: the same call in the atomic form gives the same logits, d_pooled and predictions bit for bit and
    the same weight gradients (the slots summed on the host; 1e-5 of the tensor's max: another order of the same tile sums)."""
    inp = inputs_of(case)
    wrong = [99.0] * len(case["forms"]) if case["dev_weights"] else None
    got = run_risk(case, inp, dev, risk, lam, coef_by_value=wrong)
    ref = reference_for(case, inp, got, risk, lam)
    kind = f"risk {risk}" + ("" if lam is None else " + kl") + (" scale50" if case["scale"] != 1.0 else "")
    check_forward(kind, case, got, ref)
    check_kl(kind, got, ref, lam)
    check_grads(kind, got, ref, case)
    if case["gpart"]:
        atom = run_risk(case, inp, dev, risk, lam, coef_by_value=wrong, gpart=False)
        assert torch.equal(atom["logits"], got["logits"]) and torch.equal(atom["preds"], got["preds"])
        for h, hd in enumerate(atom["heads"]):
            g_w, g_b = slot_sums(got, h, case["K"], case["D"])
            assert rel(hd["g_w"], g_w) < 1e-5 and rel(hd["g_b"], g_b) < 1e-5, h
            assert torch.equal(hd["d_pooled"], got["heads"][h]["d_pooled"])


@pytest.mark.parametrize("risk", RR.RISKS)
@pytest.mark.parametrize("name", ["D64 B5 K10 tokens", "D128 B65 K32 scale50"])
def test_evaluation_call_changes_nothing_else(name, risk, dev):
    """d_pooled == NULL: the same logits, losses' reference, predictions, uncertainties, combination and kl_out; no gradient buffer
    and no slot written."""
    case = next(c for c in RR.RISK_CASES if c["name"] == name)
    inp = inputs_of(case)
    train, ev = run_risk(case, inp, dev, risk, 0.3), run_risk(case, inp, dev, risk, 0.3, training=False)
    for k in ("logits", "preds", "uncertainty", "combined"):
        assert torch.equal(train[k], ev[k]), k
    ref = reference_for(case, inp, ev, risk, 0.3)
    check_forward(f"risk {risk} eval", case, ev, ref)
    check_kl(f"risk {risk} eval", ev, ref, 0.3)
    for hd in ev["heads"]:
        assert bool((hd["g_w"] == SENT).all()) and bool((hd["g_b"] == SENT).all())
    if ev["gpart"] is not None:
        assert bool((ev["gpart"] == SENT).all())


def same_call(a, b, grads=True):
    for k in ("logits", "losses", "preds", "uncertainty", "combined"):
        assert torch.equal(a[k], b[k]), k
    for ha, hb in zip(a["heads"], b["heads"]):
        for k in ("d_pooled",) + (("g_w", "g_b") if grads else ()):
            assert torch.equal(ha[k], hb[k]), k
    if a["gpart"] is not None:
        assert torch.equal(a["gpart"], b["gpart"])


@pytest.mark.parametrize("name", ["D32 B1 K2", "D64 B5 K10 tokens", "D128 B65 K32"])
def test_old_entry_equals_the_new_one_with_mse_and_no_kl_bit_for_bit(name, dev):
    """m2m_heads_edl forwards with (MSE, NULL, NULL).  Up to two sample tiles per head every sum is ordered (two atomic adds onto
    zero commute) and everything is compared; at B = 65 (five tiles) the losses and the atomically added weight gradients are not."""
    case = next(c for c in RR.RISK_CASES if c["name"] == name)
    inp = inputs_of(case)
    old, new = run_risk(case, inp, dev, "mse", None, old_entry=True), run_risk(case, inp, dev, "mse", None)
    few = case["B"] <= 8
    if not few:
        old["losses"], new["losses"] = old["losses"][:0], new["losses"][:0]
    same_call(old, new, grads=few)


@pytest.mark.parametrize("risk", RR.RISKS)
@pytest.mark.parametrize("name", ["D64 B5 K10 tokens", "D64 B5 K10 tokens scale50"])
def test_lambda_zero_equals_no_kl_bit_for_bit_and_writes_no_kl(name, risk, dev):
    """kl_coef -> 0.0f takes the branch round all KL arithmetic: the kl_coef == NULL result bit for bit; kl_out is cleared with the
    losses (exactly 0) and, with zero_losses = 0, not written at all."""
    case = next(c for c in RR.RISK_CASES if c["name"] == name)
    inp = inputs_of(case)
    none, zero = run_risk(case, inp, dev, risk, None), run_risk(case, inp, dev, risk, 0.0)
    same_call(none, zero)
    assert bool((zero["kl"] == 0.0).all())
    kept = run_risk(case, inp, dev, risk, 0.0, zero_losses=False)
    assert bool((kept["kl"] == SENT).all())
    assert torch.equal(kept["logits"], none["logits"])
    # lambda != 0 with zero_losses = 0 adds onto what kl_out held, as the losses do
    add = run_risk(case, inp, dev, risk, 0.3, zero_losses=False, kl_fill=5.0)
    ref = reference_for(case, inp, add, risk, 0.3)
    for g, r in zip(LR.f64(add["kl"]).tolist(), ref["kl"].tolist()):
        assert abs(g - 5.0 - r) / max(1.0, abs(r)) < BAR


def test_a_bad_risk_returns_minus_one_and_launches_nothing(dev):
    from m2_mixer_amd import _lib as L
    from m2_mixer_amd.runtime import _head_array
    B, D, K = 5, 64, 10
    outs = dict(g_w=torch.full((K, D), SENT, device=dev), g_b=torch.full((K,), SENT, device=dev), d_pooled=torch.full((B, D), SENT, device=dev),
                logits=torch.full((1, B, K), SENT, device=dev), losses=torch.full((2,), SENT, device=dev),
                uncertainty=torch.full((1, B), SENT, device=dev), kl=torch.full((1,), SENT, device=dev),
                preds=torch.full((1, B), -7, dtype=torch.int32, device=dev), combined=torch.full((B,), -7, dtype=torch.int32, device=dev))
    head = dict(pooled=torch.randn(B, D, device=dev), w=torch.randn(K, D, device=dev), b=torch.randn(K, device=dev), g_w=outs["g_w"],
                g_b=outs["g_b"], d_pooled=outs["d_pooled"], weight=1.0)
    arr = _head_array([head])
    lab = torch.zeros(B, dtype=torch.int64, device=dev)
    lam = torch.ones(1, device=dev)
    for risk, kl_coef in ((2, lam.data_ptr()), (-1, 0), (0, 0)):              # (the last: kl_out without kl_coef)
        rc = L.lib().m2m_heads_edl_risk(arr, 1, lab.data_ptr(), B, D, K, outs["logits"].data_ptr(), outs["losses"].data_ptr(),
                                        outs["preds"].data_ptr(), outs["uncertainty"].data_ptr(), outs["combined"].data_ptr(), 1, 0,
                                        risk, kl_coef, outs["kl"].data_ptr(), L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == -1 and len(L.lib().m2m_last_error()) > 0
        for k, t in outs.items():
            assert bool((t == (-7 if k in ("preds", "combined") else SENT)).all()), (risk, k)


# ---- the engine -----------------------------------------------------------------------------------------------------------------
# the smallest AV-MNIST configuration of tests/engine_cases.py (11297 parameters; of the three cases that share it, the smallest batch)
_BASE = next(c for c in EC.CASES if c.name == "av_fusion_two_groups_b19_d32_gen")
KEYS = dict(edl_loss="ce", kl_weight=1.0, annealing_step=10)
CASE = E.UQCase("uq_" + _BASE.name, "avmnist", dict(_BASE.cfg, **KEYS), _BASE.B, _BASE.p, {})
_PARAMS, _BATCHES = [], []


def params_of():
    if not _PARAMS:
        _PARAMS.append(G.make_params(R.case_shapes(CASE), PARAM_SEED))
    return _PARAMS[0]


def batches():
    if not _BATCHES:
        _BATCHES.extend((R.case_batch(CASE, 101), R.case_batch(CASE, 102)))
    return _BATCHES


def build(prec, dev, cfg=None, **kw):
    from m2_mixer_amd.engine import AVMnistUQEngine
    eng = AVMnistUQEngine(CASE.cfg if cfg is None else cfg, CASE.B, device=dev, precision=prec, lr=LRATE, init=False, **kw)
    eng.load_state_dict(params_of())
    return eng


def snapshot(eng, grads=True):
    out = dict(logits=eng.logits.clone(), losses=eng.losses.clone(), preds=eng.preds.clone(), uncertainty=eng.uncertainty.clone(),
               kl=eng.kl.clone(), own=own_rows(eng))
    if grads:
        out["grads"] = {k: v.clone() for k, v in eng.grads.items()}
    return out


class Holder:
    """Collects the misses of one engine comparison (test_gpu_edl's `hold`), so that one failure reports them all."""

    def __init__(self, kind, bar):
        self.kind, self.bar, self.bad = kind, bar, []

    def hold(self, what, value, tol, name):
        observe(f"{self.kind} {what}", value, tol)
        if not value < tol:
            self.bad.append(f"{name}: {value:.3e} >= {tol:.0e}")

    def forward(self, tag, got, want, kl=True):
        bar = self.bar
        self.hold("logits (abs)", err(got["logits"], want["logits"]), bar["logits"], f"{tag} logits")
        self.hold("losses (abs)", err(got["losses"], want["losses"]), bar["losses"], f"{tag} losses")
        if kl:                                                 # (at lambda = 0 the launch skips the KL arithmetic: `kl` stays 0)
            self.hold("kl (abs)", err(got["kl"], want["kl"]), bar["losses"], f"{tag} kl")
        self.hold("uncertainty (abs)", err(got["uncertainty"], want["uncertainty"]), bar["logits"], f"{tag} uncertainty")
        if not torch.equal(got["preds"], got["own"]):
            self.bad.append(f"{tag}: preds rows are not [image, audio, combined] of the engine's own logits and uncertainties")

    def grads(self, tag, got, want):
        for k, g in want["grads"].items():
            scale = float(g.abs().max())
            if k.endswith(R.NOISE_KEYS):
                floor = float(want["grads"][k[:-4] + "weight"].abs().max())
                scale = scale if scale > 1e-6 * floor else floor
            self.hold("gradients (rel to max)", err(got["grads"][k], g) / max(scale, 1e-30), self.bar["grads"], f"{tag} grad {k}")

    def params(self, got, want):
        self.hold("parameters after the update (abs)", max(err(got[k], v) for k, v in want.items() if not k.endswith(R.NOISE_KEYS)),
                  self.bar["params"], "parameters")


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_engine_two_steps_and_an_evaluation_at_epoch_0_against_float64(prec, dev):
    """edl_loss = "ce", kl_weight = 1, epoch 0: lambda = 0, the KL term is present and adds nothing (`kl` stays exactly 0).  In the
    manner of tests/test_gpu_edl.py: autograd through the oracle's logits into edl_risk_ref's loss, fed the engine's dropout masks
    and gates, then oracle.adam_step."""
    params = params_of()
    eng = build(prec, dev)
    assert eng.edl_loss == "ce" and eng.kl_weight == 1.0 and eng.annealing_step == 10 and eng.epoch == 0
    assert eng.kl_coef.tolist() == [0.0] and tuple(eng.kl.shape) == (3,)
    b1, b2 = batches()
    g1, g2 = tuple(t.to(dev) for t in b1), tuple(t.to(dev) for t in b2)
    eng.forward_backward(*g1)
    torch.cuda.synchronize()
    masks1, got1 = R.engine_masks(eng, CASE.B), snapshot(eng)
    eng.optimizer_step()
    torch.cuda.synchronize()
    cleared, p1 = R.grads_cleared(eng), {k: v.clone() for k, v in eng.params.items()}
    eng.forward_backward(*g2)
    torch.cuda.synchronize()
    masks2, got2 = R.engine_masks(eng, CASE.B), snapshot(eng)
    eng.evaluate(*g1)
    torch.cuda.synchronize()
    gotev = snapshot(eng, grads=False)

    ref = RR.UQStep(CASE, params, LRATE, risk="ce", lam=0.0)
    one = ref.step(b1, masks1, got1["logits"].cpu() > 0)
    ref_p1 = {k: v.clone() for k, v in ref.p.items()}
    two = ref.step(b2, masks2, got2["logits"].cpu() > 0)
    ev = ref.forward(b1, ref_p1, gates=gotev["logits"].cpu() > 0)
    h = Holder(f"engine uq risk {prec}", BARS[prec])
    for tag, got, want in (("step 1", got1, one), ("step 2", got2, two), ("eval", gotev, ev)):
        h.forward(tag, got, want, kl=False)
        if float(got["kl"].abs().max()) != 0.0:
            h.bad.append(f"{tag}: kl is not exactly 0 at lambda = 0")
    h.grads("step 1", got1, one)
    if prec == "fp32":
        h.grads("step 2", got2, two)                       # (bf16: the first update's sign noise, test_gpu_engine_envelope's docstring)
    h.params(p1, ref_p1)
    if not cleared:
        h.bad.append("the update left gradient elements uncleared outside the kept ranges")
    assert not h.bad, f"{CASE.name} [{prec}]: " + "; ".join(h.bad)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_a_graph_captured_at_epoch_0_follows_set_epoch(prec, dev):
    """capture() at epoch 0, set_epoch(5), replay: the step runs under lambda = 0.5 -- against the float64 step reference, and
    against an eager clone's step (forward quantities bit for bit; the losses and kl are five atomic adds per head in any order:
    1e-6 x max(1, |value|)).  The capture is kept."""
    params = params_of()
    eng = build(prec, dev)
    b1 = batches()[0]
    g1 = tuple(t.to(dev) for t in b1)
    replay = eng.capture(*g1)
    graph = eng._graph
    eng.set_epoch(5)
    assert eng._graph is graph and eng.epoch == 5 and eng.kl_lambda() == 0.5
    eager = eng.clone()
    assert eager.epoch == 5 and eager.kl_coef.data_ptr() != eng.kl_coef.data_ptr()
    torch.cuda.synchronize()
    assert eng.kl_coef.tolist() == [0.5] and eager.kl_coef.tolist() == [0.5]
    replay(*g1)
    eager.fused_step(*g1)
    torch.cuda.synchronize()
    for k in ("logits", "preds", "uncertainty"):
        assert torch.equal(getattr(eng, k), getattr(eager, k)), k
    for k in ("losses", "kl"):
        a, b = getattr(eng, k).double().cpu(), getattr(eager, k).double().cpu()
        assert float(((a - b).abs() / b.abs().clamp(min=1.0)).max()) < 1e-6, k
    assert float(eng.kl.min()) > 0.0
    got = snapshot(eng, grads=False)
    ref = RR.UQStep(CASE, params, LRATE, risk="ce", lam=RR.kl_lambda(1.0, 5, 10))
    one = ref.step(b1, R.engine_masks(eng, CASE.B), got["logits"].cpu() > 0)
    h = Holder(f"engine uq risk replay {prec}", BARS[prec])
    h.forward("replay", got, one)
    h.params({k: v.clone() for k, v in eng.params.items()}, ref.p)
    # the KL term is in the loss: lambda x kl is a visible part of every head's loss
    assert float((0.5 * one["kl"]).max()) > 10 * BARS[prec]["losses"]
    assert not h.bad, f"{CASE.name} [{prec}]: " + "; ".join(h.bad)


def test_default_cfg_engine_calls_the_old_entry_and_nothing_new(dev):
    """Without the keys, and with the keys at their defaults: m2m_heads_edl is the heads call, m2m_heads_edl_risk is never called,
    no lambda table and no kl buffer exist, and the two engines' first steps give the same forward bit for bit (what follows the
    first update carries the fusion tower's unordered atomic sums: tests/test_gpu_edl.py)."""
    base = {k: v for k, v in CASE.cfg.items() if k not in KEYS}
    plain = build("bf16", dev, cfg=base)
    keyed = build("bf16", dev, cfg=dict(base, edl_loss="mse", kl_weight=0.0, annealing_step=10))
    g1 = tuple(t.to(dev) for t in batches()[0])
    first = []
    for eng in (plain, keyed):
        assert eng.kl_coef is None and eng.kl is None
        with Calls() as calls:
            eng.train_step(*g1)
            first.append({k: getattr(eng, k).clone() for k in ("logits", "preds", "uncertainty")})
            eng.evaluate(*g1)
            eng.set_epoch(7)                                   # (nothing on the device follows it)
            eng.train_step(*g1)
        torch.cuda.synchronize()
        names = [n for n, _ in calls.seen]
        assert names.count("m2m_heads_edl") == 3 and "m2m_heads_edl_risk" not in names and "m2m_epoch_accumulate_uq" not in names
    for k in ("logits", "preds", "uncertainty"):
        assert torch.equal(first[0][k], first[1][k]), k


def test_frozen_towers_and_their_heads_are_untouched_by_a_step(dev):
    """freeze_modalities() on the ce + KL engine at lambda = 0.5: a captured stage-two step leaves every modality-tower and
    tower-head parameter bitwise unchanged and moves the fusion part."""
    eng = build("bf16", dev)
    eng.set_epoch(5)
    g1 = tuple(t.to(dev) for t in batches()[0])
    eng.train_step(*g1)
    eng.freeze_modalities()
    frozen = eng._frozen_prefixes()
    before = {k: v.clone() for k, v in eng.params.items()}
    replay = eng.capture(*g1)
    replay(*g1)
    torch.cuda.synchronize()
    moved = [k for k in before if not torch.equal(before[k], eng.params[k])]
    assert moved and not [k for k in moved if k.startswith(frozen)], [k for k in moved if k.startswith(frozen)]
    assert any(k.startswith("fusion_mixer.") for k in moved) and any(k.startswith("classifier_fusion.") for k in moved)
    assert float(eng.kl.min()) > 0.0 and bool(torch.isfinite(eng.losses).all())
    out = eng.probe(*g1)                                       # probe(), sibling() keep working
    sib = eng.sibling(3, trains=False)
    assert bool(torch.isfinite(out).all()) and sib.kl_coef.data_ptr() == eng.kl_coef.data_ptr() and sib.epoch == 5


def test_fed_epoch_reports_the_epoch_means_of_the_uncertainties(dev):
    """A split of 2 B + 3 rows, a two-step feed graph, the ragged tail through a sibling: uncertainty, uncertainty_image and
    uncertainty_audio are the means over the three steps of each step's batch mean -- against the float64 reference stepped
    through the same three batches under the engine's dropout masks, at the uncertainty bar -- and steps / samples count them."""
    from m2_mixer_amd.accumulators import EpochFeed
    from m2_mixer_amd.data import run_epoch_fed
    from m2_mixer_amd.engine import AVMnistEngine
    B, n = CASE.B, 2 * CASE.B + 3
    rows = [torch.cat(ts)[:n].contiguous() for ts in zip(*(R.case_batch(CASE, s) for s in (201, 202, 203)))]
    eng = build("fp32", dev)
    eng.set_epoch(5)
    tail = eng._tail_engines[3] = eng.sibling(3)                # (before the capture: data.prepare_tail_engine's rule)
    feed = EpochFeed([t.to(dev) for t in rows], B, dev, uncertainty=True)
    replay = eng.capture_feed(feed, steps=2)
    out = run_epoch_fed(eng, feed, replay)
    assert out["steps"] == 3 and out["samples"] == n
    ref = RR.UQStep(CASE, params_of(), LRATE, risk="ce", lam=0.5)
    means = []
    for i, (lo, hi, e) in enumerate(((0, B, eng), (B, 2 * B, eng), (2 * B, n, tail))):
        batch = tuple(t[lo:hi] for t in rows)
        masks = {name: R.tower_masks(rt, hi - lo, e.seed, i + 1) for name, rt in (("image", e.t_a), ("audio", e.t_b), ("fusion", e.t_fus))}
        case = CASE._replace(B=hi - lo)
        ref.case = case
        means.append(ref.step(batch, masks)["uncertainty"].mean(dim=1))
    want = torch.stack(means).mean(dim=0)                       # rows image, audio, fusion
    for i, k in ((2, "uncertainty"), (0, "uncertainty_image"), (1, "uncertainty_audio")):
        assert observe("fed epoch mean uncertainty (abs)", abs(out[k] - float(want[i])), U_BAR) < U_BAR, (k, out[k], float(want[i]))
    # without the switch the feed has no such sums, and an engine without the buffer refuses the switch
    plain = EpochFeed([t.to(dev) for t in rows], B, dev)
    plain.bind(eng)
    assert plain.unc_sums is None and int(plain._acc.numel()) == 2 * 4 + 3 + 2
    ce_cfg = {k: v for k, v in CASE.cfg.items() if k not in KEYS}
    with pytest.raises(RuntimeError, match="uncertainty"):
        EpochFeed([t.to(dev) for t in rows], B, dev, uncertainty=True).bind(AVMnistEngine(ce_cfg, B, device=dev, precision="fp32", lr=LRATE))


# ---- the module -----------------------------------------------------------------------------------------------------------------
def test_bound_module_trains_a_step_and_its_kl_follows_current_epoch(dev):
    from m2_mixer_amd import models as MD
    from m2_mixer_amd.engine import AVMnistUQEngine
    bar = BARS["fp32"]
    net = MD.AVMnistMixerMultiLossUQ(dict(model_cfg(CASE), **KEYS), {"lr": LRATE}).to(dev)
    net.load_state_dict(params_of())
    eng = net.bind_engine(CASE.B, precision="fp32")
    assert type(eng) is AVMnistUQEngine and (eng.edl_loss, eng.kl_weight, eng.annealing_step) == ("ce", 1.0, 10)
    b1 = batches()[0]
    batch = {"image": b1[0].to(dev), "audio": b1[1].to(dev), "label": b1[2].to(dev)}
    val0 = net.validation_step(batch)                           # epoch 0: lambda = 0
    torch.cuda.synchronize()
    sib = net._eval_siblings[CASE.B]
    assert eng.kl_coef.tolist() == [0.0] and float(sib.kl.abs().max()) == 0.0
    net.current_epoch = 5
    out = net.training_step(batch)
    torch.cuda.synchronize()
    assert set(out) == LOSS_KEYS | UQ_KEYS | {"preds", "labels"}                      # the result keys are unchanged
    assert eng.epoch == 5 and eng.kl_coef.tolist() == [0.5] and float(eng.kl.min()) > 0.0
    ref = RR.UQStep(CASE, params_of(), LRATE, risk="ce", lam=0.5)
    one = ref.step(b1, R.engine_masks(eng, CASE.B), eng.logits.cpu() > 0)
    for i, k in enumerate(("loss_image", "loss_audio", "loss_fusion", "loss")):
        assert observe("module uq risk training losses (abs)", err(out[k], one["losses"][i]), bar["losses"]) < bar["losses"], k
    assert observe("module uq risk kl (abs)", err(eng.kl, one["kl"]), bar["losses"]) < bar["losses"]
    net.current_epoch = 20                                      # past annealing_step: lambda = kl_weight
    val = net.validation_step(batch)
    torch.cuda.synchronize()
    assert eng.kl_coef.tolist() == [1.0] and float(sib.kl.min()) > 0.0
    assert set(val) == set(val0)
    ev = ref.forward(b1, gates=torch.stack([val["image_logits"], val["audio_logits"], val["logits"]]).cpu() > 0)
    want = ev["losses"][:3] + (1.0 - 0.5) * ev["kl"]            # (the reference above carries lambda = 0.5)
    for i, k in enumerate(("loss_image", "loss_audio", "loss_fusion")):
        assert observe("module uq risk validation losses (abs)", err(val[k], want[i]), bar["losses"]) < bar["losses"], k
