"""The evidential (EDL) uncertainty model on the GPU (-m gpu): m2m_heads_edl called directly through runtime.heads_edl,
engine.AVMnistUQEngine and models.AVMnistMixerMultiLossUQ, against the float64 restatement of tests/edl_ref.py.

Leaf bars are leaf_ref's: float tensors at FP32_REL (1e-4) of the tensor's max, losses at 1e-4 x max(1, |loss|), the uncertainty
(a number in (0, 1]) at 1e-4 absolute.  The reference is given the kernel's own gate (its logits > 0: edl_ref's docstring), and
the kernel's gate must equal the reference's wherever |z_ref| exceeds 10x the logits bar.  Predictions are held where the float64
reference is decided, and at most 1 % of a case's decisions may be excluded (a property of the inputs: tests/test_host_edl.py).

Engine bars are those of tests/test_gpu_engine_envelope.py (BARS, LR), unchanged; the observed maxima are recorded
(conftest.observe)."""
import pytest
import torch

import edl_ref as E
import engine_ref as R
import gen_util as G
import leaf_ref as LR
from conftest import observe
from test_gpu_engine_envelope import BARS, LR as LRATE, PARAM_SEED

pytestmark = pytest.mark.gpu

BAR = LR.FP32_REL
U_BAR = 1e-4
SENT = -777.25            # sentinel of buffers a call must not write


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from m2_mixer_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def rel(got, ref):
    ref = LR.f64(ref)
    return float((LR.f64(got) - ref).abs().max()) / (float(ref.abs().max()) + 1e-300)


def err(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


# ---- the leaf -------------------------------------------------------------------------------------------------------------------
def run_edl(case, inp, dev, training=True, zero_losses=True, losses_fill=None, coef_by_value=None, gpart=None):
    """One call of m2m_heads_edl on the case; returns the outputs and the gradient buffers."""
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
    out = (torch.full((nh, B, K), SENT, device=dev), torch.full((nh + 1,), float(SENT if losses_fill is None else losses_fill), device=dev),
           preds, torch.full((nh, B), SENT, device=dev), combined)
    logits, losses, preds, unc, combined = heads_edl(hd, inp["labels"].to(dev), B, D, K, out=out, zero_losses=zero_losses, weights=weights)
    torch.cuda.synchronize()
    return dict(logits=logits, losses=losses, preds=preds, uncertainty=unc, combined=combined, heads=hd, gpart=slots)


def reference_for(case, inp, got):
    """The float64 reference under the kernel's own gate, after checking that gate against the reference's own."""
    plain = E.heads(inp["xs"], inp["ws"], inp["bs"], case["coef"], inp["labels"])
    gate = got["logits"].cpu() > 0
    z = plain["logits"]
    clear = z.abs() > 10.0 * BAR * float(z.abs().max())
    assert torch.equal(gate[clear], (z > 0)[clear]), "the kernel's gate differs from the reference's away from 0"
    return E.heads(inp["xs"], inp["ws"], inp["bs"], case["coef"], inp["labels"], gate=gate)


def check_forward(kind, case, got, ref, losses_offset=0.0):
    nh = len(case["forms"])
    assert observe(f"edl {kind} logits (rel to max)", rel(got["logits"], ref["logits"]), BAR) < BAR
    for i, (g, r) in enumerate(zip(LR.f64(got["losses"]).tolist(), ref["losses"].tolist())):
        assert observe(f"edl {kind} losses (abs / max(1, |loss|))", abs(g - losses_offset - r) / max(1.0, abs(r)), BAR) < BAR, (i, g, r)
    assert observe(f"edl {kind} uncertainty (abs)", err(got["uncertainty"], ref["uncertainty"]), U_BAR) < U_BAR
    hok, cok = ref["head_decided"], ref["combined_decided"]
    assert float((~hok).float().mean()) < LR.PRED_EXCLUDED_MAX and float((~cok).float().mean()) < LR.PRED_EXCLUDED_MAX
    rows = nh - 1 if case["alias"] else nh                          # aliased: the last head's row holds the combined prediction
    assert torch.equal(got["preds"].cpu().long()[:rows][hok[:rows]], ref["preds"][:rows][hok[:rows]])
    assert torch.equal(got["combined"].cpu().long()[cok], ref["combined"][cok])
    if case["alias"]:
        assert got["combined"].data_ptr() == got["preds"][nh - 1].data_ptr()


def slot_sums(got, h, K, D):
    slots = got["gpart"][h].double().cpu()
    assert float(slots[:, K * D + K:K * D + K + 2].abs().max()) == 0.0                # the two trailing slot entries
    return slots[:, :K * D].sum(0).view(K, D), slots[:, K * D:K * D + K].sum(0)


def check_grads(kind, got, ref, case):
    K, D = case["K"], case["D"]
    for h, hd in enumerate(got["heads"]):
        assert observe(f"edl {kind} d_pooled (rel to max)", rel(hd["d_pooled"], ref["d_pooled"][h]), BAR) < BAR, h
        if got["gpart"] is not None:
            g_w, g_b = slot_sums(got, h, K, D)
            assert bool((hd["g_w"] == SENT).all()) and bool((hd["g_b"] == SENT).all())    # g_w / g_b themselves untouched
        else:
            g_w, g_b = hd["g_w"], hd["g_b"]
        assert observe(f"edl {kind} g_w (rel to max)", rel(g_w, ref["g_w"][h]), BAR) < BAR, h
        assert observe(f"edl {kind} g_b (rel to max)", rel(g_b, ref["g_b"][h]), BAR) < BAR, h


@pytest.mark.parametrize("case", E.EDL_CASES, ids=lambda c: c["name"])
def test_heads_edl_vs_float64(case, dev):
    """Every output of one training call against float64.  Cases with device weights pass a wrong by-value coefficient, which
    must be ignored.  Slot cases: the slots summed on the host also equal the atomic form of the same call (same tile sums, added
    in another order: 1e-5 of the tensor's max is a hundred times the rounding of adding six fp32 partial sums)."""
    inp = E.edl_inputs(case)
    wrong = [99.0] * len(case["forms"]) if case["dev_weights"] else None
    got = run_edl(case, inp, dev, coef_by_value=wrong)
    ref = reference_for(case, inp, got)
    check_forward("leaf", case, got, ref)
    check_grads("leaf", got, ref, case)
    if case["gpart"]:
        atom = run_edl(case, inp, dev, coef_by_value=wrong, gpart=False)
        assert torch.equal(atom["logits"], got["logits"]) and torch.equal(atom["preds"], got["preds"])
        for h, hd in enumerate(atom["heads"]):
            g_w, g_b = slot_sums(got, h, case["K"], case["D"])
            assert rel(hd["g_w"], g_w) < 1e-5 and rel(hd["g_b"], g_b) < 1e-5, h
            assert torch.equal(hd["d_pooled"], got["heads"][h]["d_pooled"])


def test_evaluation_call_changes_nothing_else(dev):
    """d_pooled == NULL: the same logits, losses, predictions, uncertainties and combination, and no gradient buffer written."""
    case = next(c for c in E.EDL_CASES if c["name"] == "D64 B65 K10 h3 tokens alias")
    inp = E.edl_inputs(case)
    train, ev = run_edl(case, inp, dev), run_edl(case, inp, dev, training=False)
    for k in ("logits", "preds", "uncertainty", "combined"):
        assert torch.equal(train[k], ev[k]), k
    check_forward("eval", case, ev, reference_for(case, inp, ev))
    for hd in ev["heads"]:
        assert bool((hd["g_w"] == SENT).all()) and bool((hd["g_b"] == SENT).all())


def exact_case(B, K, nh, D=32):
    """Zero weights and chosen biases: the logits ARE the biases, exactly."""
    return dict(name="exact", B=B, D=D, K=K, forms=["p"] * nh, coef=[1.0] * nh, gpart=False, dev_weights=False, alias=False)


def exact_inputs(case, biases, seed=5):
    gen = torch.Generator().manual_seed(seed)
    B, D, K, nh = case["B"], case["D"], case["K"], len(case["forms"])
    return dict(xs=[torch.randn(B, D, generator=gen) for _ in range(nh)], bufs=[None] * nh, ws=[torch.zeros(K, D) for _ in range(nh)],
                bs=[b.float() for b in biases], labels=torch.randint(0, K, (B,), generator=gen))


def test_all_negative_logits_give_no_evidence(dev):
    """u == 1 exactly; preds, combined, d_pooled and the weight gradients exactly 0; the loss is that of the uniform p = 1 / K."""
    case = exact_case(5, 10, 3)
    inp = exact_inputs(case, [-1.0 - 0.25 * torch.arange(10.0) - h for h in range(3)])
    got = run_edl(case, inp, dev)
    assert bool((got["uncertainty"] == 1.0).all())
    assert int(got["preds"].abs().max()) == 0 and int(got["combined"].abs().max()) == 0
    for hd in got["heads"]:
        for k in ("d_pooled", "g_w", "g_b"):
            assert float(hd[k].abs().max()) == 0.0, k
    check_forward("no evidence", case, got, reference_for(case, inp, got))


def test_one_huge_logit_among_zeros_stays_finite(dev):
    case = exact_case(5, 10, 2)
    b = torch.zeros(10)
    b[3] = 1e4
    inp = exact_inputs(case, [b, b.roll(4)])
    got = run_edl(case, inp, dev)
    for t in (got["logits"], got["losses"], got["uncertainty"]) + tuple(h[k] for h in got["heads"] for k in ("d_pooled", "g_w", "g_b")):
        assert bool(torch.isfinite(t).all())
    assert got["preds"].tolist() == [[3] * 5, [7] * 5]
    # (forward only against float64: with p = 10001 / 10010 the gradient's (y - p) - sum (y - p) p cancels to 1e-3 of its terms)
    check_forward("huge", case, got, reference_for(case, inp, got))


def test_two_heads_bit_equal_at_the_smallest_uncertainty_combine_to_zero(dev):
    """Heads 0 and 1 carry the same logits (class 3, the smaller u), head 2 has no evidence: no head is strictly least."""
    case = exact_case(4, 10, 3)
    b = torch.zeros(10)
    b[3], b[6] = 2.5, 1.0
    inp = exact_inputs(case, [b, b.clone(), -torch.ones(10)])
    got = run_edl(case, inp, dev)
    assert torch.equal(got["uncertainty"][0], got["uncertainty"][1]) and bool((got["uncertainty"][0] < got["uncertainty"][2]).all())
    assert got["preds"].tolist() == [[3] * 4, [3] * 4, [0] * 4]
    assert got["combined"].tolist() == [0] * 4
    # one head strictly least: its prediction
    inp = exact_inputs(case, [b, 0.5 * b, -torch.ones(10)])
    assert run_edl(case, inp, dev)["combined"].tolist() == [3] * 4


def test_gradients_and_losses_accumulate(dev):
    """A second call onto the same g_w / g_b doubles them (one sample tile per head: the sums are exact), and zero_losses = 0 adds
    the losses onto what the buffer held."""
    from m2_mixer_amd.runtime import heads_edl
    case = next(c for c in E.EDL_CASES if c["name"] == "D128 B4 K10 h3 alias")
    inp = E.edl_inputs(case)
    got = run_edl(case, inp, dev)
    once = [(h["g_w"].clone(), h["g_b"].clone()) for h in got["heads"]]
    heads_edl(got["heads"], inp["labels"].to(dev), case["B"], case["D"], case["K"])
    torch.cuda.synchronize()
    for (g_w, g_b), hd in zip(once, got["heads"]):
        assert float(g_w.abs().max()) > 0.0 and torch.equal(hd["g_w"], 2 * g_w) and torch.equal(hd["g_b"], 2 * g_b)
    ref = reference_for(case, inp, got)
    check_forward("accumulate", case, run_edl(case, inp, dev, zero_losses=False, losses_fill=5.0), ref, losses_offset=5.0)
    check_forward("overwrite", case, run_edl(case, inp, dev, zero_losses=True, losses_fill=5.0), ref)


@pytest.mark.parametrize("what", ["K=33", "five heads", "D=48", "B=0", "NULL uncertainty"])
def test_refusals_return_minus_one_and_launch_nothing(what, dev):
    from m2_mixer_amd import _lib as L
    B, D, K, nh = 8, 128, 10, 1
    if what == "K=33": K = 33
    if what == "five heads": nh = 5
    if what == "D=48": D = 48
    Bcall = 0 if what == "B=0" else B
    x = torch.randn(B * 256 + 8, device=dev)
    w, b = torch.randn(64, 256, device=dev), torch.randn(64, device=dev)
    outs = dict(g_w=torch.full((64, 256), SENT, device=dev), g_b=torch.full((64,), SENT, device=dev),
                d_pooled=torch.full((B, 256), SENT, device=dev), logits=torch.full((5, B, 64), SENT, device=dev),
                losses=torch.full((8,), SENT, device=dev), uncertainty=torch.full((5, B), SENT, device=dev),
                preds=torch.full((5, B), -7, dtype=torch.int32, device=dev), combined=torch.full((B,), -7, dtype=torch.int32, device=dev))
    arr = (L.Head * 5)()
    for h in range(5):
        arr[h].pooled, arr[h].w, arr[h].b = x.data_ptr(), w.data_ptr(), b.data_ptr()
        arr[h].g_w, arr[h].g_b, arr[h].d_pooled, arr[h].weight = outs["g_w"].data_ptr(), outs["g_b"].data_ptr(), outs["d_pooled"].data_ptr(), 1.0
    lab = torch.zeros(B, dtype=torch.int64, device=dev)
    unc = 0 if what == "NULL uncertainty" else outs["uncertainty"].data_ptr()
    rc = L.lib().m2m_heads_edl(arr, nh, lab.data_ptr(), Bcall, D, K, outs["logits"].data_ptr(), outs["losses"].data_ptr(),
                               outs["preds"].data_ptr(), unc, outs["combined"].data_ptr(), 1, 0, L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1 and len(L.lib().m2m_last_error()) > 0
    for k, t in outs.items():
        assert bool((t == (-7 if k in ("preds", "combined") else SENT)).all()), k


# ---- the engine -----------------------------------------------------------------------------------------------------------------
CASE_S = E.UQCase("uq_avmnist_S", "avmnist", dict(G.AVMNIST["S"], dropout=0.1), 8, 0.1, {})
_PARAMS, _REFS = {}, []


def params_of(case):
    if case.name not in _PARAMS:
        _PARAMS[case.name] = G.make_params(R.case_shapes(case), PARAM_SEED)
    return _PARAMS[case.name]


def build(case, prec, dev, params=None, **kw):
    from m2_mixer_amd.engine import AVMnistUQEngine
    eng = AVMnistUQEngine(case.cfg, case.B, device=dev, precision=prec, lr=LRATE, init=False, **kw)
    eng.load_state_dict(params_of(case) if params is None else params)
    return eng


def same(a, b):
    if isinstance(a, dict):
        return all(torch.equal(x[k], y[k]) for n in a for x, y in zip(a[n], b[n]) for k in x)
    return torch.equal(a, b)


def ref_step(case, params, batch, masks, gates):
    """One float64 reference step from `params` (computed once per distinct (masks, gates); never changed afterwards)."""
    key = (case.name, id(params), id(batch))
    for k, m, g, out in _REFS:
        if k == key and same(m, masks) and same(g, gates):
            return out
    ref = E.UQStep(case, params, LRATE)
    one = ref.step(batch, masks, gates)
    out = dict(one=one, p1={k: v.clone() for k, v in ref.p.items()}, ref=ref)
    _REFS.append((key, masks, gates, out))
    return out


def own_rows(eng):
    """preds rows [image, audio, combined] recomputed in torch from the engine's OWN logits and uncertainties."""
    ev = torch.relu(eng.logits)
    p = ev.argmax(dim=2)
    return torch.stack([p[0], p[1], E.combine(p, eng.uncertainty)]).int()


_BATCHES = {}


def batches(case):
    if case.name not in _BATCHES:
        _BATCHES[case.name] = (R.case_batch(case, 101), R.case_batch(case, 102))
    return _BATCHES[case.name]


def snapshot(eng, grads=True):
    out = dict(logits=eng.logits.clone(), losses=eng.losses.clone(), preds=eng.preds.clone(), uncertainty=eng.uncertainty.clone(),
               own=own_rows(eng))
    if grads:
        out["grads"] = {k: v.clone() for k, v in eng.grads.items()}
    return out


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_engine_two_steps_and_an_evaluation_against_float64(prec, dev):
    """AV-MNIST M2-Mixer-S, dropout 0.1, B = 8, in the manner of test_gpu_engine_envelope: autograd through the oracle's logits
    into edl_ref's loss, fed the engine's dropout masks and gates, then oracle.adam_step."""
    case = CASE_S
    params = params_of(case)
    eng = build(case, prec, dev)
    assert eng._head_part is not None and not eng._fused_heads and eng._heads_are_ce() is False
    assert eng.loss_weights.tolist() == [1.0, 1.0, 1.0] and tuple(eng.preds.shape) == (3, 8) and tuple(eng.uncertainty.shape) == (3, 8)
    with pytest.raises(NotImplementedError):
        eng.set_fusion_loss_weight(0.5)
    b1, b2 = batches(case)
    g1, g2 = tuple(t.to(dev) for t in b1), tuple(t.to(dev) for t in b2)
    eng.forward_backward(*g1)
    torch.cuda.synchronize()
    masks1, got1 = R.engine_masks(eng, case.B), snapshot(eng)
    eng.optimizer_step()
    torch.cuda.synchronize()
    cleared, p1 = R.grads_cleared(eng), {k: v.clone() for k, v in eng.params.items()}
    eng.forward_backward(*g2)
    torch.cuda.synchronize()
    masks2, got2 = R.engine_masks(eng, case.B), snapshot(eng)
    counters = (float(eng.adam_state[0]), int(eng.drop_step[0]))
    out = eng.evaluate(*g1)
    torch.cuda.synchronize()
    gotev = snapshot(eng, grads=False)
    assert torch.equal(out["preds"], eng.preds[2]) and torch.equal(out["uncertainty"], eng.uncertainty[2])
    assert torch.equal(out["uncertainty_image"], eng.uncertainty[0]) and torch.equal(out["uncertainty_audio"], eng.uncertainty[1])

    first = ref_step(case, params, b1, masks1, got1["logits"].cpu() > 0)
    ref = E.UQStep(case, first["p1"], LRATE)
    ref.t, ref.m, ref.v = 1, dict(first["ref"].m), dict(first["ref"].v)
    two = ref.step(b2, masks2, got2["logits"].cpu() > 0)
    ev = first["ref"].forward(b1, first["p1"], gates=gotev["logits"].cpu() > 0)
    bar, kind, bad = BARS[prec], f"engine uq {prec}", []

    def hold(what, value, tol, name):
        observe(f"{kind} {what}", value, tol)
        if not value < tol:
            bad.append(f"{name}: {value:.3e} >= {tol:.0e}")

    for tag, got, want in (("step 1", got1, first["one"]), ("step 2", got2, two), ("eval", gotev, ev)):
        hold("logits (abs)", err(got["logits"], want["logits"]), bar["logits"], f"{tag} logits")
        hold("losses (abs)", err(got["losses"], want["losses"]), bar["losses"], f"{tag} losses")
        hold("uncertainty (abs)", err(got["uncertainty"], want["uncertainty"]), bar["logits"], f"{tag} uncertainty")
        if not torch.equal(got["preds"], got["own"]):
            bad.append(f"{tag}: preds rows are not [image, audio, combined] of the engine's own logits and uncertainties")
    for tag, got, want in (("step 1", got1, first["one"]), ("step 2", got2, two)):
        if tag == "step 2" and prec != "fp32":
            continue                                   # (the first update's bf16 sign noise: test_gpu_engine_envelope's docstring)
        for k, g in want["grads"].items():
            scale = float(g.abs().max())
            if k.endswith(R.NOISE_KEYS):
                floor = float(want["grads"][k[:-4] + "weight"].abs().max())
                scale = scale if scale > 1e-6 * floor else floor
            hold("gradients (rel to max)", err(got["grads"][k], g) / max(scale, 1e-30), bar["grads"], f"{tag} grad {k}")
    hold("parameters after the update (abs)", max(err(p1[k], v) for k, v in first["p1"].items() if not k.endswith(R.NOISE_KEYS)),
         bar["params"], "parameters")
    if not cleared:
        bad.append("the update left gradient elements uncleared outside the kept ranges")
    if counters != (2.0, 2):
        bad.append(f"step counters (Adam, dropout) after step 2: {counters}")
    assert not bad, f"{case.name} [{prec}]: " + "; ".join(bad)


def unordered_towers(eng):
    """Prefixes of the towers whose backward adds its small gradients (LayerNorms, token mixing, biases) with float atomics from
    more than two workgroups: no per-workgroup slots (runtime.TowerRuntime.has_small_slots: bf16 at hidden_dim 128 only) and
    ceil(B / (16 // N)) > 2 sample tiles.  (Two atomic adds onto zero commute exactly; three or more land in any order.)  The
    parent's cross-entropy engine has the same property: it belongs to the tower kernels, not to the heads."""
    a, b = eng.MODS
    out = []
    for prefix, t in ((f"{a}_mixer.", eng.t_a), (f"{b}_mixer.", eng.t_b), ("fusion_mixer.", eng.t_fus)):
        tiles = -(-eng.B // max(1, 16 // t.N))
        if not t.has_small_slots() and tiles > 2:
            out.append(prefix)
    return tuple(out)


def test_captured_replay_equals_the_eager_step_bit_for_bit_in_bf16(dev):
    """M2-Mixer-S, B = 8, bf16: logits, per-head losses, predictions, uncertainties, and the parameters and Adam moments of every
    tensor whose gradient is summed in a fixed order -- the heads (slots), the embeddings, the two modality towers -- are equal
    BIT FOR BIT between an eager step and a captured replay.  At this shape the fusion tower (hidden_dim 32: no slots; N = 8: four
    sample tiles) adds its small gradients with float atomics in any order, in the parent's engine as well (two eager
    AVMnistEngine steps differ in exactly those tensors, by <= 2.4e-10 of a first moment of 2.6e-4): its tensors are held at
    the bar of test_gpu_engine_envelope.test_captured_step_equals_the_eager_step, 2e-4 of the first moment's max.  The whole-model
    bit-for-bit comparison is made where every sum is ordered: test_hidden_dim_128_... below.  (losses[3] sums six atomic
    contributions in any order: 1e-6.)  A two-step graph leaves the last step's uncertainties in the buffer."""
    case = CASE_S
    batch = tuple(t.to(dev) for t in batches(case)[0])
    eager, graphed = build(case, "bf16", dev), build(case, "bf16", dev)
    eager.fused_step(*batch)
    replay = graphed.capture(*batch)
    replay(*batch)
    torch.cuda.synchronize()
    assert float(graphed.adam_state[0]) == 1.0 and int(graphed.drop_step[0]) == 1
    for k in ("logits", "preds", "uncertainty"):
        assert torch.equal(getattr(graphed, k), getattr(eager, k)), k
    assert torch.equal(graphed.losses[:3], eager.losses[:3]) and err(graphed.losses, eager.losses) < 1e-6
    assert torch.equal(graphed.preds, own_rows(graphed))
    loose = unordered_towers(eager)
    assert loose == ("fusion_mixer.",)
    for k in eager.params:
        if k.startswith(loose):
            scale = float(eager.exp_avg[k].abs().max())
            assert err(graphed.exp_avg[k], eager.exp_avg[k]) <= 2e-4 * scale, k
            continue
        for name in ("params", "exp_avg", "exp_avg_sq"):
            assert torch.equal(getattr(graphed, name)[k], getattr(eager, name)[k]), (name, k)
    assert R.grads_cleared(graphed) and R.grads_cleared(eager)
    # steps = 2: per-step preds slots hold [image, audio, combined] of their step; `uncertainty` holds the last step's values
    b2 = tuple(t.to(dev) for t in batches(case)[1])
    multi = build(case, "bf16", dev)
    multi.capture(*batch, steps=2)(*batch, *b2)
    torch.cuda.synchronize()
    assert torch.equal(multi.preds_steps[0], eager.preds)
    for i in range(2):
        ev = torch.relu(multi.logits_steps[i]).argmax(dim=2)
        assert torch.equal(multi.preds_steps[i][:2], ev[:2].int())
    last = torch.stack([ev[0], ev[1], E.combine(ev, multi.uncertainty)]).int()
    assert torch.equal(multi.preds_steps[1], last)                       # the buffer holds the LAST step's uncertainties
    assert bool((multi.uncertainty > 0).all()) and bool((multi.uncertainty <= 1).all())


def test_ragged_batch_through_a_sibling(dev):
    """A training sibling of batch 5 over the engine's parameters: its step against float64, then the parent evaluates."""
    case = CASE_S
    small = case._replace(name="uq_avmnist_S_b5", B=5)
    eng = build(case, "fp32", dev)
    sib = eng.sibling(5)
    assert type(sib) is type(eng) and tuple(sib.uncertainty.shape) == (3, 5) and sib.loss_weights.data_ptr() == eng.loss_weights.data_ptr()
    b = tuple(t[:5].contiguous() for t in batches(case)[0])
    sib.pack()
    sib.forward_backward(*(t.to(dev) for t in b))
    torch.cuda.synchronize()
    got = snapshot(sib)
    ref = E.UQStep(small, params_of(case), LRATE).step(b, R.engine_masks(sib, 5), got["logits"].cpu() > 0)
    bar = BARS["fp32"]
    assert observe("engine uq sibling logits (abs)", err(got["logits"], ref["logits"]), bar["logits"]) < bar["logits"]
    assert observe("engine uq sibling losses (abs)", err(got["losses"], ref["losses"]), bar["losses"]) < bar["losses"]
    assert observe("engine uq sibling uncertainty (abs)", err(got["uncertainty"], ref["uncertainty"]), bar["logits"]) < bar["logits"]
    for k in ("classifier_image.weight", "classifier_audio.bias", "classifier_fusion.classifer.weight", "image_mixer.to_patch_embedding.0.weight"):
        g = ref["grads"][k]
        assert observe("engine uq sibling gradients (rel to max)", err(got["grads"][k], g) / float(g.abs().max()), bar["grads"]) < bar["grads"], k
    assert torch.equal(got["preds"], got["own"])
    sib.optimizer_step()
    eng.pack()
    out = eng.evaluate(*(t.to(dev) for t in batches(case)[0]))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out["loss"])) and torch.equal(eng.preds, own_rows(eng))


def test_score_tables_count_the_preds_rows_as_given(dev):
    """scores=True: the training table's confusion matrices are those of rows [image, audio, combined] against the labels."""
    case = CASE_S
    eng = build(case, "fp32", dev, scores=True)
    batch = tuple(t.to(dev) for t in batches(case)[0])
    eng.fused_step(*batch)
    torch.cuda.synchronize()
    K, labels = eng.K, batch[2].cpu()
    want = torch.stack([torch.bincount(labels * K + eng.preds[h].cpu().long(), minlength=K * K).view(K, K) for h in range(3)])
    assert torch.equal(eng.scores.counts(), want)
    table = eng.new_score_table()
    eng.evaluate(*batch, scores=table)
    torch.cuda.synchronize()
    want = torch.stack([torch.bincount(labels * K + eng.preds[h].cpu().long(), minlength=K * K).view(K, K) for h in range(3)])
    assert torch.equal(table.counts(), want)


def test_hidden_dim_128_takes_the_slot_path_and_two_bf16_runs_are_bit_identical(dev):
    """M2-Mixer-B (hidden_dim 128, K = 10: K D + K + 2 = 1292 <= 1472), bf16, B = 128 -- the configuration whose cross-entropy
    training is bit-reproducible (tests/test_gpu_parity.py test_bf16_training_is_bit_reproducible): with the evidential heads'
    weight gradients in the slots it stays so.  Every gradient of the first step between two engines, then the parameters and
    outputs after three more steps, eager on one engine and captured replays on the other: bit for bit."""
    from m2_mixer_amd.engine import AVMnistUQEngine
    cfg, B = dict(G.AVMNIST["B"]), 128
    make = lambda: AVMnistUQEngine(cfg, B, device=dev, precision="bf16", lr=1e-3, seed=3)
    eng, alt = make(), make()
    alt.load_state_dict(eng.state_dict())
    batch = tuple(t.to(dev) for t in G.avmnist_batch(B, 5, cfg))
    for e in (eng, alt):
        assert e._head_part is not None and e._wgrad_heads is None
        e.forward_backward(*batch)
        assert e._wgrad_heads is not None and all(h.get("g_part") is not None for h in e._wgrad_heads)
    torch.cuda.synchronize()
    assert torch.equal(eng.logits, alt.logits) and torch.equal(eng.uncertainty, alt.uncertainty) and torch.equal(eng.preds, alt.preds)
    differing = [k for k in eng.grads if not torch.equal(eng.grads[k], alt.grads[k])]
    assert not differing, differing
    for k in ("classifier_image.weight", "classifier_audio.bias", "classifier_fusion.classifer.weight"):
        assert float(eng.grads[k].abs().max()) > 0.0, k                 # the slots were added
    assert unordered_towers(eng) == ()                                   # every sum of this step has a fixed order
    eng.optimizer_step()
    alt.optimizer_step()
    replay = alt.capture(*batch)                                         # eager steps on one side, captured replays on the other
    for _ in range(3):
        eng.train_step(*batch)
        replay(*batch)
    torch.cuda.synchronize()
    assert torch.equal(eng.flat_p, alt.flat_p) and torch.equal(eng.uncertainty, alt.uncertainty)
    assert torch.equal(eng.preds, own_rows(eng)) and err(eng.losses, alt.losses) < 1e-6


# ---- the module -----------------------------------------------------------------------------------------------------------------
def model_cfg(case):
    c = case.cfg
    mods = {"image": dict(c["image"], block_type="MLPMixer"), "audio": dict(c["audio"], block_type="MLPMixer"),
            "multimodal": dict(c["multimodal"], block_type="FusionMixer", fusion_function="ConcatFusion"),
            "classification": dict(classifier="StandardClassifier", num_classes=c["num_classes"],
                                   input_shape=[16, 49, c["multimodal"]["hidden_dim"]])}
    return {"dropout": c["dropout"], "modalities": mods, "fusion_loss_change": 0.25}


UQ_KEYS = {"uncertainty", "uncertainty_image", "uncertainty_audio"}
LOSS_KEYS = {"loss", "loss_image", "loss_audio", "loss_fusion"}
EVAL_KEYS = LOSS_KEYS | UQ_KEYS | {"preds", "preds_image", "preds_audio", "labels", "image_logits", "audio_logits", "logits"}


def test_bound_module_steps_and_the_unbound_shared_step(dev):
    """One training_step and one validation_step of the bound AVMnistMixerMultiLossUQ: the reference's keys, the values of the
    engine test's float64 reference; the unbound shared_step on the same (updated) weights agrees with the bound validation_step
    at the fp32 bar."""
    from m2_mixer_amd import models as MD
    from m2_mixer_amd.engine import AVMnistUQEngine
    case, bar = CASE_S, BARS["fp32"]
    params = params_of(case)
    net = MD.AVMnistMixerMultiLossUQ(model_cfg(case), {"lr": LRATE}).to(dev)
    net.load_state_dict(params)
    eng = net.bind_engine(case.B, precision="fp32")
    assert type(eng) is AVMnistUQEngine
    b1 = batches(case)[0]
    batch = {"image": b1[0].to(dev), "audio": b1[1].to(dev), "label": b1[2].to(dev)}
    out = net.training_step(batch)
    torch.cuda.synchronize()
    assert set(out) == LOSS_KEYS | UQ_KEYS | {"preds", "labels"}
    first = ref_step(case, params, b1, R.engine_masks(eng, case.B), eng.logits.cpu() > 0)
    one = first["one"]
    for i, k in enumerate(("loss_image", "loss_audio", "loss_fusion", "loss")):
        assert observe("module uq training losses (abs)", err(out[k], one["losses"][i]), bar["losses"]) < bar["losses"], k
    for i, k in ((2, "uncertainty"), (0, "uncertainty_image"), (1, "uncertainty_audio")):
        assert out[k].dim() == 0
        assert observe("module uq training mean uncertainty (abs)", err(out[k], one["uncertainty"][i].mean()), bar["logits"]) < bar["logits"], k
    assert out["preds"].dtype == torch.int64 and torch.equal(out["preds"], eng.preds[2].long()) and torch.equal(out["labels"], batch["label"])
    # the schedule moves the module's attribute and does not reach the engine (whose loss has no fusion_loss_weight)
    w0 = net.fusion_loss_weight
    net.validation_epoch_end([])
    assert net.fusion_loss_weight == pytest.approx(w0 + 0.25) and eng.loss_weights.tolist() == [1.0, 1.0, 1.0]

    val = net.validation_step(batch)
    torch.cuda.synchronize()
    assert set(val) == EVAL_KEYS
    got_logits = torch.stack([val["image_logits"], val["audio_logits"], val["logits"]])
    ev = first["ref"].forward(b1, first["p1"], gates=got_logits.cpu() > 0)
    assert observe("module uq validation logits (abs)", err(got_logits, ev["logits"]), bar["logits"]) < bar["logits"]
    for i, k in enumerate(("loss_image", "loss_audio", "loss_fusion", "loss")):
        assert observe("module uq validation losses (abs)", err(val[k], ev["losses"][i]), bar["losses"]) < bar["losses"], k
    for i, k in ((2, "uncertainty"), (0, "uncertainty_image"), (1, "uncertainty_audio")):
        assert observe("module uq validation mean uncertainty (abs)", err(val[k], ev["uncertainty"][i].mean()), bar["logits"]) < bar["logits"], k

    # unbound, on the weights the bound module now holds
    import m2_mixer_amd as M
    was = M.get_precision()
    M.set_precision("fp32")                          # the module path's towers in the bound engine's precision
    try:
        free = MD.AVMnistMixerMultiLossUQ(model_cfg(case), {"lr": LRATE}).to(dev)
        free.load_state_dict(net.state_dict())
        free.eval()
        with torch.no_grad():
            un = free.shared_step(batch, mode="val")
        torch.cuda.synchronize()
    finally:
        M.set_precision(was)
    assert set(un) == EVAL_KEYS
    for k in ("image_logits", "audio_logits", "logits"):
        assert observe("module uq unbound vs bound logits (abs)", err(un[k], val[k]), bar["logits"]) < bar["logits"], k
    for k in sorted(LOSS_KEYS):
        assert observe("module uq unbound vs bound losses (abs)", err(un[k], val[k]), bar["losses"]) < bar["losses"], k
    for k in sorted(UQ_KEYS):
        assert observe("module uq unbound vs bound mean uncertainty (abs)", err(un[k], val[k]), bar["logits"]) < bar["logits"], k
    head_ok, comb_ok = E.decisions(ev["logits"])
    for i, k in ((0, "preds_image"), (1, "preds_audio")):
        assert torch.equal(un[k].cpu()[head_ok[i]], val[k].cpu()[head_ok[i]]), k
    assert torch.equal(un["preds"].cpu()[comb_ok], val["preds"].cpu()[comb_ok])
