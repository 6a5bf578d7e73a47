"""Value envelope of the tower kernels (-m gpu): every case of tests/value_cases.py -- trained-weight magnitudes instead of the
initialisation-scale values every other tower test draws -- runs forward and backward in training mode through the module path,
in fp32 and bf16 (the column-split path: bf16, forced with M2M_SPLIT=1), and is compared with the float64 oracle at the bars of
tests/test_gpu_shape_envelope.py: the output, dx and every parameter gradient over the whole tensor and over the shape envelope's
tails, for outlier_channels also per channel class (value_ref.compare), and nothing may be NaN or Inf.  Dropout cases feed the
oracle the kernels' own keep-masks.  Every error is recorded under a kind that names the regime (conftest.observe).

Then: the backward is linear in the upstream gradient, so the same forward followed by backwards under dy, dy 2^-20 and dy 2^20
must give results that differ by exactly that power of two (bit for bit on the bf16 fused launch, whose gradients go through
slots with a fixed summation order -- DESIGN section 8; to 1e-6 of the tensor's maximum where float atomics or another launch
order may reorder fp32 sums): an absolute threshold, an fp16 temporary or a flush in a backward launch breaks it.  And the
evaluation-mode forward of gelu_tails and ln_offset, per path, against the oracle.

tests/test_host_value_cases.py checks on the CPU that each regime reaches the code it is named for, that the reference side
leaves a margin of 3 x (bf16) / 4 x (fp32) under these bars, and that this comparison misses by >= 3 x on an oracle that computes
what a subtly wrong kernel would.
"""
import pytest
import torch

import value_cases as VC
import value_ref as VR
from conftest import observe
from test_gpu_shape_envelope import dev, kernel_masks, make_module, precision, run_case  # noqa: F401

pytestmark = pytest.mark.gpu

RUNS = [(vc, prec) for vc in VC.CASES for prec in VC.precisions(vc)]
_REFS = {}       # case name -> float64 reference of a case without dropout: computed once, shared by the two precisions


def reference(vc, params, x, dy, masks):
    if masks is not None:
        return VR.run(vc, params, x, dy, masks=masks)
    if vc.name not in _REFS:
        _REFS[vc.name] = VR.run(vc, params, x, dy)
    return _REFS[vc.name]


def on_path(vc, mod):
    """The launch path the case is listed under is the one its calls take."""
    rt = mod._rts[0]
    if vc.path == "split":
        assert rt.split_form(vc.case.B, True) == 2, "the case is off the column-split path"
    else:
        assert rt.split_form(vc.case.B, True) == 0


def hold(vc, prec, got, ref, label="", **kw):
    bad = []
    for kind, what, err, cls in VR.compare(vc, got, ref, **kw):
        tol = VR.BARS[prec][cls]
        observe(f"value {vc.regime} {vc.path} {prec} {label}{kind}", err, tol)
        if not err < tol:
            bad.append(f"{what}: {err:.3e} > {tol:.0e}")
    return bad


@pytest.mark.parametrize("vc,prec", RUNS, ids=[f"{vc.name}-{prec}" for vc, prec in RUNS])
def test_value_case_vs_float64_oracle(vc, prec, dev, precision, monkeypatch):
    precision(prec)
    monkeypatch.setenv("M2M_SPLIT", "1" if vc.path == "split" else "0")
    mod, params, x, dy, y, xd = run_case(vc.case, prec, dev, transform=VC.transform(vc.regime))
    on_path(vc, mod)
    masks = kernel_masks(mod, vc.case) if vc.case.p > 0 else None
    ref = reference(vc, params, x, dy, masks)
    got = {"out": y.detach(), "dx": xd.grad}
    for k, prm in mod.named_parameters():
        assert prm.grad is not None, k
        got[k] = prm.grad
    assert set(got) == set(ref)
    nonfinite = [k for k, v in got.items() if not bool(torch.isfinite(v).all())]
    assert not nonfinite, f"{vc.name} [{prec}]: NaN or Inf in {nonfinite}"
    bad = hold(vc, prec, got, ref)
    assert not bad, f"{vc.name} [{prec}]: " + "; ".join(bad)


# ---- one shape per path for the two properties below ------------------------------------------------------------------------------
PATH_SHAPE = {"fused": "fused_n4_d64", "wide": "wide_n16_d64", "split": "split_u4_s2"}


def path_runs(regimes, tags=("",)):
    out = []
    for shape in PATH_SHAPE.values():
        for regime in regimes:
            for tag in tags:
                vc = VC.by_name(f"{regime}-{shape}{tag}")
                out += [(vc, prec) for prec in VC.precisions(vc)]
    return out


HOMOGENEITY = path_runs(("trained",), ("", "_half"))
SCALES = (1.0, 2.0 ** -20, 2.0 ** 20)


@pytest.mark.parametrize("vc,prec", HOMOGENEITY, ids=[f"{vc.name}-{prec}" for vc, prec in HOMOGENEITY])
def test_backward_is_homogeneous_in_the_upstream_gradient(vc, prec, dev, precision, monkeypatch):
    precision(prec)
    monkeypatch.setenv("M2M_SPLIT", "1" if vc.path == "split" else "0")
    params, x, dy = VR.inputs(vc)
    mod = make_module(vc.case).to(dev)
    mod.load_state_dict(params)
    mod.train()
    xd = x.to(dev).requires_grad_(True)
    y = mod(xd)
    on_path(vc, mod)
    leaves = [xd] + [p for _, p in mod.named_parameters()]
    names = ["dx"] + [k for k, _ in mod.named_parameters()]

    def backward(scale):
        gs = torch.autograd.grad(y, leaves, grad_outputs=(dy * scale).to(dev), retain_graph=True)
        torch.cuda.synchronize()
        return dict(zip(names, (g.clone() for g in gs)))

    base = backward(1.0)
    assert all(bool(torch.isfinite(v).all()) for v in base.values())
    exact = prec == "bf16" and vc.path == "fused"
    bad = []
    for scale in SCALES:          # (scale 1 again: the saved activations survive a backward, the launches are repeatable)
        got = backward(scale)
        for k in names:
            back = got[k] / scale                                   # a power of two: exact
            if exact:
                same = torch.equal(back, base[k])
                observe(f"value homogeneity {vc.path} {prec} (differing elements)", float((back != base[k]).sum()), 1.0)
            else:
                floor = VR.zero_gradient_floor(k, base)
                err = float((back - base[k]).abs().max()) / max(float(base[k].abs().max()), floor, 1e-30)
                observe(f"value homogeneity {vc.path} {prec} (rel to max)", err, 1e-6)
                same = err <= 1e-6
            if not same:
                d = (back - base[k]).abs().max() / base[k].abs().max().clamp_min(1e-30)
                bad.append(f"{k} at dy x {scale:g}: off by {float(d):.3e} of its max")
    assert not bad, f"{vc.name} [{prec}]: " + "; ".join(bad)


EVAL = path_runs(("gelu_tails", "ln_offset"))


@pytest.mark.parametrize("vc,prec", EVAL, ids=[f"{vc.name}-{prec}" for vc, prec in EVAL])
def test_evaluation_forward_vs_float64_oracle(vc, prec, dev, precision, monkeypatch):
    precision(prec)
    monkeypatch.setenv("M2M_SPLIT", "1" if vc.path == "split" else "0")
    params, x, dy = VR.inputs(vc)
    mod = make_module(vc.case).to(dev)
    mod.load_state_dict(params)
    mod.eval()
    with torch.no_grad():
        y = mod(x.to(dev))
    torch.cuda.synchronize()
    rt = mod._rts[0]
    assert rt.split_form(vc.case.B, False) == (2 if vc.path == "split" else 0)
    ref = reference(vc, params, x, dy, None)          # (no dropout in these cases: the training forward computes the same)
    assert bool(torch.isfinite(y).all())
    bad = hold(vc, prec, {"out": y}, ref, label="eval ", acts=("out",))
    assert not bad, f"{vc.name} [{prec}] eval: " + "; ".join(bad)


# ---- engine level: the one-launch Adam + re-pack on weights of magnitude ~10 and gradients spanning decades -----------------------
_ENGINE_REFS = {}


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", VR.ENGINE_CASES)
def test_engine_steps_with_trained_towers(name, prec, dev):
    """Two training steps and an evaluation of a tests/engine_cases.py configuration whose towers carry the `trained` parameters
    (heads and embeddings at initialisation scale), against engine_ref.Step at test_gpu_engine_envelope.BARS: logits, losses and
    gradients of both steps -- the second sees the updated, re-packed weights --, the evaluation, and the parameters after the
    update wherever the reference gradient exceeds 1e-6 of its tensor's maximum (below that Adam's normalisation turns rounding
    noise into +-lr steps).  tests/test_host_value_cases.py: an un-updated parameter set would move the step-2 logits by >= 10
    bars."""
    import engine_ref as R
    from engine_cases import CASES
    from test_gpu_engine_envelope import BARS, LR, build, err
    case = next(c for c in CASES if c.name == name)
    params = VR.engine_params(case)
    eng = build(case, prec, dev, params)
    b1, b2 = R.case_batch(case, 101), R.case_batch(case, 102)
    g1, g2 = tuple(t.to(dev) for t in b1), tuple(t.to(dev) for t in b2)
    snap = lambda: dict(logits=eng.logits.clone(), losses=eng.losses.clone(), grads={k: v.clone() for k, v in eng.grads.items()})
    eng.forward_backward(*g1)
    torch.cuda.synchronize()
    masks1 = R.engine_masks(eng, case.B) if case.p > 0 else None
    got1 = snap()
    eng.optimizer_step()
    torch.cuda.synchronize()
    p1 = {k: v.clone() for k, v in eng.params.items()}
    eng.forward_backward(*g2)
    torch.cuda.synchronize()
    masks2 = R.engine_masks(eng, case.B) if case.p > 0 else None
    got2 = snap()
    eng.evaluate(*g1)
    torch.cuda.synchronize()
    gotev = dict(logits=eng.logits.clone(), losses=eng.losses.clone())

    hit = _ENGINE_REFS.get(name)
    if hit is None or not (R.masks_equal(hit[0], masks1) and R.masks_equal(hit[1], masks2)):
        ref = R.Step(case, params, LR)
        one = ref.step(b1, masks1)
        p1ref = {k: v.clone() for k, v in ref.p.items()}
        two = ref.step(b2, masks2)
        hit = _ENGINE_REFS[name] = (masks1, masks2, dict(one=one, p1=p1ref, two=two, ev=ref.forward(b1, p1ref)))
    ref = hit[2]
    bar, kind, bad = BARS[prec], f"value trained engine {name} {prec}", []

    def hold_(what, value, tol, label):
        observe(f"{kind} {what}", value, tol)
        if not value < tol:
            bad.append(f"{label}: {value:.3e} >= {tol:.0e}")

    for tag, got, want in (("step 1", got1, ref["one"]), ("step 2", got2, ref["two"]), ("eval", gotev, ref["ev"])):
        assert bool(torch.isfinite(got["logits"]).all()) and bool(torch.isfinite(got["losses"]).all()), tag
        hold_(f"{tag} logits (abs)", err(got["logits"], want["logits"]), bar["logits"], f"{tag} logits")
        hold_(f"{tag} losses (abs)", err(got["losses"], want["losses"]), bar["losses"], f"{tag} losses")
    for tag, got, want in (("step 1", got1, ref["one"]), ("step 2", got2, ref["two"])):
        for k, g in want["grads"].items():
            scale = float(g.abs().max())
            if k.endswith(R.NOISE_KEYS):                     # (the existing exemption: tests/test_gpu_engine_envelope.py)
                floor = float(want["grads"][k[:-4] + "weight"].abs().max())
                scale = scale if scale > 1e-6 * floor else floor
            assert bool(torch.isfinite(got["grads"][k]).all()), (tag, k)
            hold_(f"{tag} gradients (rel to max)", err(got["grads"][k], g) / max(scale, 1e-30), bar["grads"], f"{tag} grad {k}")
    worst = 0.0
    for k, v in ref["p1"].items():
        if k.endswith(R.NOISE_KEYS):
            continue
        g = ref["one"]["grads"][k]
        sure = g.abs() > 1e-6 * g.abs().max()
        assert bool(torch.isfinite(p1[k]).all()), k
        if bool(sure.any()):
            worst = max(worst, float((p1[k].double().cpu() - v).abs()[sure].max()))
    hold_("parameters after the update (abs)", worst, bar["params"], "parameters")
    assert float(eng.adam_state[0]) == 2.0          # (as tests/test_gpu_engine_envelope.py reads it after the second forward_backward)
    assert not bad, f"{name} [{prec}]: " + "; ".join(bad)
