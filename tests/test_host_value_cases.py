"""The value envelope's table (tests/value_cases.py) on the CPU: every regime reaches what it is named for, leaves the comparison
well conditioned, covers every LayerNorm statistics site and GELU table form, and the comparison of tests/test_gpu_value_envelope.py
can see the kernels it is there to catch.

Margins (the bars stay the project's: fp32 1e-4, bf16 2e-2 for outputs and dx, 4e-2 for gradients): the float64 oracle with
bf16-rounded `linear` operands (value_ref.bf16_twin) is within 1/3 of the bf16 bars, and the oracle evaluated in float32 within 1/4
of 1e-4, per (regime, shape, dropout rate), under every measurement the GPU test makes (value_ref.compare: whole tensors, tails
and channel classes, each relative to the float64 reference's maximum over the same slice).
"""
import pytest

import value_cases as VC
import value_ref as VR

IDS = [c.name for c in VC.CASES]
_CACHE = {}


def reference(vc):
    if vc.name not in _CACHE:
        _CACHE[vc.name] = VR.reference(vc)
    return _CACHE[vc.name]


def test_table_is_well_formed():
    assert len(set(IDS)) == len(IDS)
    for path, shape in VC.SHAPES:
        for regime in VC.REGIMES:
            ps = sorted(c.case.p for c in VC.CASES if c.regime == regime and c.case.name == shape.name)
            assert ps == ([0.0, 0.1, 0.5] if regime in VC.DROPOUT_REGIMES else [0.0]), (regime, shape.name)
    # the shapes: fused D 64 with a ragged tile (SPW 4, B 5), the D = 128 builds, a two-block tower; wide with two samples per
    # workgroup (D 32), D 256 and N > 8; the smallest column-split case
    by = {s.name: (p, s) for p, s in VC.SHAPES}
    assert by["fused_n4_d64"][1].B % (16 // by["fused_n4_d64"][1].N) and by["fused_n3_d32_x2"][1].nb == 2
    assert by["wide_n9_d32"][1].D == 32 and by["wide_n5_d256"][1].D == 256 and by["wide_n16_d64"][1].N > 8
    import split_cases as SC
    assert SC.split_form(by["split_u4_s2"][1]) == 2 and all(SC.nunits(c.C) >= SC.nunits(by["split_u4_s2"][1].C) for c in SC.CASES)


@pytest.mark.parametrize("vc", VC.CASES, ids=IDS)
def test_regime_reaches_what_it_is_named_for(vc):
    blocks = VR.reach(vc)
    params, x, _ = VR.inputs(vc)
    c = vc.case
    if vc.regime in ("gelu_tails", "trained"):
        d = blocks[0]                                     # (the tails are on the first block: tests/value_cases.py)
        for k in ("tok_lo", "tok_hi", "ch_lo", "ch_hi"):
            assert d[k] >= 0.05, (k, d[k])
    if vc.regime == "gelu_tails":
        near_lo, near_hi = min(d["tok_near_lo"], d["ch_near_lo"]), min(d["tok_near_hi"], d["ch_near_hi"])
        assert near_lo <= VR.CELL and near_hi <= VR.CELL, (near_lo, near_hi)
    if vc.regime == "ln_offset":
        assert all(d["ratio"] >= 50 for d in blocks), [d["ratio"] for d in blocks]
    if vc.regime == "trained":
        assert blocks[0]["ratio"] >= 50, blocks[0]["ratio"]
    if vc.regime in ("ln_constant_zero", "ln_constant_three"):
        value = 0.0 if vc.regime == "ln_constant_zero" else 3.0
        rows = x[VC.constant_samples(c.B), -VC.CONST_TOKENS:]
        assert len(VC.constant_samples(c.B)) >= 1 and bool((rows == value).all())
        assert blocks[0]["var_min"] == 0.0 and blocks[0]["var_max"] > 0.1          # the other rows are ordinary
    if vc.regime in ("ln_gamma", "trained"):
        lo, hi = (VC.FULL if vc.regime == "ln_gamma" else VC.TRAINED)["gamma_lo"], (VC.FULL if vc.regime == "ln_gamma" else VC.TRAINED)["gamma_hi"]
        gammas = [v for k, v in params.items() if k.endswith(("token_mix.0.weight", "channel_mix.0.weight", "layer_norm.weight"))]
        assert len(gammas) == 2 * c.nb + (c.kind != "block")
        for g in gammas:
            nz = g[g != 0].abs()
            assert bool((g == 0).any()) and bool((g < 0).any()) and bool((g > 0).any())
            assert float(nz.min()) >= lo * 0.999 and float(nz.max()) <= hi * 1.001
            assert float(nz.max()) / float(nz.min()) >= 0.5 * hi / lo / 4          # the draw spans most of the range
    if vc.regime == "outlier_channels":
        hot = list(VC.outlier_index(c.D))
        cold = [i for i in range(c.D) if i not in hot]
        assert float(x[..., hot].pow(2).mean().sqrt()) >= 0.8 * VC.FULL["outlier_scale"] * float(x[..., cold].pow(2).mean().sqrt())


@pytest.mark.parametrize("vc", VC.CASES, ids=IDS)
def test_reference_side_margins(vc):
    ref = reference(vc)
    assert VR.finite(ref)
    twin = VR.worst(vc, VR.bf16_twin(vc), ref)
    f32 = VR.worst(vc, VR.float32_oracle(vc), ref)
    bf, fp = VR.BARS["bf16"], VR.BARS["fp32"]
    print(f"{vc.name}: twin / bar {twin['act'] / bf['act']:.2f} {twin['grad'] / bf['grad']:.2f}; "
          f"float32 / bar {f32['act'] / fp['act']:.3f} {f32['grad'] / fp['grad']:.3f}")
    assert twin["act"] <= bf["act"] / 3 and twin["grad"] <= bf["grad"] / 3, twin
    assert f32["act"] <= fp["act"] / 4 and f32["grad"] <= fp["grad"] / 4, f32


def test_table_reaches_every_statistics_site_and_table_form():
    sites, forms = {}, {}
    for vc in VC.CASES:
        for s in VC.ln_sites(vc):
            sites.setdefault(s, set()).add(vc.regime)
        for prec in VC.precisions(vc):
            for f in VC.table_forms(vc, prec):
                forms.setdefault(f, set()).add((vc.regime, vc.case.p))
    assert set(sites) == set(VC.LN_SITES) and set(forms) == set(VC.TABLE_FORMS)
    for s in VC.LN_SITES:                      # every site sees every regime about row statistics
        assert {"ln_offset", "ln_constant_zero", "ln_constant_three", "ln_gamma", "outlier_channels", "trained"} <= sites[s], s
    for f in VC.TABLE_FORMS:                   # every form sees the tails; the masked one at p = 0.5, the others with the scale 1 / 0.9
        want = {("gelu_tails", 0.5), ("trained", 0.5)} if f == "fp16 masked" else {("gelu_tails", 0.0), ("gelu_tails", 0.1), ("trained", 0.1)}
        assert want <= forms[f], f
    # the kernel builds behind those labels, classified with the rules test_host_cpu restates for the shape envelope:
    # (path, precision, D, NMAX or TM, drop mode) -- every regime reaches every instantiation class, the dropout regimes in all
    # three drop modes
    from test_host_cpu import _builds_of, _is_wide
    for vc in VC.CASES:
        assert _is_wide(vc.case.N, vc.case.D) == (vc.path == "wide"), vc.name
    for regime in VC.REGIMES:
        builds = set().union(*(_builds_of(vc.case) for vc in VC.CASES if vc.regime == regime and vc.path != "split"))
        modes = ("none", "half", "gen") if regime in VC.DROPOUT_REGIMES else ("none",)
        for prec in ("fp32", "bf16"):
            for dm in modes:
                for build in (("fused", prec, 64, 4, dm), ("fused", prec, 128, 8, dm), ("fused", prec, 32, 4, dm),
                              ("wide", prec, 64, 16, dm), ("wide", prec, 256, 32, dm), ("wide", prec, 32, 16, dm)):
                    assert build in builds, (regime, build)


@pytest.mark.parametrize("name", list(VR.MUTANTS))
def test_comparison_sees_a_subtly_wrong_kernel(name):
    """The oracle with one primitive replaced by what a subtly wrong kernel would compute misses the GPU test's bar by >= 3 x on
    every case of the regimes that are there for it -- under the very comparison the GPU test applies (value_ref.compare)."""
    _, _, prec, regimes = VR.MUTANTS[name]
    bar, seen = VR.BARS[prec], 0
    for vc in VC.CASES:
        if vc.regime not in regimes:
            continue
        w = VR.worst(vc, VR.mutant(vc, name), reference(vc))
        factor = max(w["act"] / bar["act"], w["grad"] / bar["grad"])
        print(f"{name} on {vc.name}: {factor:.1f} x the {prec} bar")
        assert factor >= 3.0, (vc.name, factor)
        seen += 1
    assert seen >= len(VC.SHAPES)


# ---- engine level: tests/engine_cases.py configurations with `trained` towers ----------------------------------------------------
@pytest.mark.parametrize("name", VR.ENGINE_CASES)
def test_engine_reference_with_trained_towers_would_show_a_stale_parameter_set(name):
    """As tests/test_host_engine_cases.py for the table: the float64 step is finite, the towers carry the trained magnitudes, and
    the step-2 logits computed with the parameters of before the first update are at least ten bf16 logits bars away."""
    import torch

    import engine_ref as R
    import gen_util as G
    from engine_cases import CASES
    from test_host_engine_cases import BF16_LOGITS, LR
    case = next(c for c in CASES if c.name == name)
    init = G.make_params(R.case_shapes(case), VR.ENGINE_PARAM_SEED)
    params = VR.engine_params(case)
    assert list(params) == list(init)
    for k in params:
        changed = not torch.equal(params[k], init[k])
        tower = k.startswith(VR.ENGINE_TOWERS) and "to_patch_embedding" not in k
        assert not changed or tower, k                    # embeddings and heads keep their initialisation scale
    assert max(float(v.abs().max()) for v in params.values()) >= 8.0
    ref = R.Step(case, params, LR)
    b1, b2 = R.case_batch(case, 101), R.case_batch(case, 102)
    out = ref.step(b1)
    assert all(bool(torch.isfinite(t).all()) for t in (out["logits"], out["losses"], *out["grads"].values(), *ref.p.values()))
    tops = [float(g.abs().max()) for k, g in out["grads"].items() if not k.endswith(R.NOISE_KEYS)]
    assert max(tops) / min(tops) >= 100.0                  # the update sees gradients spanning decades
    true2 = ref.forward(b2)["logits"]
    stale2 = ref.forward(b2, {k: v.double() for k, v in params.items()})["logits"]
    gap = float((true2 - stale2).abs().max())
    assert gap >= 10 * BF16_LOGITS, f"{name}: stale parameters move the step-2 logits by {gap:.3f} only"
