"""CPU tests of the engine configuration table (tests/engine_cases.py): hygiene, coverage of every dispatch decision, the float64
reference on every config, and the condition that makes the GPU test's second step mean something."""
import pytest
import torch

import engine_ref as R
import gen_util as G
from engine_cases import CASES, DECISIONS, FIXED_DECISIONS

LR = 2e-3              # tests/test_gpu_engine_envelope.py trains with it (see there)
PARAM_SEED = 31
BF16_LOGITS = 2e-2     # the looser precision's logits bar of the GPU test


def test_table_hygiene():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    for c in CASES:
        assert c.engine in ("avmnist", "mmimdb", "mimic"), c.name
        assert c.expect and set(c.expect) <= set(DECISIONS), (c.name, set(c.expect) - set(DECISIONS))
        assert c.cfg["dropout"] == c.p and 0.0 <= c.p < 1.0, c.name
        for v in c.expect.values():
            assert not isinstance(v, dict) or set(v) == {"fp32", "bf16"}, c.name
    # dropout is spread over the cases: off, the one-bit stream and a general rate; masks in a grouped and an ungrouped case
    assert {0.0, 0.5} <= {c.p for c in CASES} and any(c.p not in (0.0, 0.5) for c in CASES)
    for grouped in (True, False):
        assert any(c.p > 0 and c.expect.get("grouped") is grouped for c in CASES), grouped
    # MIMIC with dropout: both streams, the riding MLP flushed on its own (fused time tower) and carried (wide time tower)
    mimic = [c for c in CASES if c.engine == "mimic" and c.p > 0]
    assert 0.5 in {c.p for c in mimic} and any(c.p != 0.5 for c in mimic)
    for time_wide in (True, False):
        assert any(c.expect.get("mlp_ride") is True and c.expect.get("time_wide") is time_wide for c in mimic), time_wide


def _values(decision):
    out = set()
    for c in CASES:
        v = c.expect.get(decision)
        if isinstance(v, dict):
            out |= set(v.values())
        elif v is not None:
            out.add(v)
    return out


def test_every_decision_takes_both_values():
    """Each decision the engines take from the configuration is asserted at both of its values somewhere in the table (row
    groups: 1, 2 and >= 3).  FIXED_DECISIONS have one value a configuration can reach; the table pins it."""
    for d in DECISIONS:
        vals = _values(d)
        if d in FIXED_DECISIONS:
            assert vals == {FIXED_DECISIONS[d]}, (d, vals)
        elif d.startswith("groups_"):
            assert all(isinstance(v, int) and v >= 1 for v in vals), d
        else:
            assert vals == {True, False}, (d, vals)
    groups = set().union(*(_values(f"groups_{t}") for t in ("a", "b", "fus")))
    assert 1 in groups and 2 in groups and any(g >= 3 for g in groups), groups


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_reference_runs_and_a_stale_parameter_set_would_show(case):
    """The float64 reference takes the config (non-square images, unequal token counts, N = 1) and its step is finite; and the
    step-2 logits computed with the parameters of BEFORE the first update differ from the true ones by at least ten times the
    bf16 logits bar: a packed operand copy, a slot or a step counter that the update left behind cannot hide inside the
    tolerance of the GPU test's second step.  A condition on LR, the parameter seed and the batches -- not on the kernels."""
    shapes = R.case_shapes(case)
    params = G.make_params(shapes, PARAM_SEED)
    ref = R.Step(case, params, LR)
    b1, b2 = R.case_batch(case, 101), R.case_batch(case, 102)
    out = ref.step(b1)
    assert list(out["grads"]) == list(shapes)
    assert out["logits"].shape == (3, case.B, case.cfg["num_classes"]) and out["losses"].shape == (4,)
    assert all(bool(torch.isfinite(t).all()) for t in (out["logits"], out["losses"], *out["grads"].values(), *ref.p.values()))
    true2 = ref.forward(b2)["logits"]
    stale2 = ref.forward(b2, {k: v.double() for k, v in params.items()})["logits"]
    gap = float((true2 - stale2).abs().max())
    assert gap >= 10 * BF16_LOGITS, f"{case.name}: stale parameters move the step-2 logits by {gap:.3f} only"


def random_masks(case, seed):
    """Random keep-masks (rate 1 - p) for the three mask groups of a MIMIC case, in the layouts oracle.mimic_forward takes."""
    gen = torch.Generator().manual_seed(seed)
    keep = 1 - R.p_effective(case.p or 0.5)
    draw = lambda *shape: (torch.rand(*shape, generator=gen) < keep).double()
    B, ct, cs, cm = case.B, case.cfg["time"], case.cfg["static"], case.cfg["multimodal"]

    def tower(c, N):
        D, T, C = c["hidden_dim"], c["token_dim"], c["channel_dim"]
        return [{"tok_h": draw(B, D, T), "tok_o": draw(B, D, N), "ch_h": draw(B, N, C), "ch_o": draw(B, N, D)} for _ in range(c["num_mixers"])]

    return {"time": tower(ct, ct["num_patch"]), "fusion": tower(cm, 1 + ct["num_patch"]),
            "static": [draw(B, cs["hidden_dim"]) for _ in range(cs["num_blocks"])]}


MIMIC_CASES = [c for c in CASES if c.engine == "mimic"]


@pytest.mark.parametrize("case", MIMIC_CASES, ids=[c.name for c in MIMIC_CASES])
def test_mimic_reference_takes_masks_in_all_three_groups(case):
    """The float64 MIMIC reference under random keep-masks for the time tower, the fusion tower and the static MLP (the successor of
    "the MIMIC cases stay at p = 0"): finite, and every group's masks reach the loss -- replacing one group's masks by all-ones
    moves it.  On the cases with dropout the reference's whole step (autograd + Adam) runs with the masks."""
    params = {k: v.double() for k, v in G.make_params(R.case_shapes(case), PARAM_SEED).items()}
    batch, masks = R.case_batch(case, 101), random_masks(case, 7)
    drop_p = R.p_effective(case.p or 0.5)
    ones = lambda m: {k: torch.ones_like(v) for k, v in m.items()} if isinstance(m, dict) else torch.ones_like(m)
    with torch.no_grad():
        full = R.case_forward(case, batch, params, drop_p, masks)
        assert bool(torch.isfinite(full["logits"]).all()) and bool(torch.isfinite(full["losses"]).all())
        for group in ("time", "fusion", "static"):
            other = dict(masks, **{group: [ones(m) for m in masks[group]]})
            moved = float((R.case_forward(case, batch, params, drop_p, other)["losses"] - full["losses"]).abs().max())
            assert moved > 1e-3, (group, moved)
    if case.p > 0:
        out = R.Step(case, params, LR).step(batch, masks)
        assert torch.equal(out["losses"], full["losses"])
        assert all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for k, g in out["grads"].items() if not k.endswith(R.NOISE_KEYS))
