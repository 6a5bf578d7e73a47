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
        assert c.engine != "mimic" or c.p == 0.0, "the MIMIC cases stay at p = 0 (no mask export for the static MLP)"
        for v in c.expect.values():
            assert not isinstance(v, dict) or set(v) == {"fp32", "bf16"}, c.name
    # dropout is spread over the cases: off, the one-bit stream and a general rate; masks in a grouped and an ungrouped case
    assert {0.0, 0.5} <= {c.p for c in CASES} and any(c.p not in (0.0, 0.5) for c in CASES)
    for grouped in (True, False):
        assert any(c.p > 0 and c.expect.get("grouped") is grouped for c in CASES), grouped


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
