"""CPU tests of the module-path lifecycle table (tests/lifecycle_cases.py): its reach, the premise about torch's optimizers that
the `adam_fused` cases rest on, and the condition on the inputs that keeps the GPU test's oracle comparison from passing
vacuously."""
import pytest
import torch

from lifecycle_cases import (CASES, GRAPH_UPDATES, MODELS, OBSERVATIONS, SILENT_UPDATES, TASKS, UPDATES, applies, is_packed)
from lifecycle_ref import Ref

FP32_ATOL = 1e-3       # the logits bar of tests/test_gpu_module_lifecycle.py


def test_table_hygiene():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    for c in CASES:
        assert c.model in MODELS, c.name
        assert c.precs and set(c.precs) <= {"fp32", "bf16"}, c.name
        assert all(e in UPDATES or e in OBSERVATIONS for e in c.events), c.name
        assert c.events[0] in UPDATES and c.events[-1] in OBSERVATIONS, c.name
        assert all(applies(e, c.model) for e in c.events if e in UPDATES), f"{c.name}: GraphedStep takes dict batches"
        assert c.lr >= 1e-2 and c.p == 0.0, c.name
        # every observation follows an update directly: the stale distance compares with the weights of before that update
        assert all(c.events[i - 1] in UPDATES for i, e in enumerate(c.events) if e in OBSERVATIONS), c.name
    assert not any(applies(u, "mimic") for u in GRAPH_UPDATES) and all(applies(u, "avmnist") for u in UPDATES)


def _observed_after(case):
    """[(observation, updates since the previous observation, number of observations before it)]"""
    out, since = [], []
    for e in case.events:
        if e in UPDATES:
            since.append(e)
        else:
            out.append((e, tuple(since), len(out)))
            since = []
    return out


def test_table_reaches_every_update_observation_and_second_evaluation():
    seen = {(c.model, u, o) for c in CASES for o, since, _ in _observed_after(c) for u in since}
    for m in TASKS:
        for u in UPDATES:
            if applies(u, m):
                assert (m, u, "eval") in seen, (m, u)
    for o in OBSERVATIONS:
        assert any(s[2] == o for s in seen), o
        for u in ("adam_fused", "graph_fused"):
            assert any(s[1] == u and s[2] == o for s in seen), (u, o)
    # the evaluation that a GraphedStep's constructor cannot cover for: a second observation with only updates of the one kind since
    # the first
    for u in SILENT_UPDATES:
        assert any(nth >= 1 and set(since) == {u} for c in CASES for _, since, nth in _observed_after(c)), u
    # after graph replays, every observation kind occurs as such a later observation
    for o in OBSERVATIONS:
        assert any(obs == o and nth >= 1 and set(since) == {"graph_fused"} for c in CASES for obs, since, nth in _observed_after(c)), o
    assert any(len(set(e for e in c.events if e in UPDATES)) > 1 for c in CASES), "one mixed sequence"
    assert any(c.model == "deep" for c in CASES), "one tower deeper than a descriptor"


def test_fused_adam_leaves_the_version_counters_alone():
    """The premise of the `adam_fused` cases: torch.optim.Adam(fused=True).step() changes the parameters without advancing their
    `_version`, the foreach form advances it -- so a pack keyed on the counters alone goes stale after fused steps."""
    moved = {}
    for fused in (False, True):
        p = torch.nn.Parameter(torch.ones(8))
        opt = torch.optim.Adam([p], lr=1e-2, fused=fused, foreach=not fused)
        p.grad = torch.full((8,), 0.5)
        v0 = p._version
        opt.step()
        assert not torch.equal(p.detach(), torch.ones(8))
        moved[fused] = p._version - v0
    assert moved[False] >= 1, "the foreach form no longer advances _version: the `adam_foreach` cases are no control any more"
    assert moved[True] == 0, ("torch's fused Adam now advances the parameters' version counters: the `adam_fused` cases of "
                              "tests/lifecycle_cases.py have lost their bite (a version-keyed pack would pass them)")


@pytest.mark.parametrize("name", list(MODELS))
def test_stale_packed_tensors_would_show(name):
    """The float64 oracle trained by torch's CPU Adam at the table's learning rate: after each of four steps, logits computed with
    the packed tensors of BEFORE the step and everything else current differ from the true ones by at least ten times the fp32
    logits bar, in every head a tower feeds.  A condition on the learning rate, the seeds and the batches; the GPU test asserts
    the same on the weights its own updates produce."""
    lrs = {c.lr for c in CASES if c.model == name}
    assert lrs
    ref = Ref(name)
    for lr in lrs:
        p = {k: v.double().requires_grad_(True) for k, v in ref.params().items()}
        assert any(is_packed(k) for k in p)
        opt = torch.optim.Adam(list(p.values()), lr=lr)
        for n in range(1, 5):
            prev = {k: v.detach().clone() for k, v in p.items()}
            opt.zero_grad()
            ref.forward(ref.batch(1000 + n), p)["loss"].backward()
            opt.step()
            gap = ref.stale_distance(ref.batch(3001 + n), {k: v.detach() for k, v in p.items()}, prev)
            assert gap >= 10 * FP32_ATOL, f"{name}, lr {lr:g}, step {n}: stale packed tensors move the logits by {gap:.2e} only"
