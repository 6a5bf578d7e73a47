"""CPU checks of the tower I/O case table (tests/tower_io_cases.py): every case takes the path the table names under the restated
host rules, the table reaches every path, and -- with the float64 oracle alone -- the inputs of tests/test_gpu_tower_io.py make
its clauses sharp: a kernel that dropped one of the two upstream terms, one input part, or took one token for the token mean,
would miss the float64 reference by a quarter of the tensor's maximum, far above the bf16 bar; and the gradient pre-fill G0
costs the accumulation clause none of its bar."""
import pytest
import torch

import split_cases as SC
import tower_io_cases as IO
from test_gpu_shape_envelope import BF16_GRAD_REL, BF16_REL, FP32_REL, path_of, rel

SHARP = 0.25            # of the reference tensor's maximum: more than ten times the widest bar
TOWERS = [(n, i) for n in IO.NAMES for i in range(len(IO.towers_of(n)))]


def test_every_case_takes_the_path_the_table_names():
    assert len(set(IO.NAMES)) == len(IO.NAMES) == len(IO.PATHS) == 9
    for name in IO.NAMES:
        for prec in IO.precisions(name):
            assert IO.path_of(name, prec) == IO.PATHS[name], (name, prec)
        for t, _ in IO.towers_of(name):
            # the descriptor check of the library (m2m_check_tower) takes the tower
            assert t.D in (32, 64, 128, 256) and 1 <= t.N <= 128 and 1 <= t.T <= 32 and 1 <= t.nb <= SC.MAX_BLOCKS, name
            assert IO.is_wide(t) or t.T % 8 == 0, name
            assert t.p == 0.0, name
    for c in IO.SINGLES:       # the module path's classification agrees with the restated rule
        assert (path_of(c) == "wide") == IO.is_wide(IO.towers_of(c.name)[0][0]), c.name
    # the split cases run fused without the switch, and fp32 never splits
    assert IO.path_of("split_single", "bf16", split=False) == ("fused", "single")
    assert IO.path_of("split_pair", "bf16", split=False) == ("fused", "pair")
    assert SC.split_form(IO.towers_of("split_single")[0][0], prec="fp32") == 0
    assert all(SC.split_form(a, b) == 0 for n, (a, b) in IO.PAIRS.items() if n != "split_pair")


def test_table_reaches_every_path_and_every_ragged_tile():
    assert set(IO.PATHS.values()) == {(p, k) for p in ("fused", "wide", "split") for k in ("single", "pair")}
    assert not all(ln for n in IO.NAMES for _, ln in IO.towers_of(n))                   # a tower without the final LayerNorm
    tow = lambda n, i=0: IO.towers_of(n)[i][0]
    tiles = lambda t: SC.mix_tiles(t.B, t.N)
    t = tow("fused_n3")
    assert tiles(t) == 2 and t.B % SC.spw(t.N) == 2 and SC.spw(t.N) * t.N == 15
    assert SC.fused_class(tow("fused_n7_noln").N, tow("fused_n7_noln").T) == (8, 8)
    a, b = tow("fused_pair"), tow("fused_pair", 1)
    assert (tiles(a), tiles(b)) == (2, 2) and a.B % SC.spw(a.N) != b.B % SC.spw(b.N) and a.nb != b.nb
    a, b = tow("fused_pair_tiles"), tow("fused_pair_tiles", 1)
    assert (tiles(a), tiles(b)) == (1, 3)
    t = tow("wide_d32")
    assert t.D == 32 and t.B % 2 == 1 and (t.B * t.N) % 16 != 0
    assert tow("wide_d256").D == 256 and tow("wide_d256").N <= 8
    a, b = tow("wide_pair"), tow("wide_pair", 1)
    assert a.N != b.N and IO.can_group_wide(a, b, a.B) and not IO.can_group(a, b)
    a, b = tow("split_pair"), tow("split_pair", 1)
    assert (SC.chain_row_tiles(a.B, a.N), SC.chain_row_tiles(b.B, b.N)) == (1, 2)
    assert set(IO.ACCUMULATE) <= set(IO.NAMES) and {IO.PATHS[n] for n in IO.ACCUMULATE} == set(IO.PATHS.values())
    assert {IO.PATHS[n][0] for n in IO.EVAL_CASES} == {"fused", "wide", "split"}
    assert {IO.PATHS[n] for n in IO.PARTS_CASES} == {("fused", "pair"), ("split", "pair")}


def test_restated_wide_grouping_rule():
    T = IO.Tow
    a, b = IO.PAIRS["wide_pair"]
    assert IO.can_group_wide(a, b, 3) and IO.can_group_wide(a, b, 64) and not IO.can_group_wide(a, b, 65)   # 4 chunks x B <= 256
    assert not IO.can_group_wide(a, b._replace(T=24), 3) and not IO.can_group_wide(a._replace(T=24), b._replace(T=24), 3)
    assert not IO.can_group_wide(a, b._replace(nb=1), 3) and not IO.can_group_wide(a._replace(nb=5), b._replace(nb=5), 3)
    assert not IO.can_group_wide(a, b._replace(p=0.5), 3)
    assert not IO.can_group_wide(T(128, 9, 8, 33, 2, 3, 0.0), T(128, 9, 8, 33, 2, 3, 0.0), 3)              # hidden_dim 256 only
    assert not IO.can_group_wide(T(128, 4, 8, 33, 2, 3, 0.0), a, 3)                                         # a fused tower


# ---- conditions on the inputs (float64 oracle only) ------------------------------------------------------------------------
# Operand rounding is one of about four bf16 roundings of comparable size between a kernel's inputs and a parameter gradient (the
# operands of the forward products, the stored activations, the operands of the backward products, the operand images of the
# weight-gradient launch); a reference that operand rounding alone moves by a quarter of a bar leaves the kernels no room, and
# the case would measure its inputs.  The seed of a tower is the first whose reference stays below that.
COND_SHARE = 0.25


def conditions(name, i, seed=None):
    """The conditions the float64 reference of tower i misses at `seed` (None: the case's own): [] when the inputs are good."""
    tow, has_ln = IO.towers_of(name)[i]
    ref = lambda parts, form, **kw: IO.reference(name, i, parts, form, seed, **kw)
    bad = []
    both = ref(1, "both")["dx"]
    bad += [f"upstream {f}" for f in ("out", "pooled") if rel(ref(1, f)["dx"], both) < SHARP]
    runs = [(1, f) for f in ("out", "pooled", "both")]
    if name in IO.PARTS_CASES and i == 0:
        params, xparts, d_out, _ = IO.draw(tow, has_ln, IO.seed_of(name, i) if seed is None else seed)
        for parts in (2, 3, 4):
            runs.append((parts, "both"))
            for drop in range(parts):
                x = sum(xparts[p].double() for p in range(parts) if p != drop)
                if rel(IO.run_oracle(tow, has_ln, params, x, d_out, None)["out"], ref(parts, "out")["out"]) < SHARP:
                    bad.append(f"part {drop} of {parts}")
    if name in IO.PAIRS and tow.N > 1:
        r = ref(1, "out")
        bad += [f"token mean vs token {n}" for n in (0, -1) if rel(r["out"][:, n], r["pooled"]) < SHARP]
    for parts, form in runs:
        acts, grads = IO.conditioning(name, i, parts, form, seed)
        if not (acts < COND_SHARE * BF16_REL and grads < COND_SHARE * BF16_GRAD_REL):
            bad.append(f"conditioning {parts} {form}: {acts:.1e} {grads:.1e}")
    return bad


@pytest.mark.parametrize("name,i", TOWERS, ids=[f"{n}[{i}]" for n, i in TOWERS])
def test_seed_is_the_first_whose_reference_meets_the_conditions(name, i):
    """Upstream forms differ, every input part matters, the token mean is no single token, and bf16 operand rounding moves no
    reference tensor by more than a quarter of its bar -- at the tower's seed, and at no seed between its base and that one:
    the choice depends on the reference alone and is fixed (tower_io_cases.SEEDS)."""
    assert conditions(name, i) == []
    base = IO.base_seed(name, i)
    assert base <= IO.seed_of(name, i) < base + 100
    for seed in range(base, IO.seed_of(name, i)):
        assert conditions(name, i, seed) != [], seed


@pytest.mark.parametrize("name,i", TOWERS, ids=[f"{n}[{i}]" for n, i in TOWERS])
def test_upstream_forms_differ(name, i):
    """d_x0 under both upstream gradients differs from d_x0 under either alone by a quarter of its maximum: a kernel that drops
    d_out or d_pooled cannot hide under a bar.  With neither the reference is exactly zero."""
    both = IO.reference(name, i, 1, "both")["dx"]
    for form in ("out", "pooled"):
        assert rel(IO.reference(name, i, 1, form)["dx"], both) >= SHARP, form
    none = IO.reference(name, i, 1, "none")
    assert float(none["dx"].abs().max()) == 0.0 and all(float(g.abs().max()) == 0.0 for g in none["grads"].values())


@pytest.mark.parametrize("name", IO.PARTS_CASES)
@pytest.mark.parametrize("parts", [2, 3, 4])
def test_every_input_part_matters(name, parts):
    tow, has_ln = IO.towers_of(name)[0]
    params, xparts, d_out, _ = IO.draw(tow, has_ln, IO.seed_of(name, 0))
    ref = IO.reference(name, 0, parts, "out")["out"]
    for drop in range(parts):
        x = sum(xparts[p].double() for p in range(parts) if p != drop)
        assert rel(IO.run_oracle(tow, has_ln, params, x, d_out, None)["out"], ref) >= SHARP, (parts, drop)


@pytest.mark.parametrize("name,i", [(n, i) for n, i in TOWERS if n in IO.PAIRS], ids=lambda v: str(v))
def test_token_mean_differs_from_any_single_token(name, i):
    """A mean that read one row would otherwise pass.  (A tower of ONE token has nothing to tell apart: its mean is its token.)"""
    tow, _ = IO.towers_of(name)[i]
    ref = IO.reference(name, i, 1, "out")
    if tow.N == 1:
        assert torch.equal(ref["pooled"], ref["out"][:, 0])
        return
    assert rel(ref["out"][:, 0], ref["pooled"]) >= SHARP and rel(ref["out"][:, -1], ref["pooled"]) >= SHARP


@pytest.mark.parametrize("name", IO.ACCUMULATE)
def test_prefill_costs_no_precision(name):
    """G0 + reference in float32 differs from the same sum in float64 by less than a tenth of the fp32 bar of the reference."""
    assert FP32_REL < BF16_REL < BF16_GRAD_REL
    for i in range(len(IO.towers_of(name))):
        grads = IO.reference(name, i, 1, "both")["grads"]
        for k, ref in grads.items():
            g0 = IO.g0_of(k, grads)
            assert torch.equal(g0.float().double(), g0) and float(g0.abs().max()) > 0, k
            scale = max(float(ref.abs().max()), IO.grad_floor(k, grads))
            assert float(g0.abs().max()) <= 2 * scale, k
            err = float(((g0.float() + ref.float()).double() - (g0 + ref)).abs().max()) / scale
            assert err < FP32_REL / 10, (k, err)


def test_runtime_refuses_a_tower_of_no_blocks():
    """The kernels have no final-LayerNorm-only form (m2m_check_tower refuses nblocks < 1): the runtime says so before it
    allocates anything."""
    from m2_mixer_amd import _lib as L
    from m2_mixer_amd.runtime import TowerRuntime
    with pytest.raises(RuntimeError, match="at least one block"):
        TowerRuntime(32, 3, 8, 33, 0, True, 0.0, L.PREC_BF16)
