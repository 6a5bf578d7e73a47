"""CPU checks of the column-split case table (tests/split_cases.py) and of the bars its GPU tests use: the table, classified
with the restated host rules, reaches every decision of the path; a float32 evaluation of every sharp case stays inside the
bars against float64; and the float64 result with ONE 32-column unit's hidden activation missing, or with one split's share
of the channel output missing, does not -- so the bars are neither unreachable nor vacuous before anything runs on a GPU."""
import numpy as np
import pytest
import torch

import gen_util as G
import split_cases as SC
from oracle import m2mixer_oracle as O
from test_gpu_shape_envelope import BF16_GRAD_REL, BF16_REL, case_shapes, make_input, rel

W1, B1, W2 = "channel_mix.1.net.0.weight", "channel_mix.1.net.0.bias", "channel_mix.1.net.3.weight"


def _splits(case):
    S = SC.split_count(case.C)
    return S, SC.unit_ranges(case.C, S)


def test_table_matches_the_restated_rules():
    assert len({c.name for c in SC.CASES}) == len(SC.CASES)
    for c in SC.CASES:
        assert c.D == 128 and 1 <= c.N <= 8 and c.T % 8 == 0 and 1 <= c.nb <= SC.MAX_BLOCKS, c.name
        assert SC.split_form(c) == SC.EXPECT_S[c.name], c.name
        S, rng = _splits(c)
        assert rng[0][0] == 0 and rng[-1][1] == SC.nunits(c.C) and all(a[1] == b[0] for a, b in zip(rng, rng[1:])), c.name
        assert all(2 <= u1 - u0 <= SC.SP_MAX_UNITS_PER_SPLIT for u0, u1 in rng), c.name
        assert SC.split_form(c, mode=0) == 0
    for name, prec, c, _ in SC.REFUSED:
        assert SC.split_form(c, prec=prec) == 0, name


def test_table_reaches_every_decision():
    cs = SC.CASES
    per = {c.name: [u1 - u0 for u0, u1 in _splits(c)[1]] for c in cs}
    assert {SC.EXPECT_S[c.name] for c in cs} == set(range(2, 9))
    assert any(all(SC.chunks(0, n) == 1 for n in per[c.name]) for c in cs)                        # nch == 1 in every split
    assert any(n % 2 for c in cs for n in per[c.name][:-1]) and any(per[c.name][-1] % 2 for c in cs)   # odd: non-final, final
    assert {SC.fused_class(c.N, c.T) for c in cs} == {(4, 8), (8, 16), (8, 8)}
    assert {c.N for c in cs} == set(range(1, 9))
    assert {c.T for c in cs} == {8, 16, 24, 32}
    assert {SC.drop_mode(c.p) for c in cs} == {"none", "half", "gen"}
    assert {1, 2, 8} <= {c.nb for c in cs}
    assert {c.kind for c in cs} == {"block", "fusion"}                                             # without / with final LayerNorm
    rows = {c.B * c.N for c in cs}
    assert min(rows) < 128 and 128 in rows and 129 in rows
    assert any(SC.chain_row_tiles(c.B, c.N) == 2 for c in cs)
    assert any(c.B % SC.spw(c.N) == 1 and SC.spw(c.N) > 1 and SC.mix_tiles(c.B, c.N) > 1 for c in cs)   # last mix tile: one sample
    assert {16 - SC.spw(c.N) * c.N for c in cs} >= {0, 1, 2, 4}                                    # 16, 15, 14 and 12 rows of 16 used
    assert any(SC.image_rows(c.B, c.N) > (c.B * c.N + 15) // 16 * 16 for c in cs)                  # more image rows than ceil16(B N)
    assert any(max(per[c.name]) == SC.SP_MAX_UNITS_PER_SPLIT for c in cs)
    assert any(c.C % 32 for c in cs)
    # token MLP zero padding in LDS: N below NMAX
    assert any(c.N < SC.fused_class(c.N, c.T)[0] for c in cs)


def test_pair_cases_follow_the_grouping_rules():
    a, b = SC.PAIR_UNEQUAL
    assert SC.split_form(a, b) == 2 and SC.nunits(a.C) != SC.nunits(b.C)
    assert SC.chain_row_tiles(a.B, a.N) == 1 and SC.chain_row_tiles(b.B, b.N) == 2
    for name, (a, b) in SC.PAIR_NOT_GROUPABLE.items():
        assert SC.split_form(a) >= 2 and SC.split_form(b) >= 2 and SC.split_form(a, b) == 0, name
    a, b = SC.PAIR_MIXED
    assert SC.split_form(a) == 2 and SC.split_form(b) == 0 and SC.split_form(a, b) == 0 and SC.split_form(b, a) == 0
    # M2M_SPLIT_MIN_ROWS: from B N == threshold on
    c = SC.CASES[0]
    assert SC.split_form(c, mode=-1, min_rows=c.B * c.N) == 2 and SC.split_form(c, mode=-1, min_rows=c.B * c.N + 1) == 0
    assert SC.split_form(c, mode=-1) == 0


# ---- sensitivity of the bars ---------------------------------------------------------------------------------------------
def _block_run(case, dtype, ch_keep=None):
    """One-block case on the CPU in `dtype`: (output, {W1, b1, W2 gradients}); ch_keep: (C,) 0/1 over the hidden columns."""
    params = G.make_params(case_shapes(case), 4242)
    x = make_input(case, np.random.default_rng(977))
    rng = np.random.default_rng(5)
    dy = torch.from_numpy(rng.standard_normal((case.B, case.N, case.D)))
    leaves = {k: v.to(dtype).requires_grad_(True) for k, v in params.items()}
    pre = "" if case.kind == "block" else "mixer_blocks.0."
    masks, p = None, 0.0
    if ch_keep is not None:
        one = lambda *s: torch.ones(s, dtype=dtype)
        masks = {"tok_h": one(case.B, case.D, case.T), "tok_o": one(case.B, case.D, case.N),
                 "ch_h": ch_keep.to(dtype).expand(case.B, case.N, case.C), "ch_o": one(case.B, case.N, case.D)}
        p = 1e-30                                                     # (the oracle applies masks only where p > 0; scale 1)
    if case.kind == "block":
        y = O.mixer_block(x.to(dtype), leaves, "", p, masks)
    else:
        y = O.fusion_mixer(x.to(dtype), leaves, "", 1, p, None if masks is None else [masks])
    (y * dy.to(dtype)).sum().backward()
    return y.detach(), {k: leaves[pre + k].grad for k in (W1, B1, W2)}


def _errors(y, g, yr, gr):
    """The GPU test's measurements that involve the channel MLP: (output, worst unit slice of W1, of W2)"""
    worst = lambda k: max(rel(a, b) for a, b in zip(SC.unit_slices(k, g[k]), SC.unit_slices(k, gr[k])))
    return rel(y, yr), worst(W1), worst(W2)


SHARP = [c for c in SC.CASES if c.nb == 1 and c.name not in SC.INSENSITIVE]


@pytest.mark.parametrize("case", SHARP, ids=[c.name for c in SHARP])
def test_bars_see_a_lost_unit_and_a_lost_slab(case):
    yr, gr = _block_run(case, torch.float64)
    e_out, e_w1, e_w2 = _errors(*_block_run(case, torch.float32), yr, gr)
    assert e_out < BF16_REL / 100 and e_w1 < BF16_GRAD_REL / 100 and e_w2 < BF16_GRAD_REL / 100, (e_out, e_w1, e_w2)
    S, rng = _splits(case)
    odd = [r for r in rng if (r[1] - r[0]) % 2] or rng
    u = odd[-1][1] - 1                                     # the last unit of an odd split (the half chunk), else of the last split
    keep = torch.ones(case.C, dtype=torch.float64)
    keep[32 * u:32 * u + 32] = 0
    lost_unit = _errors(*_block_run(case, torch.float64, keep), yr, gr)
    u0, u1 = rng[S // 2]
    keep = torch.ones(case.C, dtype=torch.float64)
    keep[32 * u0:32 * u1] = 0
    lost_slab = _errors(*_block_run(case, torch.float64, keep), yr, gr)
    for what, (e_out, e_w1, e_w2) in (("unit", lost_unit), ("slab", lost_slab)):
        assert e_out > BF16_REL, (what, e_out)
        assert e_w1 > BF16_GRAD_REL and e_w2 > BF16_GRAD_REL, (what, e_w1, e_w2)


def test_every_block_count_has_a_sharp_neighbour():
    """The cases the sensitivity check cannot run (more than one block: the perturbation would have to name a block; one unit of
    512) share their split shapes with cases it does run."""
    assert {c.name for c in SC.CASES} - {c.name for c in SHARP} == {"u5_s2_odd", "u9_s4", "u17_s8_x8", "u512_s8_edge"}
