"""CPU checks of the patch-embedding case table (tests/embed_cases.py) and of the bar its GPU tests use (tests/embed_ref.py):
the table, classified with the restated host rules, reaches every launch form; a float32 evaluation of every case stays inside
the derived bound against float64; and the float64 result with one term left out does not -- so the bound is neither
unreachable nor vacuous before anything runs on a GPU."""
import pytest
import torch

import embed_cases as EC
import embed_ref as ER
from embed_cases import G


def _fwd_units():
    """(prec, D, geometry name, B, nsplit) of every forward the GPU tests run"""
    out = [(p, D, g, B, 1) for p, D, g, B in EC.FWD_SINGLE]
    for p, D, gs, B, nss in EC.FWD_GROUP:
        out += [(p, D, g, B, ns) for g in gs for ns in nss]
    for p, D, gs, B, nss in EC.FWD_GENERIC_PARTS:
        out += [(p, D, g, B, ns) for g, ns in zip(gs, nss)]
    out += [("bf16", D, g, B, parts) for D, g, B, parts in EC.CONSUMER]
    for p, D, _, gs, B in EC.TOWER_FWD:
        out += [(p, D, g, B, 1) for g in gs if g is not None]
    return out


def _rows_units():
    """(prec, D, geometry name, B, merged) of every row-group weight gradient"""
    out = []
    for merged in (False, True):
        out += [(p, D, g, B, merged) for p, D, g, B in EC.WGRAD_ROWS]
        for p, D, gs, B in EC.WGRAD_ROWS_GROUP:
            out += [(p, D, g, B, merged) for g in gs]
    return out


def _owner_units():
    """(D, geometry name, B, input offset by 4 bytes) of every single-owner weight gradient"""
    return [(D, g, B, off) for D, gs, B, _, offs in EC.WGRAD_OWNER for g, off in zip(gs, offs)]


def test_every_geometry_is_legal():
    for name, g in G.items():
        assert g.H % g.ph == 0 and g.W % g.pw == 0, name
        for prec in ("bf16", "fp32"):
            assert EC.padK(EC.geomK(g), prec) <= 3968, name
    for p, D, C, gs, B in EC.TOWER_FWD:
        for g in gs:
            assert g is None or 16 % EC.geomN(G[g]) == 0           # whole samples per 16-row tile
    assert all(B <= 320 for *_, B, _ in _fwd_units()) and all(B <= 320 for _, _, _, B, _ in _rows_units())
    assert all(B <= 320 for _, _, B, _ in _owner_units())


def test_forward_cases_reach_every_form():
    units = _fwd_units()
    fast = {EC.fwd_fast_ok(G[g], p) for p, D, g, B, ns in units}
    assert fast == {True, False}
    assert {D for _, D, *_ in units} == {32, 64, 128, 256}
    gen = [(p, G[g], B) for p, D, g, B, ns in units if not EC.fwd_fast_ok(G[g], p)]
    assert any(g.ph > g.pw for _, g, _ in gen) and any(g.ph < g.pw for _, g, _ in gen) and any(g.Cin == 3 for _, g, _ in gen)
    assert any(p == "bf16" and g.pw % 8 != 0 for p, g, _ in gen) and any(p == "fp32" for p, g, _ in gen)
    assert any(EC.geomK(g) % EC.kblock(p) != 0 for p, g, _ in gen)
    assert any(EC.geomK(g) < EC.EMB_KS for _, g, _ in gen) and any(129 <= EC.geomK(g) <= 144 for _, g, _ in gen)
    assert any(B * EC.geomN(g) < 16 for _, g, B in gen) and any(B * EC.geomN(g) % 16 != 0 for _, g, B in gen)
    # the fast body's k-splits
    splits = [(G[g], ns) for p, D, g, B, ns in units if EC.fwd_fast_ok(G[g], p)]
    assert {ns for _, ns in splits} == {1, 2, 3, 4}
    assert {EC.geomK(g) for g, _ in splits} >= {40, 256, 264, 640, 1024}
    stages = [(EC.split_stages(g, ns), ns) for g, ns in splits if ns > 1]
    assert any(any(lo >= hi for lo, hi in st) for st, _ in stages), "no empty part"
    assert any(st[-1][1] % 2 == 1 for st, _ in stages) and any((hi - lo) % 2 == 1 for st, _ in stages for lo, hi in st), "no odd stage count"
    # K = 640 (3 stages) in 4 parts: part 3 is empty; K = 1024 (4 stages) in 3 parts: part 2 is empty
    assert EC.split_stages(G["c1_32x40_p16x40"], 4) == [(0, 1), (1, 2), (2, 3), (3, 3)]
    assert EC.split_stages(G["c4_16x32_p16"], 3) == [(0, 2), (2, 4), (4, 4)]
    # both argument orders are run, and the dispatch order differs from the argument order in one of them
    for p, D, (a, b), B, nss in EC.FWD_GROUP:
        assert {EC.fwd_first(G[a], G[b], p), EC.fwd_first(G[b], G[a], p)} == {0, 1}, (a, b)
    # what m2m_embed_fwd_splits answers: 2 from Kp = 1024 on the fast body
    assert EC.fwd_splits(G["c4_16x32_p16"], "bf16") == 2 and EC.fwd_splits(G["c1_32x40_p16x40"], "bf16") == 1
    assert EC.fwd_splits(G["c4_16x32_p16"], "fp32") == 1
    # embeddings inside the tower launch: N in {1, 2, 4, 8}, both bodies, both precisions, a NULL embedding, a partial last tile
    tw = [(p, G[g], B) for p, D, C, gs, B in EC.TOWER_FWD for g in gs if g is not None]
    assert {EC.geomN(g) for _, g, _ in tw} == {1, 2, 4, 8} and {p for p, *_ in tw} == {"bf16", "fp32"}
    assert {EC.fwd_fast_ok(g, p) for p, g, _ in tw} == {True, False}
    assert any(g is None for *_, gs, _ in EC.TOWER_FWD for g in gs)
    assert all(B % (16 // EC.geomN(g)) != 0 for _, g, B in tw)
    assert sum(1 for p, D, C, gs, B in EC.TOWER_FWD if p == "fp32" and D == 32 and C <= 32) >= 2       # the small-LDS launches


def test_weight_gradient_cases_reach_every_form():
    plans = [(EC.wgrad_plan(G[g], B, EC.wgrad_target(D, merged)), G[g]) for p, D, g, B, merged in _rows_units()]
    assert any(pl.groups == 1 for pl, _ in plans)
    ragged = [pl for pl, _ in plans if pl.groups >= 2 and pl.last < pl.tpg and pl.M % 32 != 0]
    assert ragged, "no plan with a shorter last group"
    assert EC.wgrad_plan(G["c3_12x12_p4"], 31, 256)[2:] == (1, 2, 5, 9, 4)
    assert EC.wgrad_plan(G["c1_16x24_p16x8"], 113, 256)[2:] == (2, 2, 6, 11, 5)
    assert any(EC.geomK(g) < 64 for _, g in plans) and any(EC.geomK(g) % 64 != 0 and pl.nchunks > 1 for pl, g in plans)
    for merged in (False, True):
        for p, D, (a, b), B in EC.WGRAD_ROWS_GROUP:
            t = EC.wgrad_target(D, merged)
            assert {EC.wgrad_first(G[a], G[b], B, t), EC.wgrad_first(G[b], G[a], B, t)} == {0, 1}, (a, b)
    own = [(EC.wgrad_owner_args(G[g], B, 4 if off else 16), G[g], D, B) for D, g, B, off in _owner_units()]
    assert all(EC.wgrad_owner_ok(g, "bf16", D, B) for _, g, D, B in own)
    assert {o.vec2 for o, *_ in own} == {True, False}
    assert any(not o.vec2 and (g.pw % 2 or g.W % 2) for o, g, *_ in own) and any(not o.vec2 and g.pw % 2 == 0 and g.W % 2 == 0 for o, g, *_ in own)
    assert {o.rpt for o, *_ in own} >= {14, 15, 16}
    assert {EC.geomN(g) for _, g, *_ in own} >= {1, 3, 4, 5, 7, 8} and {D for _, _, D, _ in own} == {32, 64, 128}
    assert {o.npairs for o, *_ in own} >= {1, 3, 6} and any(o.npairs >= 11 for o, *_ in own)
    assert any(o.npairs < EC.owner_waves(D) for o, _, D, _ in own) and any(o.npairs > 2 * EC.owner_waves(D) for o, _, D, _ in own)
    assert any(EC.geomK(g) < 32 for _, g, *_ in own) and any(EC.geomK(g) % 32 != 0 for _, g, *_ in own)
    assert any(B % (16 // EC.geomN(g)) != 0 for _, g, _, B in own)                         # last chain tile partly filled
    assert {ow for *_, ow, _ in EC.WGRAD_OWNER} == {True, False}


@pytest.mark.parametrize("unit", sorted(set(_fwd_units())), ids=lambda u: "-".join(map(str, u)))
def test_forward_bound_holds_in_float32_and_is_sharp(unit):
    prec, D, name, B, ns = unit
    g = G[name]
    x, w, b, _ = ER.make_inputs(g, D, B, seed=7)
    ref, S = ER.fwd_ref(x, w, b, g, prec)
    n = ER.count_fwd(g, ns)
    f32 = ER.patches(ER.rnd(x, prec).float(), g) @ ER.rnd(w, prec).float().reshape(D, -1).t() + b
    assert ER.check_bound(f32, ref, n, S) <= 1.0
    assert ER.is_sharp(ref, ER.fwd_ref_short(x, w, b, g, prec), n, S)


def _wgrad_units():
    out = {(p, D, g, B, False, EC.wgrad_plan(G[g], B, EC.wgrad_target(D, m)).groups) for p, D, g, B, m in _rows_units()}
    out |= {("bf16", D, g, B, True, EC.owner_waves(D)) for D, g, B, _ in _owner_units()}
    return sorted(out)


@pytest.mark.parametrize("unit", _wgrad_units(), ids=lambda u: "-".join(map(str, u)))
def test_weight_gradient_bound_holds_in_float32_and_is_sharp(unit):
    prec, D, name, B, owner, extra = unit
    g = G[name]
    x, _, _, dx0 = ER.make_inputs(g, D, B, seed=9)
    M = B * EC.geomN(g)
    gw, Sw, gb, Sb = ER.wgrad_ref(x, dx0, g, prec, owner)
    n = ER.count_owner(g, B, extra) if owner else ER.count_rows(g, B, extra)
    sw, sb = ER.sentinel(D * EC.geomK(g)).double().reshape(gw.shape), ER.sentinel(D).double()
    P32, d32 = ER.patches(ER.rnd(x, prec).float(), g), ER.rnd(dx0, prec).float()
    b32 = d32 if owner else dx0
    assert ER.check_bound(sw.float() + d32.t() @ P32, sw + gw, n, Sw + sw.abs()) <= 1.0
    assert ER.check_bound(sb.float() + b32.sum(0), sb + gb, n, Sb + sb.abs()) <= 1.0
    gw1, _, gb1, _ = ER.wgrad_ref(x, dx0, g, prec, owner, rows=M - 1)
    assert ER.is_sharp(sw + gw, sw + gw1, n, Sw + sw.abs()) and ER.is_sharp(sb + gb, sb + gb1, n, Sb + sb.abs())
