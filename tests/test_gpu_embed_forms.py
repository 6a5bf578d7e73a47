"""Every launch form of the patch embeddings (tests/embed_cases.py) against the float64 references of tests/embed_ref.py.

Inputs and parameters are sign * U(0.5, 1.5).  Every output buffer has 64 guard floats behind it and is pre-filled, guard
included: NaN where the launch writes, a known finite pattern where it adds.  After the launch the guard is bit-unchanged, no
NaN remains, and every element is inside the derived bound

    |got - ref| <= (n + 2) 2^-23 S          (embed_ref.py: n fp32 additions, S the magnitude sum)

around the reference (pattern + reference for "+=" outputs).  Each case also shows on the CPU that its bar is sharp: the
reference with the last token row (forward: the last k column) left out violates it.  The largest err / bound of every form is
recorded with conftest.observe and printed in the test summary.
"""
import ctypes as C

import pytest
import torch

import embed_cases as EC
import embed_ref as ER
from conftest import observe
from embed_cases import G

pytestmark = pytest.mark.gpu
GUARD = ER.GUARD


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from m2_mixer_amd import _lib
    _lib.lib()      # the HIP library must be there: no fallback
    return torch.device("cuda:0")


def _prec(prec):
    from m2_mixer_amd import _lib as L
    return L.PREC_BY_NAME[prec]


def _ids(c):
    return "-".join(str(v) for v in c).replace(" ", "")


class Guarded:
    """n floats + GUARD behind them, pre-filled with NaN (fill=None) or with fill * embed_ref.sentinel."""

    def __init__(self, n, dev, fill=None):
        self.n = n
        self.init = (torch.full((n + GUARD,), float("nan")) if fill is None else fill * ER.sentinel(n + GUARD)).to(dev)
        self.buf = self.init.clone()

    def check(self):
        """Guard bit-unchanged, nothing unwritten; returns the payload on the CPU."""
        assert torch.equal(self.buf[self.n:].view(torch.int32), self.init[self.n:].view(torch.int32)), "guard floats were written"
        out = self.buf[:self.n].cpu()
        assert not torch.isnan(out).any(), "an output element was never written"
        return out

    def start(self):
        return self.init[:self.n].double().cpu()


def off4(t):
    """A copy of `t` whose address is 4 bytes past a 16-byte boundary."""
    v = torch.empty(t.numel() + 1, device=t.device)[1:].view_as(t)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def make_embed(g, D, prec, w, b, dev):
    from m2_mixer_amd.runtime import EmbedRuntime
    e = EmbedRuntime(g.Cin, g.H, g.W, g.ph, g.pw, D, _prec(prec))
    e.bind_params(w.to(dev).contiguous(), b.to(dev).contiguous())
    e.pack()
    return e


def make_tower(D, N, C, prec, dev, seed, B=None, image=False):
    """A one-block tower (token_dim 8, no dropout) with seeded parameters, packed, gradients bound."""
    from m2_mixer_amd.runtime import TowerRuntime, block_param_shapes
    gen = torch.Generator().manual_seed(seed)
    bp = {}
    for f, s in block_param_shapes(D, N, 8, C).items():
        if f in ("ln1_w", "ln2_w"):
            t = 1 + 0.1 * torch.randn(s, generator=gen)
        elif len(s) == 1:
            t = 0.1 * torch.randn(s, generator=gen)
        else:
            t = torch.randn(s, generator=gen) * s[1] ** -0.5
        bp[f] = t.to(dev).contiguous()
    lnf = ((1 + 0.1 * torch.randn(D, generator=gen)).to(dev), (0.1 * torch.randn(D, generator=gen)).to(dev))
    rt = TowerRuntime(D, N, 8, C, 1, True, 0.0, _prec(prec))
    rt.bind_params([bp], lnf)
    rt.bind_grads(torch.zeros(rt.grad_numel(), device=dev))
    if image:
        assert rt.enable_dx0_image(B)
    rt.pack()
    return rt


def train_towers(towers, x0s, B, dev, seed=5):
    """A real training forward and backward with a random d_out; returns the d_x0 the backward wrote, (B N, D) each."""
    from m2_mixer_amd.runtime import towers_backward, towers_forward
    gen = torch.Generator().manual_seed(seed)
    outs = [torch.empty(B, t.N, t.D, device=dev) for t in towers]
    d_outs = [torch.randn(B, t.N, t.D, generator=gen).to(dev) for t in towers]
    d_x0s = [torch.zeros(B * t.N, t.D, device=dev) for t in towers]
    if len(towers) == 2:
        towers_forward(towers, [(x, t.N * t.D, o, t.N * t.D, None) for t, x, o in zip(towers, x0s, outs)], B, True, seed, 0)
        towers_backward(towers, [(d, t.N * t.D, None, dx, t.N * t.D) for t, d, dx in zip(towers, d_outs, d_x0s)], B, seed, 0)
    else:
        t = towers[0]
        t.forward(x0s[0], t.N * t.D, B, outs[0], t.N * t.D, None, True, seed, 0)
        t.backward(B, d_outs[0], t.N * t.D, None, d_x0s[0], t.N * t.D, seed, 0)
    torch.cuda.synchronize()
    return d_x0s


def assert_fwd(got, x, w, b, g, prec, nsplit, kind):
    ref, S = ER.fwd_ref(x, w, b, g, prec)
    n = ER.count_fwd(g, nsplit)
    ratio = observe(f"embed {kind} [{prec}] err / bound", ER.check_bound(got, ref, n, S), 1.0)
    assert ratio <= 1.0, (kind, ratio)
    assert ER.is_sharp(ref, ER.fwd_ref_short(x, w, b, g, prec), n, S)


# ---- forward, one embedding per launch ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", EC.FWD_SINGLE, ids=_ids)
def test_forward_single(case, dev):
    prec, D, name, B = case
    g = G[name]
    x, w, b, _ = ER.make_inputs(g, D, B, seed=11)
    e = make_embed(g, D, prec, w, b, dev)
    assert e.fwd_splits() == EC.fwd_splits(g, prec)
    out = Guarded(B * EC.geomN(g) * D, dev)
    xd = x.to(dev)
    assert xd.data_ptr() % 16 == 0
    e.forward(xd, B, out.buf)
    torch.cuda.synchronize()
    kind = "forward, fast body" if EC.fwd_fast_ok(g, prec) else "forward, generic body"
    assert_fwd(out.check(), x, w, b, g, prec, 1, kind)


# ---- forward, two embeddings per launch, k-split parts ------------------------------------------------------------------------
def _run_group(prec, D, names, B, nsplits, dev, offset=False, zero_weight=False, seed=13):
    """m2m_embeds_forward on the two geometries in the given order -> [(parts (ns, M D) on the CPU, inputs)] per embedding."""
    from m2_mixer_amd.runtime import embeds_forward
    es, xs, outs, ins = [], [], [], []
    for i, name in enumerate(names):
        g = G[name]
        x, w, b, _ = ER.make_inputs(g, D, B, seed=seed + sum(map(ord, name)))      # (the same data in either argument order)
        if zero_weight:
            w = torch.zeros_like(w)
        es.append(make_embed(g, D, prec, w, b, dev))
        xd = x.to(dev)
        xs.append(off4(xd) if offset else xd)
        outs.append(Guarded(nsplits[i] * B * EC.geomN(g) * D, dev))
        ins.append((x, w, b, g))
    embeds_forward(es, xs, [o.buf for o in outs], B, list(nsplits))
    torch.cuda.synchronize()
    return [(o.check().view(ns, -1), i) for o, ns, i in zip(outs, nsplits, ins)]


@pytest.mark.parametrize("case", EC.FWD_GROUP, ids=_ids)
def test_forward_group_parts_and_order(case, dev):
    prec, D, names, B, nss = case
    for ns in nss:
        per_order = []
        for order in (names, names[::-1]):
            res = _run_group(prec, D, order, B, (ns, ns), dev)
            for parts, (x, w, b, g) in res:
                if EC.fwd_fast_ok(g, prec):
                    for s, (lo, hi) in enumerate(EC.split_stages(g, ns)):
                        if lo >= hi:
                            assert not parts[s].any(), f"part {s} of {ns} is empty and must be exactly 0"
                    assert_fwd(parts.double().sum(0), x, w, b, g, prec, ns, f"forward, fast body, {ns} part(s)")
                else:                                   # the generic body: part 0 holds the whole sum
                    assert not parts[1:].any()
                    assert_fwd(parts[0], x, w, b, g, prec, 1, "forward, generic body (grouped)")
            per_order.append(res if order is names else res[::-1])
        # the results are per embedding: the same bits whichever embedding is named first
        for (pa, _), (pb, _) in zip(*per_order):
            assert torch.equal(pa, pb)
    # the bias appears in part 0 only: with a zero weight part 0 is the bias, bit for bit, and the other parts are 0
    ns = max(nss)
    for parts, (x, w, b, g) in _run_group(prec, D, names, B, (ns, ns), dev, zero_weight=True):
        assert torch.equal(parts[0].view(-1, D), b.expand(parts.shape[1] // D, D)) and not parts[1:].any()


@pytest.mark.parametrize("case", EC.FWD_GENERIC_PARTS, ids=_ids)
def test_generic_body_asked_for_parts(case, dev):
    prec, D, names, B, nsplits = case
    for parts, (x, w, b, g) in _run_group(prec, D, names, B, nsplits, dev, offset=True):
        assert not EC.fwd_fast_ok(g, prec, align=4)
        assert not parts[1:].any(), "parts 1.. of the generic body must be exactly 0"
        assert_fwd(parts[0], x, w, b, g, prec, 1, "forward, generic body asked for parts")


# ---- the consumer of the parts -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", EC.CONSUMER, ids=_ids)
def test_tower_forward_adds_the_parts_in_order(case, dev):
    """m2m_towers_forward given k-split parts against the same call given their fp32 sum, formed on the device in part order
    (the kernel adds part p to the running sum for p = 1, 2, ...: tower_fwd_body's input loop): bit-identical outputs."""
    from m2_mixer_amd.runtime import embeds_forward, towers_forward
    D, name, B, parts = case
    g = G[name]
    N, M = EC.geomN(g), B * EC.geomN(g)
    towers = [make_tower(D, N, 32, "bf16", dev, seed=21 + i) for i in range(2)]
    es, xs = [], []
    for i in range(2):
        x, w, b, _ = ER.make_inputs(g, D, B, seed=17 + i)
        es.append(make_embed(g, D, "bf16", w, b, dev))
        xs.append(x.to(dev))
    bufs = [torch.full((parts, M, D), float("nan"), device=dev) for _ in range(2)]
    embeds_forward(es, xs, bufs, B, [parts, parts])
    outs = [Guarded(M * D, dev) for _ in range(2)]
    towers_forward(towers, [(bf, N * D, o.buf, N * D, None, parts, M * D) for bf, o in zip(bufs, outs)], B, False, 0, 0)
    sums = []
    for bf in bufs:
        s = bf[0].clone()
        for p in range(1, parts):
            s = s + bf[p]
        sums.append(s)
    outs1 = [Guarded(M * D, dev) for _ in range(2)]
    towers_forward(towers, [(s, N * D, o.buf, N * D, None) for s, o in zip(sums, outs1)], B, False, 0, 0)
    torch.cuda.synchronize()
    for o, o1 in zip(outs, outs1):
        assert torch.equal(o.check(), o1.check())


# ---- embeddings inside the tower forward launch --------------------------------------------------------------------------------
def _towers_forward_embeds(towers, ios, embeds, inputs, B):
    """runtime.towers_forward(..., embeds=, inputs=) with embeds[i] = None allowed (m2m_towers_forward_embeds takes a NULL
    embedding: that tower reads the x0 it is given)."""
    from m2_mixer_amd import _lib as L
    n = len(towers)
    for t in towers:
        t.ensure_workspace(B)
    host = (C.POINTER(L.Tower) * n)(*[C.pointer(t.desc) for t in towers])
    io = (L.TowerIO * n)()
    for i, (x0, out) in enumerate(ios):
        nd = towers[i].N * towers[i].D
        io[i].x0, io[i].x0_ss, io[i].out, io[i].out_ss, io[i].pooled = x0.data_ptr(), nd, out.data_ptr(), nd, None
        io[i].x0_parts, io[i].x0_part_stride = 1, 0
    ep = (C.POINTER(L.Embed) * n)(*[C.pointer(e.desc) if e is not None else None for e in embeds])
    ip = (C.c_void_p * n)(*[t.data_ptr() if t is not None else None for t in inputs])
    assert L.lib().m2m_towers_forward_embeds_ok(host, n, ep, B)
    L.check(L.lib().m2m_towers_forward_embeds(host, io, n, ep, ip, None, B, 0, 0, 0, None, L.stream_ptr()), "towers_forward_embeds")


@pytest.mark.parametrize("case", EC.TOWER_FWD, ids=_ids)
def test_embeddings_inside_the_tower_forward(case, dev):
    from m2_mixer_amd.runtime import towers_forward
    prec, D, Cc, names, B = case
    Ns = [EC.geomN(G[n]) for n in names if n is not None]
    towers, es, xs, x0s, data = [], [], [], [], []
    for i, name in enumerate(names):
        N = EC.geomN(G[name]) if name is not None else Ns[0]
        towers.append(make_tower(D, N, Cc, prec, dev, seed=31 + i))
        if name is None:
            es.append(None); xs.append(None); data.append(None)
            x0s.append(torch.randn(B * N * D, generator=torch.Generator().manual_seed(3)).to(dev))
            continue
        g = G[name]
        x, w, b, _ = ER.make_inputs(g, D, B, seed=41 + i)
        es.append(make_embed(g, D, prec, w, b, dev))
        xs.append(x.to(dev))
        data.append((x, w, b, g))
        x0s.append(Guarded(B * N * D, dev))
    outs = [Guarded(B * t.N * D, dev) for t in towers]
    _towers_forward_embeds(towers, [(x0 if e is None else x0.buf, o.buf) for x0, e, o in zip(x0s, es, outs)], es, xs, B)
    torch.cuda.synchronize()
    scratch = []
    for x0, d in zip(x0s, data):
        if d is None:
            scratch.append(x0)
            continue
        x, w, b, g = d
        kind = "fast" if EC.fwd_fast_ok(g, prec) else "generic"
        assert_fwd(x0.check(), x, w, b, g, prec, 1, f"forward inside the tower launch, {kind} body")
        scratch.append(x0.buf[:x0.n].clone())
    # the towers themselves: the same launch fed the scratch the embedding prologue left -- the same arithmetic, bit for bit
    outs1 = [Guarded(B * t.N * D, dev) for t in towers]
    towers_forward(towers, [(s, t.N * D, o.buf, t.N * D, None) for s, t, o in zip(scratch, towers, outs1)], B, False, 0, 0)
    torch.cuda.synchronize()
    for o, o1 in zip(outs, outs1):
        assert torch.equal(o.check(), o1.check())


# ---- weight gradient, row-group form ------------------------------------------------------------------------------------------
def _merged_target(prec, D):
    # (bf16 at hidden_dim 128: the merged launch has 320-thread workgroups and launches the row-group form separately)
    return EC.wgrad_target(D, merged=not (prec == "bf16" and D == 128))


def _rows_setup(prec, D, name, B, dev, seed):
    g = G[name]
    x, w, b, dx0 = ER.make_inputs(g, D, B, seed=seed + sum(map(ord, name)))
    e = make_embed(g, D, prec, w, b, dev)
    gw, gb = Guarded(D * EC.geomK(g), dev, fill=1.0), Guarded(D, dev, fill=1.0)
    e.bind_grads(gw.buf, gb.buf)
    return dict(g=g, x=x, dx0=dx0, e=e, gw=gw, gb=gb, xd=x.to(dev), dxd=dx0.to(dev), prec=prec, B=B)


def _rows_check(s, target, kind):
    g, prec, B = s["g"], s["prec"], s["B"]
    pl = EC.wgrad_plan(g, B, target)
    n = ER.count_rows(g, B, pl.groups)
    rw, Sw, rb, Sb = ER.wgrad_ref(s["x"], s["dx0"], g, prec, owner=False)
    rw1, _, rb1, _ = ER.wgrad_ref(s["x"], s["dx0"], g, prec, owner=False, rows=pl.M - 1)
    for got, ref, ref1, S, what in ((s["gw"], rw, rw1, Sw, "g_w"), (s["gb"], rb, rb1, Sb, "g_b")):
        s0 = got.start().reshape(ref.shape)
        ratio = observe(f"embed wgrad, row groups, {kind} [{prec}] {what} err / bound", ER.check_bound(got.check(), s0 + ref, n, S + s0.abs()), 1.0)
        assert ratio <= 1.0, (kind, what, ratio, pl)
        assert ER.is_sharp(s0 + ref, s0 + ref1, n, S + s0.abs())


@pytest.mark.parametrize("case", EC.WGRAD_ROWS, ids=_ids)
def test_row_group_weight_gradient(case, dev):
    """m2m_embed_wgrad, then the merged weight-gradient launch of a tower carrying the one embedding (nembeds = 1)."""
    from m2_mixer_amd.runtime import towers_wgrad
    prec, D, name, B = case
    s = _rows_setup(prec, D, name, B, dev, seed=51)
    s["e"].wgrad(s["xd"], s["dxd"], B)
    torch.cuda.synchronize()
    _rows_check(s, EC.wgrad_target(D, merged=False), "own launch")
    s = _rows_setup(prec, D, name, B, dev, seed=52)
    tower = make_tower(D, 4, 32, prec, dev, seed=61)
    train_towers([tower], [torch.randn(B * 4, D, generator=torch.Generator().manual_seed(1)).to(dev)], B, dev)
    towers_wgrad([tower], B, [s["e"]], [s["xd"]], [s["dxd"]])
    torch.cuda.synchronize()
    _rows_check(s, _merged_target(prec, D), "merged launch, one embedding")


@pytest.mark.parametrize("case", EC.WGRAD_ROWS_GROUP, ids=_ids)
def test_row_group_weight_gradient_pairs(case, dev):
    """m2m_embeds_wgrad and the merged launch with nembeds = 2 (no d_x0 images: the row-group form), in both argument orders."""
    from m2_mixer_amd.runtime import embeds_wgrad, towers_wgrad
    prec, D, names, B = case
    tower = make_tower(D, 4, 32, prec, dev, seed=62)
    train_towers([tower], [torch.randn(B * 4, D, generator=torch.Generator().manual_seed(2)).to(dev)], B, dev)
    for order in (names, names[::-1]):
        ss = [_rows_setup(prec, D, n, B, dev, seed=53) for n in order]
        embeds_wgrad([s["e"] for s in ss], [s["xd"] for s in ss], [s["dxd"] for s in ss], B)
        torch.cuda.synchronize()
        for s in ss:
            _rows_check(s, EC.wgrad_target(D, merged=False), "own launch, two embeddings")
        ss = [_rows_setup(prec, D, n, B, dev, seed=54) for n in order]
        towers_wgrad([tower], B, [s["e"] for s in ss], [s["xd"] for s in ss], [s["dxd"] for s in ss])
        torch.cuda.synchronize()
        for s in ss:
            _rows_check(s, _merged_target(prec, D), "merged launch, two embeddings")


# ---- weight gradient, single-owner form ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", EC.WGRAD_OWNER, ids=_ids)
def test_single_owner_weight_gradient(case, dev):
    """bf16 fused towers with the d_x0^T image, after a real training forward and backward: the embedding gradients of the merged
    launch against the float64 contraction of the bf16-rounded d_x0 the backward wrote."""
    from m2_mixer_amd import _lib as L
    from m2_mixer_amd.runtime import can_group, towers_wgrad
    D, names, B, overwrite, offsets = case
    towers, es, xs, x0s, st = [], [], [], [], []
    for i, (name, off) in enumerate(zip(names, offsets)):
        g = G[name]
        N = EC.geomN(g)
        x, w, b, _ = ER.make_inputs(g, D, B, seed=71 + i)
        e = make_embed(g, D, "bf16", w, b, dev)
        e.set_wgrad_overwrite(overwrite)
        gw, gb = Guarded(D * EC.geomK(g), dev, fill=1000.0 if overwrite else 1.0), Guarded(D, dev, fill=1.0)
        e.bind_grads(gw.buf, gb.buf)
        xd = off4(x.to(dev)) if off else x.to(dev)
        x0 = torch.empty(B * N, D, device=dev)
        e.forward(xd, B, x0)
        towers.append(make_tower(D, N, 32, "bf16", dev, seed=81 + i, B=B, image=True))
        es.append(e); xs.append(xd); x0s.append(x0)
        st.append(dict(g=g, x=x, gw=gw, gb=gb, args=EC.wgrad_owner_args(g, B, 4 if off else 16)))
        assert EC.wgrad_owner_ok(g, "bf16", D, B)
    assert can_group(towers[0], towers[1], B)
    d_x0s = train_towers(towers, x0s, B, dev)
    ep = (C.POINTER(L.Embed) * 2)(*[C.pointer(e.desc) for e in es])
    tp = (C.POINTER(L.Tower) * 2)(*[C.pointer(t.desc) for t in towers])
    assert L.lib().m2m_embeds_wgrad_form(ep, tp, 2, B) == 1
    # Second pass: the same launch after the image's padding rows (slots rpt..15 of every 16-row chain tile, which the backward
    # leaves zero) are set to 1.0.  g_w must not move: the kernel masks those rows at the second operand (`r < rpt`), so it does
    # not lean on the producer's zeros.  (g_b does -- it sums the image as it is -- and is checked in the first pass only.)
    for poisoned in (False, True):
        if poisoned:
            if all(s["args"].rpt == 16 for s in st):
                break
            for s, t in zip(st, towers):
                _poison_padding_rows(t, s["args"].rpt)
                for got in (s["gw"], s["gb"]):
                    got.buf.copy_(got.init)
        towers_wgrad(towers, B, es, xs, d_x0s, embed_towers=towers)
        torch.cuda.synchronize()
        for s, dx in zip(st, d_x0s):
            g = s["g"]
            n = ER.count_owner(g, B, EC.owner_waves(D))
            rw, Sw, rb, Sb = ER.wgrad_ref(s["x"], dx, g, "bf16", owner=True)
            rw1, _, rb1, _ = ER.wgrad_ref(s["x"], dx, g, "bf16", owner=True, rows=B * EC.geomN(g) - 1)
            for got, ref, ref1, S, what, adds in ((s["gw"], rw, rw1, Sw, "g_w", not overwrite), (s["gb"], rb, rb1, Sb, "g_b", True)):
                if poisoned and what == "g_b":
                    continue
                s0 = got.start().reshape(ref.shape) if adds else torch.zeros_like(ref)     # "=": the garbage is gone
                ratio = observe(f"embed wgrad, single owner [bf16] {what} err / bound", ER.check_bound(got.check(), s0 + ref, n, S + s0.abs()), 1.0)
                assert ratio <= 1.0, (what, ratio, s["args"], poisoned)
                assert ER.is_sharp(s0 + ref, s0 + ref1, n, S + s0.abs())


def _poison_padding_rows(tower, rpt):
    """bf16 1.0 into every padding row of the tower's d_x0^T image.  Layout (embed_wgrad.h, embed_wgrad_fast_body): [32-row pair]
    [d tile][lane = 16 g + il] 16 bytes = 8 bf16, element e = token slot 16 (e >> 2) + 4 g + (e & 3) of the pair."""
    img = tower._keep["dx0_chn"].view(torch.int16).view(-1, tower.D // 16, 4, 16, 8)
    for gq in range(4):
        for e in range(8):
            if 4 * gq + (e & 3) >= rpt:
                img[:, :, gq, :, e] = 0x3F80
