"""Envelope of the column-split tower path (-m gpu; csrc/split.h, forced on with M2M_SPLIT=1): every case of
tests/split_cases.py -- every split count 2..8, splits of two units (one chunk) and of odd unit counts, all three token classes
of the mix kernels, N = 1..8, ragged row tiles, 1 / 2 / 8 blocks, with and without the final LayerNorm, 64 units per split --
runs forward and backward in training mode and is compared with the oracle evaluated in float64 on the CPU, with the harness
and the bars of tests/test_gpu_shape_envelope.py: the output, dx and every parameter gradient over the whole tensor and over
its tails, and in addition the channel-mixing gradients per 32-channel unit, so that a unit lost at ANY split boundary is a
tail.  m2m_split_form says which path a call takes, so no case can pass through a silent fall-back to the fused kernels; the
slab buffer is the second witness (S slabs written, the rest untouched).

Pairs drive runtime.towers_forward / towers_backward: a groupable pair of unequal towers, pairs that are eligible one by one
but not as a pair (they must run fused and be right, or be refused, never run and be wrong), and the engine whose two modality
towers get different split counts.
"""
import numpy as np
import pytest
import torch

import drop_ref as DR
import gen_util as G
import split_cases as SC
from conftest import observe
from oracle import m2mixer_oracle as O
from test_gpu_shape_envelope import (BF16_GRAD_REL, BF16_REL, case_shapes, dev, kernel_masks, make_input, make_module,  # noqa: F401
                                     oracle, precision, rel, tail_of, tensor_class)

pytestmark = pytest.mark.gpu

NAN0 = 0x7FC00000        # quiet NaN; the low bits carry the element index, so a slab that was moved is seen as well


def p_effective(p):
    return DR.p_effective(p) if p > 0 else 0.0          # the kernels' 16-bit keep probability


def nan_fill(t):
    pat = NAN0 | (torch.arange(t.numel(), device=t.device, dtype=torch.int64) & 0xFFFF)
    t.view(torch.int32).view(-1).copy_(pat.to(torch.int32))
    return t.view(torch.int32).clone()


def rt_masks(rt, B, seed, step):
    """The keep-masks the kernels draw for (seed, step), per block, in the oracle's layout (TowerRuntime.dropout_mask)."""
    m = lambda b, site, *shape: rt.dropout_mask(b, site, B, seed, step).view(*shape).double().cpu()
    return [{"tok_h": m(b, 0, B, rt.D, rt.T), "tok_o": m(b, 1, B, rt.D, rt.N),
             "ch_h": m(b, 2, B, rt.N, rt.Cp)[:, :, :rt.C], "ch_o": m(b, 3, B, rt.N, rt.D)} for b in range(rt.nblocks)]


# A unit slice is measured against its own maximum.  The rounding error of an element of these gradients is set by the TENSOR's
# scale (a sum over the token rows of bf16-rounded terms; about 0.5 % of the tensor's maximum on the fused launch as well), so the
# measure says something about the kernels only where the slice's maximum is comparable with the tensor's.  A slice of 32
# channels always is; the 2 channels that C = 130 leaves in its last unit are not under every dropout draw (their gradient is
# a sum over 21 rows, half of them dropped): one draw gave them a tenth of the tensor's maximum, and 4.2e-3 of the tensor's
# maximum -- the tensor-wide error of that run, on both launches -- was 4.2e-2 of theirs.  The dropout seed of a case is
# therefore the first one whose float64 REFERENCE gradients have every unit slice at a quarter of the tensor's maximum or more
# (nothing the kernels compute enters the choice), and it is fixed from then on: the test is deterministic.
SLICE_MIN = 0.25
DROP_SEEDS = range(100, 116)


def well_conditioned(ref_grads):
    for k, g in ref_grads.items():
        for sl in SC.unit_slices(k, g):
            if float(sl.abs().max()) < SLICE_MIN * float(g.abs().max()):
                return False
    return True


class Report:
    """Collects every miss of a case (the assertion names them all), and records every error (conftest.observe)."""

    def __init__(self, label):
        self.label, self.bad = label, []

    def want(self, kind, got, ref, tol, what, floor=0.0):
        err = rel(got, ref, floor)
        observe(f"{self.label} {kind}", err, tol)
        if not err < tol:
            self.bad.append(f"{what}: {err:.3e} > {tol:.0e} (reference max {float(ref.detach().abs().max()):.3e} over {ref.numel()} elements)")

    def acts(self, what, got, ref):
        self.want(f"{what} (rel to max)", got, ref, BF16_REL, what)
        self.want(f"{what} tail (rel to slice max)", got[-1], ref[-1], BF16_REL, f"{what}[last sample]")
        if got.dim() == 3:
            self.want(f"{what} tail (rel to slice max)", got[:, -1], ref[:, -1], BF16_REL, f"{what}[:, last token]")

    def grad(self, k, got, ref, floor=0.0):
        cls = tensor_class(k)
        self.want(f"{cls} (rel to max)", got, ref, BF16_GRAD_REL, k, floor)
        tg, tr = tail_of(k, got, None), tail_of(k, ref, None)
        if tg is not None:
            self.want(f"{cls} tail (rel to slice max)", tg, tr, BF16_GRAD_REL, f"{k}[tail]", floor)
        for u, (sg, sr) in enumerate(zip(SC.unit_slices(k, got), SC.unit_slices(k, ref))):
            self.want(f"{cls} per 32-channel unit (rel to slice max)", sg, sr, BF16_GRAD_REL, f"{k}[unit {u}]")

    def grads(self, named, ref_of):
        for k, g in named:
            assert g is not None, k
            ref, floor = ref_of(k), 0.0
            if k.endswith("token_mix.2.net.3.bias"):
                # a tower that ends in a LayerNorm removes the shift this bias adds: its true gradient is exactly zero there and
                # is measured against its weight's gradient scale (tests/test_gpu_shape_envelope.py)
                floor = float(ref_of(k[:-4] + "weight").abs().max())
                if float(ref.abs().max()) > 1e-6 * floor:
                    floor = 0.0
            self.grad(k, g, ref, floor)

    def done(self, name):
        assert not self.bad, f"{name} [{self.label}]: " + "; ".join(self.bad)


# ---- single towers through the module path -----------------------------------------------------------------------------------
def train_pass(mod, x, dy, dev):
    mod.zero_grad(set_to_none=True)
    xd = x.to(dev).requires_grad_(True)
    y = mod(xd)
    torch.cuda.synchronize()
    return xd, y


@pytest.mark.parametrize("case", SC.CASES, ids=[c.name for c in SC.CASES])
def test_split_case_vs_float64_oracle(case, dev, precision, monkeypatch):
    precision("bf16")
    monkeypatch.setenv("M2M_SPLIT", "1")
    S, B = SC.EXPECT_S[case.name], case.B
    params = G.make_params(case_shapes(case), 4242)
    rng = np.random.default_rng(977)
    x = make_input(case, rng)
    dy = torch.from_numpy(rng.standard_normal(tuple(x.shape)).astype(np.float32))
    mod = make_module(case).to(dev)
    mod.load_state_dict(params)
    mod.train()
    mod._site_base = 0                       # (a process-wide counter otherwise: the dropout draw would depend on the tests run before)
    # ---- the path the calls will take, before anything runs
    mod._runtime()
    rt = mod._rts[0]
    assert len(mod._rts) == 1
    rt.ensure_buffers(B)
    rt.ensure_workspace(B)
    assert rt.split_form(B, True) == S == SC.split_form(case) and rt.split_form(B, False) == S
    monkeypatch.setenv("M2M_SPLIT", "0")
    assert rt.split_form(B, True) == 0
    monkeypatch.setenv("M2M_SPLIT", "1")
    # ---- float64 oracle on the keep-masks the kernels will draw; the dropout seed: see well_conditioned
    from m2_mixer_amd import config
    step0, drop_p = mod._drop_step, p_effective(case.p)
    for dseed in DROP_SEEDS:
        masks = rt_masks(rt, B, dseed, step0 + 1) if case.p > 0 else None
        leaves = {k: v.double().requires_grad_(True) for k, v in params.items()}
        xr = x.double().requires_grad_(True)
        yo = oracle(case, xr, leaves, drop_p, masks)
        (yo * dy.double()).sum().backward()
        if well_conditioned({k: v.grad for k, v in leaves.items()}) or case.name in SC.INSENSITIVE:
            break                            # (512 slices over 8 rows: some slice is small under every draw; the first seed, fixed)
        assert case.p > 0, "without dropout there is no seed to choose: change the case"
    else:
        raise AssertionError("no dropout seed gives well-conditioned unit slices: change the case")
    print(f"{case.name}: dropout seed {dseed}")
    monkeypatch.setitem(config._state, "seed", dseed)
    # ---- training forward: the slab buffer as a witness
    slabs = rt._keep["split"]["slabs"]
    assert slabs.shape == (SC.NSPLIT, SC.image_rows(B, case.N), case.D)
    before = nan_fill(slabs)
    xd, y = train_pass(mod, x, dy, dev)
    assert rt._keep["split"]["slabs"] is slabs
    assert bool(torch.isfinite(slabs[:S]).all()), "a slab the launch owns was not written in full"
    assert torch.equal(slabs[S:].view(torch.int32), before[S:]), "a slab beyond the split count was written"
    (y * dy.to(dev)).sum().backward()
    torch.cuda.synchronize()
    assert config.dropout_seed() == dseed and mod._drop_step == step0 + (1 if case.p > 0 else 0)
    if case.p > 0:                           # the masks the oracle was given are the masks of the step that ran
        again = kernel_masks(mod, case)
        assert all(torch.equal(a[k], b[k]) for a, b in zip(again, masks) for k in a)
    rep = Report("split bf16")
    rep.acts("out", y, yo)
    rep.acts("dx", xd.grad, xr.grad)
    rep.grads([(k, p.grad) for k, p in mod.named_parameters()], lambda k: leaves[k].grad)
    rep.done(case.name)
    split_out = (y.detach().clone(), xd.grad.clone(), {k: p.grad.clone() for k, p in mod.named_parameters()})
    # ---- the same step on the fused launch (same dropout step: same masks), against the same oracle
    monkeypatch.setenv("M2M_SPLIT", "0")
    mod._drop_step = step0
    if SC.padC(case.C) > 4096:                 # beyond the fused launch's channel_dim: nothing to compare with
        with pytest.raises(RuntimeError, match="exceed the workgroup's LDS"):
            train_pass(mod, x, dy, dev)
    else:
        xf, yf = train_pass(mod, x, dy, dev)
        (yf * dy.to(dev)).sum().backward()
        torch.cuda.synchronize()
        rep = Report("fused bf16 (split cases)")
        rep.acts("out", yf, yo)
        rep.acts("dx", xf.grad, xr.grad)
        rep.grads([(k, p.grad) for k, p in mod.named_parameters()], lambda k: leaves[k].grad)
        rep.done(case.name)
        # (they differ by the GELU table form and by summation order: recorded, held to nothing tighter than the oracle bars)
        observe("split vs fused bf16 out (rel to max)", rel(split_out[0], yf), 2 * BF16_REL)
        observe("split vs fused bf16 dx (rel to max)", rel(split_out[1], xf.grad), 2 * BF16_REL)
        for k, p in mod.named_parameters():
            if not k.endswith("token_mix.2.net.3.bias"):
                observe(f"split vs fused bf16 {tensor_class(k)} (rel to max)", rel(split_out[2][k], p.grad), 2 * BF16_GRAD_REL)
    # ---- evaluation forward: no dropout, no saved activations, the carry rewritten in place
    monkeypatch.setenv("M2M_SPLIT", "1")
    mod.eval()
    assert rt.split_form(B, False) == S
    with torch.no_grad():
        ye = mod(x.to(dev))
        yoe = oracle(case, x.double(), {k: v.double() for k, v in params.items()}, 0.0, None)
    torch.cuda.synchronize()
    rep = Report("split bf16 eval")
    rep.acts("out", ye, yoe)
    rep.done(case.name)


@pytest.mark.parametrize("name,prec,case,fused_refuses", SC.REFUSED, ids=[r[0] for r in SC.REFUSED])
def test_shapes_outside_the_path_take_the_other_launch(name, prec, case, fused_refuses, dev, precision, monkeypatch):
    """M2M_SPLIT=1 does not pull a shape onto the path that it cannot run: the query says 0, and the call runs fused / wide and
    is right (output against float64) -- or, beyond the fused launch's channel_dim too, is refused outright."""
    precision(prec)
    monkeypatch.setenv("M2M_SPLIT", "1")
    params = G.make_params(case_shapes(case), 4242)
    x = make_input(case, np.random.default_rng(977))
    mod = make_module(case).to(dev)
    mod.load_state_dict(params)
    mod.eval()
    mod._runtime()
    rt = mod._rts[0]
    rt.ensure_buffers(case.B)
    rt.ensure_workspace(case.B)
    assert rt.split_form(case.B, True) == 0 and rt.split_form(case.B, False) == 0 and SC.split_form(case, prec=prec) == 0
    if fused_refuses:
        with pytest.raises(RuntimeError, match="exceed the workgroup's LDS"):
            with torch.no_grad():
                mod(x.to(dev))
        return
    with torch.no_grad():
        y = mod(x.to(dev))
    torch.cuda.synchronize()
    yo = oracle(case, x.double(), {k: v.double() for k, v in params.items()}, 0.0, None)
    tol = BF16_REL if prec == "bf16" else 1e-4
    assert rel(y, yo) < tol


def test_min_rows_threshold_is_exact(dev, precision, monkeypatch):
    """M2M_SPLIT_MIN_ROWS takes the path exactly from B N == threshold on (asked of m2m_split_form; nothing is launched)."""
    precision("bf16")
    monkeypatch.delenv("M2M_SPLIT", raising=False)
    case = SC.CASES[1]                                       # N = 3, B = 7: 21 rows
    mod = make_module(case).to(dev)
    mod._runtime()
    rt = mod._rts[0]
    rt.ensure_buffers(case.B)
    rt.ensure_workspace(case.B)
    rows = case.B * case.N
    assert rt.split_form(case.B) == 0                         # off by default
    for thr, want in ((rows + 1, 0), (rows, 2), (rows - 1, 2), (1, 2)):
        monkeypatch.setenv("M2M_SPLIT_MIN_ROWS", str(thr))
        assert rt.split_form(case.B) == want == SC.split_form(case, mode=-1, min_rows=thr), thr
    monkeypatch.setenv("M2M_SPLIT", "0")
    assert rt.split_form(case.B) == 0


# ---- pairs through runtime.towers_forward / towers_backward ------------------------------------------------------------------
SEED = 1234


class PairTower:
    """One tower (blocks + optional final LayerNorm) driven through the runtime, with its float64 twin.

    Defaults: a FusionMixer-shaped bf16 tower on dense buffers, fed `parts` k-split input parts and read out through its output
    or (pooled) its token mean.  tests/test_gpu_tower_io.py also sets has_final_ln, the precision, pads (floats behind every
    sample of x0 / out / d_out / d_x0, filled with the index-carrying NaN of nan_fill) and inputs = (params, xparts, d_out,
    d_pooled) of its own; `up` then names the upstream gradients the backward is given ("out", "pooled", "both", "none")."""

    def __init__(self, tow, seed, site_base, dev, parts=1, pooled=False, has_final_ln=True, prec="bf16", pads=None, inputs=None,
                 up=None):
        from m2_mixer_amd import _lib as L
        from m2_mixer_amd.runtime import BLOCK_FIELDS, BLOCK_KEYS, TowerRuntime
        self.tow, self.parts, self.pooled, self.dev, self.has_final_ln = tow, parts, pooled, dev, has_final_ln
        self.up_form = up if up is not None else ("pooled" if pooled else "out")
        cfg = dict(hidden_dim=tow.D, token_dim=tow.T, channel_dim=tow.C, num_mixers=tow.nb)
        self.keys = [f"mixer_blocks.{i}.{BLOCK_KEYS[f]}" for i in range(tow.nb) for f in BLOCK_FIELDS]
        self.keys += ["layer_norm.weight", "layer_norm.bias"] if has_final_ln else []
        B, N, D = tow.B, tow.N, tow.D
        if inputs is None:
            params = G.make_params(G.tower_shapes("", cfg, tow.N, "none"), seed)
            rng = np.random.default_rng(seed + 1)
            f32 = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
            xparts = f32(parts, B, N, D)                         # the tower input is the sum of the parts
            up_t = f32(B, D) if pooled else f32(B, N, D)         # upstream gradient (of the token mean, or of the output)
            d_out, d_pool = (None, up_t) if pooled else (up_t, None)
        else:
            params, xparts, d_out, d_pool = inputs
            xparts = xparts[:parts]
        self.params = {k: params[k] for k in self.keys}
        self.dparams = {k: v.to(dev) for k, v in self.params.items()}
        self.rt = rt = TowerRuntime(tow.D, tow.N, tow.T, tow.C, tow.nb, has_final_ln, tow.p, L.PREC_BY_NAME[prec], site_base)
        blocks = [{f: self.dparams[f"mixer_blocks.{i}.{BLOCK_KEYS[f]}"] for f in BLOCK_FIELDS} for i in range(tow.nb)]
        rt.bind_params(blocks, (self.dparams["layer_norm.weight"], self.dparams["layer_norm.bias"]) if has_final_ln else None)
        rt.pack(force=True)
        self.flat = torch.zeros(rt.grad_numel(), device=dev)
        self.views = rt.bind_grads(self.flat)
        self.xparts, self.d_out, self.d_pool = xparts, d_out, d_pool
        self.up = d_pool if pooled else d_out
        pads = dict(pads or {})
        # every caller buffer: (.., B, N D + pad) storage, the (.., B, N, D) view the samples live in, the sample stride
        self.bufs, self.before = {}, {}
        self.xdev, self.x_ss = self._buffer("x0", pads, xparts)
        self.out, self.out_ss = self._buffer("out", pads, torch.zeros(B, N, D))
        self.dx, self.dx_ss = self._buffer("d_x0", pads, torch.zeros(B, N, D))
        self.d_out_dev, self.d_out_ss = self._buffer("d_out", pads, d_out) if d_out is not None else (None, N * D)
        self.d_pool_dev = d_pool.to(dev) if d_pool is not None else None
        self.updev = self.d_pool_dev if pooled else self.d_out_dev
        self.pool = torch.zeros(B, D, device=dev)
        rt.ensure_buffers(B)
        rt.ensure_workspace(B)

    def _buffer(self, name, pads, values):
        N, D = self.tow.N, self.tow.D
        pad = pads.get(name, 0)
        buf = torch.zeros(*values.shape[:-2], N * D + pad, device=self.dev)
        self.before[name] = nan_fill(buf) if pad else None
        view = buf[..., :N * D].view(*values.shape)
        view.copy_(values.to(self.dev))
        self.bufs[name] = buf
        return view, N * D + pad

    def pads_untouched(self, name):
        """Every pad word of a strided buffer still holds the bits it was filled with."""
        n = self.tow.N * self.tow.D
        return self.before[name] is None or torch.equal(self.bufs[name].view(torch.int32)[..., n:], self.before[name][..., n:])

    def fwd_io(self):
        B = self.tow.B
        return (self.xdev, self.x_ss, self.out, self.out_ss, self.pool if self.pooled else None, self.parts, B * self.x_ss)

    def bwd_io(self):
        d_out = self.d_out_dev if self.up_form in ("out", "both") else None
        d_pool = self.d_pool_dev if self.up_form in ("pooled", "both") else None
        return (d_out, self.d_out_ss, d_pool, self.dx, self.dx_ss)

    def result(self):
        return (self.pool if self.pooled else self.out).clone(), self.dx.clone(), self.flat.clone()

    def reset(self, value=0.0):
        for t in (self.flat, self.dx, self.out, self.pool):
            t.fill_(value)

    def check(self, label, name, step):
        """Output (or the token mean), dx and every parameter gradient against float64."""
        tow, rt = self.tow, self.rt
        masks = rt_masks(rt, tow.B, SEED, step) if tow.p > 0 else None
        leaves = {k: v.double().requires_grad_(True) for k, v in self.params.items()}
        xr = self.xparts.double().sum(0).requires_grad_(True)
        yo = O.fusion_mixer(xr, leaves, "", tow.nb, p_effective(tow.p), masks)
        res = yo.mean(1) if self.pooled else yo
        (res * self.up.double()).sum().backward()
        rep = Report(label)
        rep.acts("out", self.pool if self.pooled else self.out, res)
        rep.acts("dx", self.dx, xr.grad)
        rep.grads(list(zip(self.keys, self.views)), lambda k: leaves[k].grad)
        rep.done(name)


def pair_step(towers, B, step, group_wgrad=True):
    from m2_mixer_amd.runtime import towers_backward, towers_forward, towers_wgrad
    rts = [t.rt for t in towers]
    towers_forward(rts, [t.fwd_io() for t in towers], B, True, SEED, step)
    towers_backward(rts, [t.bwd_io() for t in towers], B, SEED, step)
    if group_wgrad:
        towers_wgrad(rts, B, seed=SEED, step=step)
    else:
        for rt in rts:
            rt.wgrad(B, SEED, step)
    torch.cuda.synchronize()


def test_pair_of_unequal_towers_shares_the_split_launches(dev, precision, monkeypatch):
    """Two towers of unequal unit counts (5 and 4) and unequal row-tile counts (1 and 2: the shorter tower's workgroups of the
    second row tile return at once), one fed two k-split input parts, the other read out through its token mean.

    Against the two single-tower split launches on the same inputs the comparison is BIT EQUALITY, from reading the kernels: a
    grouped launch picks a tower's own argument block (a.t[blockIdx.y] in the mix launches, a.t[(id / nsplit) % ntow] in the
    chain launches) and then runs the same code over the same row tiles and unit ranges; nothing is summed across towers, a
    slab has one writer, and the slot reduction adds a tower's tiles in the same order.  The sum of the two input parts is one
    fp32 add per element in the kernel and in the test.  The weight gradients are taken with the single-tower launch in both
    runs, so that the comparison holds nothing but the split launches."""
    precision("bf16")
    monkeypatch.setenv("M2M_SPLIT", "1")
    ta, tb = SC.PAIR_UNEQUAL
    B = ta.B
    a = PairTower(ta, 31, 0, dev, parts=2)
    b = PairTower(tb, 41, 1024, dev, pooled=True)
    assert a.rt.split_form(B, True, b.rt) == 2 == SC.split_form(ta, tb) and b.rt.split_form(B, True, a.rt) == 2
    pair_step([a, b], B, step=3, group_wgrad=False)
    a.check("split pair bf16", "pair_unequal[0]", 3)
    b.check("split pair bf16", "pair_unequal[1]", 3)
    grouped = [a.result(), b.result()]
    # ---- each tower alone, same inputs and dropout stream
    for t, g in zip((a, b), grouped):
        t.reset()
        xsum = t.xdev[0] + t.xdev[1] if t.parts == 2 else t.xdev[0]
        N, D = t.tow.N, t.tow.D
        assert t.rt.split_form(B, True) == 2
        t.rt.forward(xsum.contiguous(), N * D, B, t.out, N * D, t.pool if t.pooled else None, True, SEED, 3)
        d_out, _, d_pool, dx, _ = t.bwd_io()
        t.rt.backward(B, d_out, N * D, d_pool, dx, N * D, SEED, 3)
        t.rt.wgrad(B, SEED, 3)
        torch.cuda.synchronize()
        for what, got, ref in zip(("out", "dx", "grads"), t.result(), g):
            observe(f"split pair vs single bf16 {what} (rel to max)", rel(ref, got), 1e-30)
            assert torch.equal(got, ref), what


NOT_GROUPABLE = dict(SC.PAIR_NOT_GROUPABLE, mixed=SC.PAIR_MIXED)


@pytest.mark.parametrize("form", sorted(NOT_GROUPABLE))
def test_pairs_that_cannot_share_the_split_launches(form, dev, precision, monkeypatch):
    """Towers that are eligible one by one but not as a pair (and an eligible tower beside one that is not): the pair takes the
    fused launch and must match float64 completely, m2m_towers_wgrad included -- or, where the fused pair launch has no shared
    instantiation either (N <= 4 beside N > 4), is refused by the forward.  With M2M_WGRAD_REDUCES_SMALL on an eligible tower
    the backward returns its documented refusal and touches no gradient."""
    from m2_mixer_amd.runtime import can_group, towers_backward, towers_forward
    precision("bf16")
    monkeypatch.setenv("M2M_SPLIT", "1")
    ta, tb = NOT_GROUPABLE[form]
    B = ta.B
    a, b = PairTower(ta, 51, 0, dev), PairTower(tb, 61, 1024, dev)
    assert a.rt.split_form(B, True) == SC.split_form(ta) == 2
    assert b.rt.split_form(B, True) == SC.split_form(tb)
    assert a.rt.split_form(B, True, b.rt) == 0 == SC.split_form(ta, tb) and b.rt.split_form(B, True, a.rt) == 0
    if not can_group(a.rt, b.rt, B):
        assert form == "token_class"
        with pytest.raises(RuntimeError, match="launch them separately"):
            towers_forward([a.rt, b.rt], [a.fwd_io(), b.fwd_io()], B, True, SEED, 5)
        return
    pair_step([a, b], B, step=5)
    a.check("fused pair bf16 (split-eligible towers)", f"{form}[0]", 5)
    b.check("fused pair bf16 (split-eligible towers)", f"{form}[1]", 5)
    # ---- the flag whose reduction the weight-gradient launch would skip for an eligible tower: refused, nothing written
    a.rt.set_wgrad_reduces_small(True)
    towers_forward([a.rt, b.rt], [a.fwd_io(), b.fwd_io()], B, True, SEED, 6)
    for t in (a, b):
        t.flat.fill_(-7.25)
        t.dx.fill_(-7.25)
    with pytest.raises(RuntimeError, match="eligible for the column-split path but its partner is not"):
        towers_backward([a.rt, b.rt], [a.bwd_io(), b.bwd_io()], B, SEED, 6)
    torch.cuda.synchronize()
    for t in (a, b):
        assert bool((t.flat == -7.25).all()) and bool((t.dx == -7.25).all())


def test_engine_with_two_split_counts_is_refused_at_its_first_step(dev, monkeypatch):
    """An AV-MNIST engine at hidden_dim 128 whose image and audio towers get different split counts under M2M_SPLIT=1 (channel_dim
    128: S = 2; 512: S = 8).  The engine launches the two as a pair and defers their slot reductions to the weight-gradient
    launch (M2M_WGRAD_REDUCES_SMALL); the pair cannot share the split launches, so its first step raises the library's refusal
    instead of losing the towers' LayerNorm / token-MLP / ch_b2 gradients.  INTEGRATION.md's switch list says so."""
    from m2_mixer_amd.engine import AVMnistEngine
    monkeypatch.setenv("M2M_SPLIT", "1")
    tower = lambda patch, size, C: dict(in_channels=1, hidden_dim=128, patch_size=patch, image_size=[size, size], token_dim=16,
                                        channel_dim=C, num_mixers=1)
    cfg = dict(dropout=0.0, num_classes=10, image=tower(14, 28, 128), audio=tower(56, 112, 512),
               multimodal=dict(hidden_dim=128, token_dim=16, channel_dim=128, num_mixers=1))
    B = 4
    eng = AVMnistEngine(cfg, B, device=dev, precision="bf16", lr=1e-2, init=False)
    eng.load_state_dict(dict(G.make_params(G.avmnist_shapes(cfg), 7)))
    for t in (eng.t_a, eng.t_b):
        t.ensure_buffers(B)
        t.ensure_workspace(B)
    assert eng.t_a.split_form(B) == 2 and eng.t_b.split_form(B) == 8 and eng.t_a.split_form(B, True, eng.t_b) == 0
    image, audio, labels = (t.to(dev) for t in G.avmnist_batch(B, 8, cfg))
    with pytest.raises(RuntimeError, match="eligible for the column-split path but its partner is not"):
        eng.forward_backward(image, audio, labels)
    torch.cuda.synchronize()
