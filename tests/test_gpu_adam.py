"""m2m_adam_step, m2m_adam_step_bf16 and m2m_adam_step_ranges called directly (-m gpu), against float64 Adam on the same
inputs (tests/leaf_ref.py, pinned to torch.optim.Adam in float64), one engine-level run of both update forms with
weight_decay != 0 and non-default betas / eps, and the one-launch update (m2m_adam_pack_all) held bit for bit to the flat Adam +
m2m_pack_all in the builds tests/test_gpu_bench_path.py does not reach (hidden_dim 32 / 64 / 256, fp32, both tile forms).

Bars.  For each tensor (param, exp_avg, exp_avg_sq) two errors are taken against float64 on the same inputs, each relative to the
tensor's max: the kernel's, and that of torch.optim.Adam on float32 CPU tensors.  The kernel is held to
8 x max(float32-torch error, 2^-24): the margin of 8 covers the kernel's operation order, its fma and its powf; the floor is the
half-ulp a float32 result carries at the tensor's max, below which the float32-torch error of a short tensor can fall by luck
(n = 1) and which no float32 implementation can be held under.  Both numbers go through conftest.observe.

exp_avg_sq carries one term more.  The kernels form 1 - beta2 as the float difference 1.0f - beta2 (0.00099998713 for 0.999f);
torch.optim.Adam forms it in double and rounds once (0.001f).  The library keeps its form: forming it torch's way moves every
exp_avg_sq by 1.3e-5 relative, and with it every training run's parameters, away from what the library has computed so far,
for a gain no training result shows; and the C ABI carries beta as a float, so the double the caller meant can only be guessed.
What that arithmetic predicts is exact to first order: each step adds delta2 * (1 - beta2) * g^2 to the element's error,
    delta2 = |fl32(1 - fl32(beta2)) - (1 - beta2)| / (1 - beta2)        (1.29e-5 at beta2 = 0.999, 2.4e-7 at 0.95),
and the steps before it decay by beta2 (Run.follow accumulates it in float64 beside the reference; all terms are >= 0, so it
never exceeds delta2 * exp_avg_sq).  exp_avg_sq is held to 8 x max(float32-torch error, 2^-24) + that predicted deviation,
relative to the tensor's max: the margin of 8 stays on the rounding error alone, the predicted term enters once, so this is
below 8 x (rounding + prediction).  param and exp_avg keep the plain bar (the same difference in 1 - beta1 is 2.4e-7 at 0.9).

Observed on an MI355X (largest over the cases; float32 torch | kernel, both against float64, relative to the tensor's max):
    m2m_adam_step / _ranges   param 1.44e-7 | 1.47e-7    exp_avg 4.47e-7 | 5.57e-7
    m2m_adam_step_bf16        param 1.38e-7 | 1.26e-7    exp_avg 1.33e-7 | 2.15e-7
    t = 1000                  param 3.27e-8 | 5.65e-8    exp_avg 6.93e-8 | 6.66e-8
    exp_avg_sq at the default betas: float32 torch 1.38e-7 | kernel 1.29e-5, the prediction 1.287e-5 (bar 1.3e-5 to 1.4e-5)."""
import pytest
import torch

import gen_util as G
import leaf_ref as R
from conftest import observe
from oracle import m2mixer_oracle as O

pytestmark = pytest.mark.gpu

MARGIN = 8.0
FLOOR = 2.0 ** -24
DEFAULTS = dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0)
OTHER = dict(betas=(0.8, 0.95), eps=1e-3, weight_decay=1e-2, grad_scale=0.5)
LR = 1e-2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from m2_mixer_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def relmax(a, ref):
    ref = R.f64(ref)
    return float((R.f64(a) - ref).abs().max()) / (float(ref.abs().max()) + 1e-300)


def delta_one_minus(beta):
    """|fl32(1 - fl32(beta)) - (1 - beta)| / (1 - beta): how far the kernels' float difference 1.0f - beta lies from 1 - beta."""
    b32 = torch.tensor(beta, dtype=torch.float32)
    return abs(float((1.0 - b32).double()) - (1.0 - beta)) / (1.0 - beta)


def hold(kind, got, t32, ref, predicted_v=0.0):
    """The kernel's (param, exp_avg, exp_avg_sq) against float64, at MARGIN x the float32-torch error; exp_avg_sq with the
    deviation the float difference 1.0f - beta2 predicts (relative to the tensor's max) on top."""
    for name, g, t, r in zip(("param", "exp_avg", "exp_avg_sq"), got, t32, ref):
        e32 = relmax(t, r)
        bar = MARGIN * max(e32, FLOOR)
        if name == "exp_avg_sq":
            observe(f"adam {kind} {name}: predicted by 1.0f - beta2 (rel to max)", predicted_v, bar + predicted_v)
            bar += predicted_v
        observe(f"adam {kind} {name}: float32 torch (rel to max)", e32, bar)
        assert observe(f"adam {kind} {name}: kernel (rel to max)", relmax(g, r), bar) < bar, (kind, name, e32)


class Run:
    """Device buffers of one flat segment + the float64 and float32-torch states that follow it."""

    def __init__(self, n, dev, seed, step0=0, preset=False):
        gen = torch.Generator().manual_seed(seed)
        self.n, self.dev, self.gen = n, dev, gen
        p = torch.randn(n, generator=gen)
        m = 0.01 * torch.randn(n, generator=gen) if preset else torch.zeros(n)
        v = 1e-3 * torch.rand(n, generator=gen) if preset else torch.zeros(n)
        self.p, self.m, self.v = (t.to(dev) for t in (p, m, v))
        self.g = torch.zeros(n, device=dev)
        self.state = torch.tensor([float(step0), LR, 0.0, 0.0], device=dev)
        self.ref = (p.double(), m.double(), v.double())
        self.t32 = (p.clone(), m.clone(), v.clone())
        self.step = step0
        self.dev_v = torch.zeros(n, dtype=torch.float64)     # what the float difference 1.0f - beta2 predicts for exp_avg_sq

    def new_grad(self, bf16=False):
        g = 0.1 * torch.randn(self.n, generator=self.gen)
        self.g.copy_(g)
        self.gb = g.to(torch.bfloat16).to(self.dev) if bf16 else None
        return self.gb.float().cpu() if bf16 else g          # the values the update consumes

    def follow(self, g_eff, hp):
        self.step += 1
        b2 = hp["betas"][1]
        g_tot = g_eff.double() * abs(hp["grad_scale"]) + hp["weight_decay"] * self.ref[0]
        self.dev_v = b2 * self.dev_v + delta_one_minus(b2) * (1.0 - b2) * g_tot * g_tot
        self.ref = R.adam(self.ref[0], g_eff, self.ref[1], self.ref[2], self.step, LR, **hp)
        self.t32 = R.adam_torch(self.t32[0], g_eff, self.t32[1], self.t32[2], self.step, LR, dtype=torch.float32, **hp)

    def predicted_v(self):
        return float(self.dev_v.max()) / float(self.ref[2].abs().max())

    def got(self):
        torch.cuda.synchronize()
        return self.p, self.m, self.v


def call(run, variant, hp, consume, bump=1, lo=0, n=None, ranges=None):
    """One library call on elements [lo, lo + n) of the run's buffers."""
    from m2_mixer_amd import _lib as L
    n = run.n - lo if n is None else n
    off = 4 * lo
    scale = -hp["grad_scale"] if consume else hp["grad_scale"]
    tail = (run.state.data_ptr(), hp["betas"][0], hp["betas"][1], hp["eps"], hp["weight_decay"], scale, bump)
    bufs = (run.p.data_ptr() + off, run.g.data_ptr() + off)
    mv = (run.m.data_ptr() + off, run.v.data_ptr() + off)
    gb = run.gb.data_ptr() + 2 * lo if run.gb is not None else 0
    if variant == "step":
        return L.lib().m2m_adam_step(*bufs, *mv, n, *tail, L.stream_ptr())
    if variant == "bf16":
        return L.lib().m2m_adam_step_bf16(*bufs, gb, *mv, n, *tail, L.stream_ptr())
    arr = (L.GradRange * max(1, len(ranges or [])))()
    for i, (rlo, rn, add, keep) in enumerate(ranges or []):
        arr[i].lo, arr[i].n, arr[i].add, arr[i].keep = rlo, rn, add, keep
    return L.lib().m2m_adam_step_ranges(*bufs, gb, *mv, n, *tail, arr, len(ranges or []), L.stream_ptr())


@pytest.mark.parametrize("n", [1, 255, 1024, 1025, 100003])
@pytest.mark.parametrize("hp", [DEFAULTS, OTHER], ids=["defaults", "wd"])
@pytest.mark.parametrize("variant", ["step", "bf16", "ranges"])
def test_three_steps_from_zero_moments(variant, hp, n, dev):
    """Three consecutive steps (bias corrections at t = 1, 2, 3), compared after each.  Steps 1 and 3 consume the gradient
    (negative grad_scale: cleared afterwards), step 2 leaves it in place (positive).  bf16: the gradient VALUES come from the
    bf16 copy (the float64 reference reads the same values widened) and the fp32 gradient is only cleared."""
    run = Run(n, dev, 100 + n)
    for step in (1, 2, 3):
        g_eff = run.new_grad(bf16=variant == "bf16")
        before = run.g.clone()
        consume = step != 2
        assert call(run, variant, hp, consume, ranges=[]) == 0
        run.follow(g_eff, hp)
        hold(f"{variant}", run.got(), run.t32, run.ref, run.predicted_v())
        assert float(run.state[0]) == step
        assert float(run.g.abs().max()) == 0.0 if consume else torch.equal(run.g, before)


@pytest.mark.parametrize("hp", [DEFAULTS, OTHER], ids=["defaults", "wd"])
@pytest.mark.parametrize("variant", ["step", "bf16"])
def test_step_1000_from_nonzero_moments(variant, hp, dev):
    """state[0] preset to 999, non-zero moments: the bias corrections 1 - beta^t at t = 1000."""
    run = Run(1025, dev, 7, step0=999, preset=True)
    g_eff = run.new_grad(bf16=variant == "bf16")
    assert call(run, variant, hp, True) == 0
    run.follow(g_eff, hp)
    hold(f"{variant} t=1000", run.got(), run.t32, run.ref, run.predicted_v())
    assert float(run.state[0]) == 1000.0


@pytest.mark.parametrize("hp", [DEFAULTS, OTHER], ids=["defaults", "wd"])
def test_one_bump_for_a_step_applied_as_three_calls(hp, dev):
    """A step over three disjoint segments (unaligned boundaries): the first call bumps state[0], the others do not; then n = 0
    with bump only bumps."""
    run = Run(100003, dev, 9)
    g_eff = run.new_grad()
    for i, (lo, n) in enumerate(((0, 1001), (1001, 49000), (50001, 100003 - 50001))):
        assert call(run, "step", hp, True, bump=int(i == 0), lo=lo, n=n) == 0
    run.follow(g_eff, hp)
    hold("segments", run.got(), run.t32, run.ref, run.predicted_v())
    assert float(run.state[0]) == 1.0 and float(run.g.abs().max()) == 0.0
    keep = [t.clone() for t in (run.p, run.m, run.v)]
    assert call(run, "step", hp, True, bump=1, n=0) == 0
    torch.cuda.synchronize()
    assert float(run.state[0]) == 2.0 and all(torch.equal(a, b) for a, b in zip(keep, (run.p, run.m, run.v)))


# ranges on n = 5000: 1024-element chunks [0, 1024) ... [4096, 5000)
RANGE_SETS = {
    "whole chunks": [(1024, 2048)],
    "mid-chunk ends": [(100, 500), (3000, 1500)],
    "adjacent mid-chunk": [(2100, 400), (2500, 400)],
    "zero length": [(777, 0), (4090, 10)],
    "sixteen": [(7 + 300 * i, 50 + 10 * i) for i in range(16)],
}


@pytest.mark.parametrize("mode,bf16", [("add", False), ("keep", False), ("both", False), ("both", True)],
                         ids=["add", "keep", "both", "both + bf16 grad"])
@pytest.mark.parametrize("which", list(RANGE_SETS))
def test_ranges_add_and_keep(which, mode, bf16, dev):
    """Inside a range the gradient is grad + add (add mode) and / or is not cleared (keep mode); chunks wholly inside a range
    take the uniform path, chunks that straddle a boundary the element-by-element one.  Afterwards exactly the elements outside
    the keep ranges are cleared and the kept ones hold their old values.  (`both`: every other range keeps; once more with the
    gradient values read from a bf16 copy.)"""
    n, hp = 5000, OTHER
    run = Run(n, dev, 300 + len(which), step0=4, preset=True)
    g_eff = run.new_grad(bf16=bf16).clone()
    before = run.g.clone()
    ranges, adds, kept = [], [], torch.zeros(n, dtype=torch.bool)
    for i, (lo, rn) in enumerate(RANGE_SETS[which]):
        add_ptr, keep = 0, int(mode in ("keep", "both") and (mode == "keep" or i % 2 == 0))
        if mode in ("add", "both"):
            a = 0.05 * torch.randn(rn, generator=run.gen)
            buf = torch.zeros(rn + 4, device=dev)                    # lo % 4 floats of lead padding (the header's alignment rule)
            buf[lo % 4:lo % 4 + rn] = a.to(dev)
            adds.append(buf)
            add_ptr = buf.data_ptr() + 4 * (lo % 4)
            g_eff[lo:lo + rn] = g_eff[lo:lo + rn] + a                # one fp32 add, as the kernel forms it
        if keep:
            kept[lo:lo + rn] = True
        ranges.append((lo, rn, add_ptr, keep))
    assert call(run, "ranges", hp, True, ranges=ranges) == 0
    run.follow(g_eff, hp)
    hold("ranges", run.got(), run.t32, run.ref, run.predicted_v())
    g_after = run.g.cpu()
    assert torch.equal(g_after[kept], before.cpu()[kept]) and float(g_after[~kept].abs().max()) == 0.0
    assert float(before.cpu()[kept].abs().min()) > 0.0 if bool(kept.any()) else True


@pytest.mark.parametrize("what", ["past the end", "negative lo", "seventeen ranges"])
def test_bad_ranges_are_refused_before_anything_runs(what, dev):
    run = Run(5000, dev, 11, step0=3, preset=True)
    run.new_grad()
    ranges = {"past the end": [(4000, 1001, 0, 1)], "negative lo": [(-1, 10, 0, 1)], "seventeen ranges": [(10 * i, 5, 0, 1) for i in range(17)]}[what]
    keep = [t.clone() for t in (run.p, run.g, run.m, run.v, run.state)]
    from m2_mixer_amd import _lib as L
    assert call(run, "ranges", DEFAULTS, True, bump=1, ranges=ranges) == -1 and len(L.lib().m2m_last_error()) > 0
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(keep, (run.p, run.g, run.m, run.v, run.state)))      # the step count included


@pytest.mark.parametrize("fused_update", ["0", "1"])
def test_engine_update_with_weight_decay_vs_oracle(fused_update, dev, monkeypatch):
    """AV-MNIST S, B = 8, fp32, weight_decay 1e-2, betas (0.8, 0.95), eps 1e-6: two training steps in both update forms (the flat
    Adam + re-pack, and the one-launch m2m_adam_pack_all -- the only run of ITS weight-decay line) against
    oracle.avmnist_train_step with the same hyper-parameters, at the bars of
    tests/test_gpu_bench_path.py::test_adam_moments_and_parameters_vs_oracle, with the gradient Adam consumes (g + wd * p) in
    place of g."""
    from m2_mixer_amd.engine import AVMnistEngine
    monkeypatch.setenv("M2M_FUSED_UPDATE", fused_update)
    wd, betas, eps, B = 1e-2, (0.8, 0.95), 1e-6, 8
    cfg = dict(G.AVMNIST["S"], dropout=0.0)
    eng = AVMnistEngine(cfg, B, device=dev, precision="fp32", lr=1e-2, betas=betas, eps=eps, weight_decay=wd, init=False)
    assert bool(eng._fused_update) == (fused_update == "1")
    shapes = G.avmnist_shapes(cfg)
    params = dict(G.make_params(shapes, 11))
    eng.load_state_dict(params)
    image, audio, labels = G.avmnist_batch(B, 12, cfg)
    gb = (image.to(dev), audio.to(dev), labels.to(dev))
    state, significant = {}, {k: torch.ones(s, dtype=torch.bool) for k, s in shapes.items()}
    for step in (1, 2):
        prev = {k: v.clone() for k, v in params.items()}
        ref = O.avmnist_train_step(image, audio, labels, params, cfg, state, lr=1e-2, betas=betas, eps=eps, weight_decay=wd)
        eng.train_step(*gb)
        torch.cuda.synchronize()
        assert float(eng.adam_state[0]) == step
        for k in shapes:
            if k.endswith("token_mix.2.net.3.bias"):
                continue
            g = ref["grads"][k] + wd * prev[k]
            gmax = float(g.abs().max())
            em = float((eng.exp_avg[k].cpu() - state["m"][k]).abs().max())
            ev = float((eng.exp_avg_sq[k].cpu() - state["v"][k]).abs().max())
            assert observe("adam engine wd exp_avg (rel to max g)", em / max(gmax, 1e-6), 1e-3) < 1e-3, (step, k)
            assert observe("adam engine wd exp_avg_sq (rel to max g^2)", ev / max(gmax * gmax, 1e-12), 2e-3) < 2e-3, (step, k)
            significant[k] &= g.abs() > max(1e-6, 5e-3 * gmax)
            sel = significant[k]
            if bool(sel.any()):
                err = float((eng.params[k].cpu() - params[k])[sel].abs().max())
                assert observe("adam engine wd params (abs)", err, 3e-4) < 3e-4, (step, k, err)
    assert sum(int(v.sum()) for v in significant.values()) > 0.3 * eng.n_params


# (engine, hidden_dim, channel_dim, precision, M2M_AP_ROWTILES or None: the tower is too narrow for row tiles either way).
# The one-launch update is compiled once per hidden_dim every tower of the launch shares (64, 128, 256) plus once for any other
# (32); tests/test_gpu_bench_path.py holds the 128 / bf16 build to this check, these are the others at their smallest shapes.
# channel_dim 33 -> Cp 64: one full and one ragged 32-column group (the float4 path and the element tail); 518 -> Cp 544: past the
# 512-column chunk of the row-tile form (bf16 only), one full and one ragged chunk.
UPDATE_FORMS = [("avmnist", 32, 33, "fp32", None), ("avmnist", 32, 33, "bf16", None),
                ("avmnist", 64, 33, "fp32", None), ("avmnist", 64, 33, "bf16", None),
                ("mmimdb", 256, 33, "fp32", None), ("mmimdb", 256, 33, "bf16", None),
                ("avmnist", 64, 518, "bf16", "1"), ("avmnist", 64, 518, "bf16", "0"),
                ("mmimdb", 256, 518, "bf16", "1"), ("mmimdb", 256, 518, "bf16", "0")]


@pytest.mark.parametrize("engine,D,C,prec,rowtiles", UPDATE_FORMS,
                         ids=[f"{e}-d{D}-c{C}-{p}" + ("" if r is None else f"-rowtiles{r}") for e, D, C, p, r in UPDATE_FORMS])
def test_one_launch_update_is_bit_identical_to_adam_then_repack(engine, D, C, prec, rowtiles, dev, monkeypatch):
    """Two training steps with the one-launch Adam + re-pack (M2M_FUSED_UPDATE=1) against the flat Adam followed by
    m2m_pack_all (0) on engines loaded with the same state: one block per tower, images (8, 8) and (16, 16), batch 5.  Same
    arithmetic per element, so everything the update writes must agree bit for bit.  The reference side is the flat Adam,
    which the tests above hold to float64.

    Both updates of a step consume the SAME gradient: the one-launch engine's backward runs, then its flat gradient is
    overwritten with the two-launch engine's.  At these shapes the small gradients (LayerNorms, token mixing, biases, heads, in
    fp32 the embeddings) are summed with float atomics, so two engines in the SAME update form already differ in the last bits
    after two steps (measured on every case here); without the copy the test would compare backward runs, not update forms.
    No range of these engines has a slot to add (asserted), so the flat gradient is everything the update reads."""
    import engine_cases as EC
    import engine_ref as ER
    make = EC._av if engine == "avmnist" else EC._mm
    case = make(f"update_{engine}_d{D}_c{C}", EC._tower(D, (8, 8), 4, C=C), EC._tower(D, (16, 16), 8, C=C), EC._fusion(D, C=C), B=5)
    params = G.make_params(ER.case_shapes(case), 31)
    batch = tuple(t.to(dev) for t in ER.case_batch(case, 101))
    if rowtiles is not None:
        monkeypatch.setenv("M2M_AP_ROWTILES", rowtiles)
    engs = []
    for fused in ("0", "1"):
        monkeypatch.setenv("M2M_FUSED_UPDATE", fused)
        e = ER.engine_class(case)(case.cfg, case.B, device=dev, precision=prec, lr=LR, init=False)
        e.load_state_dict(params)
        engs.append(e)
    sep, fus = engs
    assert fus._adam_pack_modules() is not None
    assert all(add is None for e in engs for _, _, add, _ in e._ranges_add)
    for _ in range(2):
        for e in engs:
            e.forward_backward(*batch)
        fus.flat_g.copy_(sep.flat_g)
        for e in engs:
            e.optimizer_step()
    torch.cuda.synchronize()
    assert float(sep.adam_state[0]) == 2.0 and float(fus.adam_state[0]) == 2.0
    ER.assert_update_forms_bit_identical(sep, fus)
