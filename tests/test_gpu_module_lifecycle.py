"""GPU tests (-m gpu) of the state that sits between launches on the module path (tests/lifecycle_cases.py): after eager
optimizer steps of either form, hipGraph replays, `.data` edits and load_state_dict, every forward -- evaluation, a train-mode
pass under no_grad, an evaluation-mode forward that is differentiated -- must compute with the weights as they are then.

Three checks at every observation event:
  * the packed operand copies of every tower and embedding runtime are those a fresh pack of the current weights gives, bit for
    bit (packing is a deterministic copy-and-round) -- fp32 and bf16;
  * fp32: the logits of every head against the float64 oracle at the module's current state_dict(), to FP32_ATOL = 1e-3; for
    `eval_grad` the gradients that carry the towers' input gradients as well (see _Model.grad_keys);
  * fp32: the oracle check can fail -- with the packed tensors (lifecycle_cases.PACKED_SUFFIXES) taken from the weights of before
    the last update and everything else current, the oracle's logits move by at least 10 x FP32_ATOL in every head that a tower
    feeds (MIMIC's `logits_static` comes from the MLP alone, which keeps no packed copy).  A condition on the inputs (learning
    rate, seeds), not on the kernels; the bf16 runs rely on the bit-equality check only (MIMIC's stale distance is 2.4 x the
    bf16 logits bar).

Two further tests: the number of pack launches (a training step issues one per runtime and forward, as before; consecutive
evaluations at most one per runtime), and the dropout stream around the construction of a GraphedStep.
"""
import pytest
import torch

from conftest import observe
from lifecycle_cases import CASES, GRAPH_UPDATES, OBSERVATIONS, UPDATES
from lifecycle_ref import HEADS, Ref
from test_gpu_parity import _model_cfg

pytestmark = pytest.mark.gpu

FP32_ATOL = 1e-3       # the suite's fp32 logits bar (BASELINE.json north_star)
GRAD_REL = 1e-3        # parameter gradients relative to the tensor's max, input gradients FP32_ATOL absolute:
                       # the bars of test_gpu_bench_path.py::test_module_path_is_reentrant
STALE_FACTOR = 10      # the stale distance must be at least this many times the logits bar


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from m2_mixer_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def abserr(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max()) / (float(b.abs().max()) + 1e-12)


# ---------------------------------------------------------------------------------------------------------------
# the model under test: one of the three task modules, or a bare 11-block FusionMixer
# ---------------------------------------------------------------------------------------------------------------
class _Model:
    def __init__(self, name, dev, lr, p=0.0):
        from m2_mixer_amd import models as MD
        from m2_mixer_amd import modules as MM
        self.name, self.dev, self.ref = name, dev, Ref(name)
        if name == "deep":
            self.net = MM.get_block_by_name(block_type="FusionMixer", num_patches=self.ref.info["N"], dropout=p, **self.ref.c).to(dev)
        else:
            model_cfg, c = _model_cfg(name)
            assert c is self.ref.c
            model_cfg["dropout"] = p
            cls = {"avmnist": MD.AVMnistMixerMultiLoss, "mimic": MD.MimicMixerMultiLoss, "mmimdb": MD.MMIMDBMixerMultiLoss}[name]
            self.net = cls(model_cfg, {"lr": lr, "betas": (0.9, 0.999), "scheduler_patience": 2}).to(dev)
        assert [k for k, _ in self.net.named_parameters()] == list(self.ref.shapes.keys())
        self.load()

    def load(self, seed=None):
        self.net.load_state_dict(self.ref.params(seed), strict=False)     # (MM-IMDb: the pos_weight buffers stay)

    def batch(self, seed):
        return self.ref.batch(seed)

    def to_dev(self, batch, grad=False):
        """The batch on the device; grad: the inputs (not the labels) require gradients."""
        f = lambda t, is_input: t.to(self.dev).requires_grad_(True) if grad and is_input else t.to(self.dev)
        if isinstance(batch, dict):
            return {k: f(v, k != "label") for k, v in batch.items()}
        return tuple(f(v, self.name == "deep" or i < len(batch) - 1) for i, v in enumerate(batch))

    def forward(self, dbatch, mode):
        """head name -> tensor, and the training loss"""
        if self.name == "deep":
            y = self.net(dbatch[0])
            return {"tokens": y}, y.square().sum()
        out = self.net.shared_step(dbatch, mode=mode)
        return {k: out[k] for k in HEADS[self.name]}, out["loss"]

    def state64(self):
        return {k: v.detach().double().cpu() for k, v in self.net.state_dict().items()}

    def hip_modules(self):
        return [m for m in self.net.modules() if hasattr(m, "invalidate_packs")]

    def runtimes(self):
        """Every tower and embedding runtime the module path has built so far."""
        rts = []
        for m in self.hip_modules():
            rts += list(m._rts or ())
            if getattr(m, "_ert", None) is not None:
                rts.append(m._ert)
        return rts

    def grad_keys(self):
        """The parameters whose gradients ARE the towers' input gradients, contracted with the inputs: the task modules'
        autograd functions return no gradient for the raw images / series (nothing upstream could use one), so the input
        gradient of a tower shows in its embedding's weight and bias gradients, and that of MIMIC's fusion tower in the static
        MLP's gradients as well.  (The bare tower of `deep` takes tokens and returns their gradient itself.)"""
        return [k for k in self.ref.shapes if ".to_patch_embedding.0." in k or ".proj." in k or k.startswith("static_extractor.")]


def _scalar(heads):
    """What `eval_grad` differentiates: every head's logits, squared and summed (O(1) gradients in every tower)."""
    return sum(v.square().sum() for v in heads.values())


def _packs_stale(model):
    """Names of the packed buffers that differ from a fresh pack of the current weights (the idiom of
    test_module_path_step_replayed_as_one_graph part (c)).  Leaves the runtimes' packed-for marks as it found them."""
    stale = []
    rts = model.runtimes()
    assert rts
    for ri, rt in enumerate(rts):
        bufs = {}
        if hasattr(rt, "nblocks"):
            for i in range(rt.nblocks):
                bufs.update({f"packed{i}.{k}": v for k, v in rt._keep[f"packed{i}"].items()})
        else:
            bufs["wn"] = rt._keep["wn"]
        have = {k: v.clone() for k, v in bufs.items()}
        mark = rt._packed_for
        rt.pack(force=True)
        rt._packed_for = mark
        torch.cuda.synchronize()
        differ = [k for k, v in bufs.items() if not torch.equal(v, have[k])]
        if differ:
            stale.append(f"{type(rt).__name__}[{ri}]: {', '.join(differ)}")
    return stale


# ---------------------------------------------------------------------------------------------------------------
# the events
# ---------------------------------------------------------------------------------------------------------------
class _Driver:
    def __init__(self, case, dev):
        self.case, self.m = case, _Model(case.model, dev, case.lr, case.p)
        self.opts, self.graphs = {}, {}
        self.prev = None              # the state_dict of before the last update event
        self.n = 0                    # events so far: every event draws its batch / its edit from a seed of its own

    def _optimizer(self, fused):
        net = self.m.net
        if self.m.name == "deep":
            return torch.optim.Adam(net.parameters(), lr=self.case.lr, fused=fused, foreach=not fused)
        opt = net.configure_optimizers()["optimizer"]
        for g in opt.param_groups:
            g["fused"], g["foreach"] = fused, not fused
        return opt

    def update(self, kind):
        from m2_mixer_amd.graphs import GraphedStep
        m, net = self.m, self.m.net
        self.n += 1
        self.prev = m.state64()
        net.train()
        if kind in ("adam_foreach", "adam_fused"):
            opt = self.opts.get(kind) or self.opts.setdefault(kind, self._optimizer(kind == "adam_fused"))
            opt.zero_grad(set_to_none=True)
            m.forward(m.to_dev(m.batch(1000 + self.n)), "train")[1].backward()
            opt.step()
        elif kind in GRAPH_UPDATES:
            b = m.to_dev(m.batch(1000 + self.n))
            if kind not in self.graphs:
                self.graphs[kind] = GraphedStep(net, self._optimizer(False), b, fused=kind == "graph_fused")
            self.graphs[kind](b)
        elif kind == "data_edit":
            gen = torch.Generator().manual_seed(2000 + self.n)
            for p in net.parameters():
                sign = torch.randint(0, 2, p.shape, generator=gen).float() * 2 - 1
                p.data.add_(sign.to(m.dev) * self.case.lr)          # behind the version counters: ...
            for mod in m.hip_modules():
                mod.invalidate_packs()                              # ... the documented call says so
        elif kind == "load_state_dict":
            m.load(m.ref.info["seed"] + 100 + self.n)
        else:
            raise AssertionError(kind)
        torch.cuda.synchronize()

    def observation(self, kind, prec):
        """-> (problems, smallest stale distance over the tower-fed heads or None, worst logits error or None)"""
        m, net = self.m, self.m.net
        self.n += 1
        batch = m.batch(3000 + self.n)
        xg = None
        if kind == "eval_grad":
            net.eval()
            net.zero_grad(set_to_none=True)
            db = m.to_dev(batch, grad=True)
            heads, _ = m.forward(db, "val")
            _scalar(heads).backward()
            xg = db[0].grad if m.name == "deep" else None
        else:
            net.eval() if kind == "eval" else net.train()
            with torch.no_grad():
                heads, _ = m.forward(m.to_dev(batch), "val")
        torch.cuda.synchronize()
        problems = [f"{kind}: not the pack of the current weights -- {s}" for s in _packs_stale(m)]
        if prec != "fp32":
            return problems, None, None
        cur = m.state64()
        leaves = {k: v.clone().requires_grad_(kind == "eval_grad" and v.is_floating_point()) for k, v in cur.items()}
        xr = None
        if kind == "eval_grad" and m.name == "deep":
            xr = batch[0].double().requires_grad_(True)
        ref = m.ref.forward((xr,) if xr is not None else batch, leaves)
        worst = 0.0
        for k in HEADS[m.name]:
            e = observe(f"module lifecycle, {m.name}: logits vs the oracle at the current weights (abs)", abserr(heads[k], ref[k]), FP32_ATOL)
            worst = max(worst, e)
            if not e < FP32_ATOL:
                problems.append(f"{kind}: {k} differs from the oracle at the current weights by {e:.3e}")
        dist = m.ref.stale_distance(batch, cur, self.prev, true={k: v.detach() for k, v in ref.items()})
        if not dist >= STALE_FACTOR * FP32_ATOL:
            problems.append(f"{kind}: stale packed tensors would move the logits by {dist:.3e} only: raise the case's lr")
        if kind == "eval_grad":
            _scalar({k: ref[k] for k in HEADS[m.name]}).backward()
            if xr is not None:
                e = observe(f"module lifecycle, {m.name}: input gradient in evaluation mode (abs)", abserr(xg, xr.grad), FP32_ATOL)
                if not e < FP32_ATOL:
                    problems.append(f"eval_grad: input gradient differs from the oracle's by {e:.3e}")
            named = dict(net.named_parameters())
            for k in m.grad_keys():
                e = observe(f"module lifecycle, {m.name}: embedding gradients in evaluation mode (rel)", relerr(named[k].grad, leaves[k].grad), GRAD_REL)
                if not e < GRAD_REL:
                    problems.append(f"eval_grad: gradient of {k} differs from the oracle's by {e:.3e} of its max")
        return problems, dist, worst


@pytest.mark.parametrize("case,prec", [(c, p) for c in CASES for p in c.precs], ids=[f"{c.name}-{p}" for c in CASES for p in c.precs])
def test_observations_see_the_current_weights(case, prec, dev):
    """Every observation event of every case of tests/lifecycle_cases.py: packed copies current bit for bit; in fp32 the logits
    (and, for eval_grad, the gradients that carry the input gradients) of the float64 oracle at the current state_dict; and the
    stale distance that keeps that comparison from passing vacuously."""
    import m2_mixer_amd as M
    from m2_mixer_amd import config
    was = M.get_precision()
    M.set_precision(prec)
    try:
        drv = _Driver(case, dev)
        problems, dists, worst = [], [], []
        for i, ev in enumerate(case.events):
            if ev in UPDATES:
                drv.update(ev)
                continue
            assert ev in OBSERVATIONS, ev
            pr, dist, w = drv.observation(ev, prec)
            problems += [f"event {i}, {p}" for p in pr]
            dists += [dist] if dist is not None else []
            worst += [w] if w is not None else []
        if dists:
            # (a lower bound, not an error: the summary line reads "smallest distance | what it has to reach")
            observe(f"lifecycle stale distance, {case.name} (lr {case.lr:g})", min(dists), STALE_FACTOR * FP32_ATOL)
            print(f"{case.name}: stale distance {min(dists):.3e}, worst logits error {max(worst):.3e}, lr {case.lr:g}")
        assert not problems, "\n".join(problems)
    finally:
        config.set_device_dropout_step(False)
        M.set_precision(was)


# ---------------------------------------------------------------------------------------------------------------
# pack launches
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["avmnist", "mimic", "deep"])
def test_pack_launches_per_step_and_per_evaluation(name, dev, monkeypatch):
    """pack() calls mark_packed exactly when it launches.  A training-mode step issues one pack launch per runtime and forward
    (what it always did: keeping evaluation current must not add a launch to the training step); k consecutive evaluation
    forwards, or train-mode forwards under no_grad, with no update between them issue at most one per runtime."""
    import m2_mixer_amd as M
    from m2_mixer_amd.runtime import EmbedRuntime, TowerRuntime
    was = M.get_precision()
    M.set_precision("fp32")
    counts = {}
    for cls in (TowerRuntime, EmbedRuntime):
        orig = cls.mark_packed

        def counted(self, _orig=orig):
            counts[id(self)] = counts.get(id(self), 0) + 1
            return _orig(self)
        monkeypatch.setattr(cls, "mark_packed", counted)
    try:
        m = _Model(name, dev, 1e-2)
        nrt = {"avmnist": 5, "mimic": 3, "deep": 2}[name]            # towers' descriptors + embeddings
        for fused in (False, True):
            opt = torch.optim.Adam(m.net.parameters(), lr=1e-2, fused=fused, foreach=not fused)

            def step(seed):
                m.net.train()
                opt.zero_grad(set_to_none=True)
                m.forward(m.to_dev(m.batch(seed)), "train")[1].backward()
                opt.step()
            step(1)                                                  # (builds the runtimes on the first pass)
            ids = [id(rt) for rt in m.runtimes()]
            assert len(ids) == nrt
            counts.clear()
            step(2)
            assert [counts.get(i, 0) for i in ids] == [1] * nrt, "pack launches of one training step"
            step(3)
            step(4)
            assert [counts.get(i, 0) for i in ids] == [3] * nrt, "pack launches of three training steps"
            for train in (False, True):
                counts.clear()
                m.net.train(train)
                with torch.no_grad():
                    for k in range(3):
                        m.forward(m.to_dev(m.batch(10 + k)), "val")
                assert all(counts.get(i, 0) <= 1 for i in ids), ("pack launches of three forwards without an update", train)
            counts.clear()
            step(5)
            assert [counts.get(i, 0) for i in ids] == [1] * nrt, "pack launches of a training step after evaluations"
        torch.cuda.synchronize()
    finally:
        M.set_precision(was)


# ---------------------------------------------------------------------------------------------------------------
# the dropout stream around GraphedStep's construction
# ---------------------------------------------------------------------------------------------------------------
def test_graphed_step_construction_leaves_the_dropout_stream_alone(dev):
    """GraphedStep's constructor takes warm-up steps and a captured one, which advance every module's dropout step counter
    (host mirror `_drop_step`, device counter `_drop_counter`).  They are undone like the parameters and the optimizer state:
    (a) after construction both equal what they were (a counter that did not exist yet reads 0, the step of a fresh module),
    and n replays advance the device counter by n; (b) "constructing a GraphedStep does not train" with dropout ON: three
    replays leave the parameters of three eager steps from the same state -- the same net, since two nets never share masks
    (`_site_base` comes from a global counter) -- to 1e-3, a tenth of one step's lr (the bar and the reasoning of the
    dropout-off comparison in test_module_path_step_replayed_as_one_graph).  With the constructor's draws left in the stream,
    the graphed run would start at mask step warmup + 2 and every update would differ by up to 2 lr."""
    import m2_mixer_amd as M
    from m2_mixer_amd import config
    from m2_mixer_amd.graphs import GraphedStep
    was = M.get_precision()
    M.set_precision("fp32")
    try:
        m = _Model("avmnist", dev, 1e-2, p=0.5)
        net = m.net
        net.train()
        batches = [m.to_dev(m.batch(40 + i)) for i in range(3)]
        # every module that draws masks (the towers' MixerBlocks carry the attribute too, but never run on their own)
        mods = [mod for mod in net.modules() if hasattr(mod, "_drop_step")]

        def counters():
            c = [getattr(mod, "_drop_counter", None) for mod in mods]
            return [mod._drop_step for mod in mods], [0 if t is None else int(t.item()) for t in c]
        # (a)
        steps0, ctr0 = counters()
        gs = GraphedStep(net, net.configure_optimizers()["optimizer"], batches[0], warmup=2)
        drawing = [getattr(mod, "_drop_counter", None) is not None for mod in mods]
        assert sum(drawing) == 3, "the three towers draw masks from device counters"
        assert counters() == (steps0, ctr0), "warm-up and capture left their draws in the dropout stream"
        for b in batches:
            gs(b)
        torch.cuda.synchronize()
        assert counters()[1] == [c + 3 if d else c for c, d in zip(ctr0, drawing)]
        # (b)
        opt = net.configure_optimizers()["optimizer"]
        for g in opt.param_groups:
            g["capturable"] = True                     # (the same optimizer implementation in both runs)
        params = list(net.parameters())

        def eager(b):
            opt.zero_grad(set_to_none=True)
            net.shared_step(b, mode="train")["loss"].backward()
            opt.step()
        eager(batches[0])                              # creates the optimizer state, so that it can be put back in place
        torch.cuda.synchronize()
        snap_p = [p.detach().clone() for p in params]
        snap_s = [{k: v.detach().clone() for k, v in opt.state[p].items() if torch.is_tensor(v)} for p in params]
        snap_steps, snap_ctr = counters()

        def restore():
            with torch.no_grad():
                for p, sp, ss in zip(params, snap_p, snap_s):
                    p.copy_(sp)
                    for k, v in ss.items():
                        opt.state[p][k].copy_(v)
            for mod, s, c in zip(mods, snap_steps, snap_ctr):
                mod._drop_step = s
                if getattr(mod, "_drop_counter", None) is not None:
                    mod._drop_counter.fill_(c)
        config.set_device_dropout_step(True)
        for b in batches:
            eager(b)
        torch.cuda.synchronize()
        want = [p.detach().clone() for p in params]
        restore()
        gs2 = GraphedStep(net, opt, batches[0], warmup=2, fused=False)
        assert all(torch.equal(p, sp) for p, sp in zip(params, snap_p)) and counters() == (snap_steps, snap_ctr)
        for b in batches:
            gs2(b)
        torch.cuda.synchronize()
        worst = max(float((p.detach() - w).abs().max()) for p, w in zip(params, want))
        observe("graphed vs eager module-path step with dropout 0.5, max parameter difference after 3 steps (abs)", worst, 1e-3)
        assert worst < 1e-3
    finally:
        config.set_device_dropout_step(False)
        M.set_precision(was)
