"""GPU tests (-m gpu) of the fusion functions on the fused engines (csrc/fusion.hip, engine._TwoTowerEngine):

  1. the kernels against float64 (sum / mean / max with ties, BiModalGatedUnit forward, input and weight gradients);
  2. an engine step against the oracle's primitives composed with the fusion (tests/fusion_ref.py): logits, losses, every
     gradient, the parameters after three Adam steps -- M2-Mixer-S / -B x four fusions, the gated_4loss shapes (with concat as
     the control), MM-IMDb with sum and gated;
  3. a captured replay against the eager steps, a ragged training sibling, evaluate;
  4. the bound task module (bind_engine + training_step, state_dict, checkpoint resume);
  5. bf16 bit-reproducibility of the gated and max steps.
"""
import pytest
import torch

import fusion_ref as R
import gen_util as G
from conftest import observe

pytestmark = pytest.mark.gpu

FP32_ATOL = 1e-3
LR = 1e-3
NOISE_KEYS = ("token_mix.2.net.3.bias",)       # rounding-level gradient (see tests/test_gpu_engine_backed.py)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from m2_mixer_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def err(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


# ---- 1. kernels -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,name", [(1, "SumFusion"), (2, "MeanFusion"), (3, "MaxFusion")])
@pytest.mark.parametrize("D", [32, 64, 128, 256])
def test_elementwise_fusion_kernels(mode, name, D, dev):
    from m2_mixer_amd import _lib as L
    rows = 37 * 3                                             # not a multiple of any tile
    gen = torch.Generator().manual_seed(D + mode)
    a = torch.randn(rows, D, generator=gen)
    b = torch.randn(rows, D, generator=gen)
    b[::3] = a[::3]                                           # ties
    b[1::7, ::2] = a[1::7, ::2]
    dy = torch.randn(rows, D, generator=gen)
    a64, b64 = a.double().requires_grad_(True), b.double().requires_grad_(True)
    y64 = R.fuse(name, a64, b64)
    y64.backward(dy.double())
    ga, gb, gy = a.to(dev), b.to(dev), dy.to(dev)
    y, da, db = torch.empty_like(ga), torch.empty_like(ga), torch.empty_like(ga)
    s = L.stream_ptr()
    L.check(L.lib().m2m_fusion_forward(mode, ga.data_ptr(), gb.data_ptr(), y.data_ptr(), rows * D, s), "fusion_forward")
    L.check(L.lib().m2m_fusion_backward(mode, ga.data_ptr(), gb.data_ptr(), gy.data_ptr(), da.data_ptr(), db.data_ptr(), rows * D, s),
            "fusion_backward")
    torch.cuda.synchronize()
    assert err(y, y64) <= 1e-6 * max(1.0, float(y64.abs().max()))
    assert err(da, a64.grad) == 0.0 and err(db, b64.grad) == 0.0      # exact: dy, dy / 2, or 0


def test_max_tie_splits_the_gradient(dev):
    from m2_mixer_amd import _lib as L
    a = torch.tensor([1.0, 2.0, 3.0, 0.0], device=dev)
    b = torch.tensor([1.0, 1.0, 4.0, 0.0], device=dev)
    dy = torch.ones(4, device=dev)
    da, db = torch.empty_like(a), torch.empty_like(a)
    L.check(L.lib().m2m_fusion_backward(3, a.data_ptr(), b.data_ptr(), dy.data_ptr(), da.data_ptr(), db.data_ptr(), 4, L.stream_ptr()))
    assert da.cpu().tolist() == [0.5, 1.0, 0.0, 0.5] and db.cpu().tolist() == [0.5, 0.0, 1.0, 0.5]


@pytest.mark.parametrize("D", [32, 64, 128, 256])
@pytest.mark.parametrize("rows", [1, 200, 1031, "large"])
def test_gate_kernels_against_float64(D, rows, dev):
    """rows "large": past the size at which the forward / backward tiles take 16 rows per thread instead of 4 (fusion.hip
    gate_rpt16), and not a multiple of either tile."""
    import ctypes as C
    from m2_mixer_amd import _lib as L
    if rows == "large":
        rows = 512 * 16 * (256 // D) + 27
    gen = torch.Generator().manual_seed(D * 7 + rows)
    mm = dict(mod1_in=D, mod2_in=D, out_size=D)
    p = {k: ((torch.rand(s, generator=gen) * 2 - 1) / (s[-1] if len(s) > 1 else D) ** 0.5) for k, s in R.gate_shapes(mm).items()}
    a, b, dy = (torch.randn(rows, D, generator=gen) for _ in range(3))
    leaves = {k: v.double().requires_grad_(True) for k, v in p.items()}
    a64, b64 = a.double().requires_grad_(True), b.double().requires_grad_(True)
    y64 = R.gate(a64, b64, leaves)
    y64.backward(dy.double())
    # the six parameters and gradients as views of flat buffers one float past a 16-byte boundary (as in the engine, where
    # they follow whatever the towers' shapes add up to)
    n = sum(v.numel() for v in p.values())
    flat_p, flat_g = torch.zeros(n + 1, device=dev), torch.full((n + 1,), 0.25, device=dev)   # the weight gradients are ADDED
    dp, gp, off = {}, {}, 1
    for k, v in p.items():
        dp[k] = flat_p[off:off + v.numel()].view(v.shape)
        dp[k].copy_(v)
        gp[k] = flat_g[off:off + v.numel()].view(v.shape)
        off += v.numel()
    f = lambda *s: torch.zeros(*s, device=dev)
    bufs = dict(t1=f(rows, D), t2=f(rows, D), z=f(rows, D), dh=f(rows, 3 * D), part=f(int(L.lib().m2m_gate_part_floats(rows, D))))
    g = L.Gate()
    g.D = D
    for fld, key in zip(("w1", "b1", "w2", "b2", "wz", "bz"),
                        [f"fusion_function.{k}.{t}" for k in R.GATE_KEYS for t in ("weight", "bias")]):
        setattr(g, fld, dp[key].data_ptr())
        setattr(g, "g_" + fld, gp[key].data_ptr())
    for fld, t in bufs.items():
        setattr(g, fld, t.data_ptr())
    ga, gb, gy = a.to(dev), b.to(dev), dy.to(dev)
    y, da, db = f(rows, D), f(rows, D), f(rows, D)
    s = L.stream_ptr()
    L.check(L.lib().m2m_gate_forward(C.byref(g), ga.data_ptr(), gb.data_ptr(), y.data_ptr(), rows, 1, s), "gate_forward")
    L.check(L.lib().m2m_gate_backward(C.byref(g), gy.data_ptr(), da.data_ptr(), db.data_ptr(), rows, s), "gate_backward")
    L.check(L.lib().m2m_gate_wgrad(C.byref(g), ga.data_ptr(), gb.data_ptr(), rows, s), "gate_wgrad")
    torch.cuda.synchronize()
    assert err(y, y64) < 2e-6
    assert err(da, a64.grad) < 1e-5 and err(db, b64.grad) < 1e-5
    for k, leaf in leaves.items():
        scale = max(1.0, float(leaf.grad.abs().max()))
        assert err(gp[k] - 0.25, leaf.grad) < 2e-6 * scale * max(1.0, rows ** 0.5), k


# ---- 2. engine step against the composed oracle ----------------------------------------------------------------------------
def _engine(task, c, B, dev, prec, params):
    from m2_mixer_amd.engine import AVMnistEngine, MMIMDBEngine
    cls = AVMnistEngine if task == "avmnist" else MMIMDBEngine
    eng = cls(dict(c, dropout=0.0), B, device=dev, precision=prec, lr=LR, init=False)
    eng.load_state_dict(params)
    return eng


def _batch(task, c, B, seed):
    if task == "avmnist":
        return G.avmnist_batch(B, seed, c)
    image, text, label = G.mmimdb_batch(B, seed, c)
    return image, text, label


CASES = ([("avmnist", "S", f) for f in R.FUSIONS] + [("avmnist", "B", f) for f in R.FUSIONS]
         + [("avmnist", "gated_4loss", "BiModalGatedUnit"), ("avmnist", "gated_4loss", "ConcatFusion"),
            ("mmimdb", "mmimdb", "SumFusion"), ("mmimdb", "mmimdb", "BiModalGatedUnit")])


def _cfg(task, shapes, fusion):
    base = {"S": G.AVMNIST["S"], "B": G.AVMNIST["B"], "gated_4loss": R.GATED_4LOSS, "mmimdb": G.MMIMDB}[shapes]
    return R.with_fusion(base, fusion)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("task,shapes,fusion", CASES, ids=[f"{s}-{f}" for _, s, f in CASES])
def test_engine_step_against_oracle(task, shapes, fusion, prec, dev):
    c = _cfg(task, shapes, fusion)
    B = 6
    params = dict(G.make_params(R.two_tower_shapes(task, c), 21))
    pw = torch.tensor(c["pos_weight"], dtype=torch.float64) if task == "mmimdb" else None
    ref = R.Step(task, c, params, LR, pw)
    eng = _engine(task, c, B, dev, prec, params)
    assert list(eng.shapes) == list(params)
    lt, lo, gr, pa = (2e-2, 2e-2, 5e-2, 1e-2) if prec == "bf16" else (FP32_ATOL, FP32_ATOL, FP32_ATOL, 2e-3)
    for step in range(3):
        xa, xb, y = _batch(task, c, B, 100 + step)
        out = ref.step(xa, xb, y)
        eng.forward_backward(xa.to(dev), xb.to(dev), y.to(dev))
        torch.cuda.synchronize()
        if step == 0:
            e_lg = err(eng.logits, out["logits"])
            e_ls = err(eng.losses, out["losses"])
            e_g = max(err(eng.grads[k], g) / max(1.0, float(g.abs().max())) for k, g in out["grads"].items())
            if prec == "fp32":
                assert e_lg < lt and e_ls < lo and e_g < gr, (e_lg, e_ls, e_g)
                if task == "avmnist":
                    assert torch.equal(eng.preds[2].cpu().long(), out["preds"])
            else:
                kind = f"fusion {fusion} {shapes} bf16"
                assert observe(kind + " logits", e_lg, lt) < lt
                assert observe(kind + " grads (rel)", e_g, gr) < gr
        eng.optimizer_step()
    torch.cuda.synchronize()
    e_p = max(err(eng.params[k], v) for k, v in ref.p.items() if not k.endswith(NOISE_KEYS))
    if prec == "fp32":
        assert e_p < pa, e_p
    else:
        assert observe(f"fusion {fusion} {shapes} bf16 params after 3 steps", e_p, pa) < pa


# ---- 3. replay, siblings, evaluation -----------------------------------------------------------------------------------
@pytest.mark.parametrize("fusion", R.FUSIONS)
def test_replay_sibling_and_evaluate(fusion, dev):
    c = _cfg("avmnist", "B", fusion)
    B = 8
    params = dict(G.make_params(R.two_tower_shapes("avmnist", c), 5))
    batches = [[t.to(dev) for t in G.avmnist_batch(B, 40 + i, c)] for i in range(3)]
    eager = _engine("avmnist", c, B, dev, "fp32", params)
    for bt in batches:
        eager.fused_step(*bt)
    graphed = _engine("avmnist", c, B, dev, "fp32", params)
    rag = graphed.sibling(3)                                  # (training siblings are built before capture)
    replay = graphed.capture(*batches[0])
    for bt in batches:
        replay(*bt)
    torch.cuda.synchronize()
    assert torch.equal(eager.flat_p, graphed.flat_p) and torch.equal(eager.flat_m, graphed.flat_m)
    # (the heads kernel adds the per-workgroup loss terms with float atomics: the reported losses agree up to rounding)
    assert err(eager.losses, graphed.losses) < 1e-5
    # ragged training sibling + evaluate against the oracle
    # the oracle continues from the engine's parameters AND Adam state (step count, moments)
    ref = R.Step("avmnist", c, {k: v.cpu() for k, v in graphed.params.items()}, LR)
    ref.t = int(graphed.adam_state[0])
    ref.m = {k: v.cpu().double() for k, v in graphed.exp_avg.items()}
    ref.v = {k: v.cpu().double() for k, v in graphed.exp_avg_sq.items()}
    xa, xb, y = G.avmnist_batch(3, 77, c)
    out = ref.step(xa, xb, y)
    rag.pack()
    rag.forward_backward(xa.to(dev), xb.to(dev), y.to(dev))
    rag.optimizer_step()
    graphed.pack()
    torch.cuda.synchronize()
    assert err(rag.logits, out["logits"]) < FP32_ATOL
    assert max(err(graphed.params[k], v) for k, v in ref.p.items() if not k.endswith(NOISE_KEYS)) < 2e-3
    ev = graphed.sibling(5, trains=False)
    xa, xb, y = G.avmnist_batch(5, 78, c)
    o = ev.evaluate(xa.to(dev), xb.to(dev), y.to(dev))
    want = ref.forward(xa, xb, y)
    assert err(o["logits"], want["logits"][2]) < FP32_ATOL and err(o["loss"], want["loss"]) < FP32_ATOL
    assert torch.equal(o["preds"].cpu().long(), want["preds"])


# ---- 4. bound task module ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fusion", ["MaxFusion", "BiModalGatedUnit"])
def test_bound_module_trains_and_resumes(fusion, dev, tmp_path):
    import m2_mixer_amd as M
    from m2_mixer_amd import models as MD
    c = _cfg("avmnist", "S", fusion)
    mods = {n: dict(c[n], block_type="MLPMixer") for n in ("image", "audio")}
    mods["multimodal"] = dict(c["multimodal"], block_type="FusionMixer")
    mods["classification"] = dict(classifier="StandardClassifier", num_classes=c["num_classes"], input_shape=[16, 4, 32])
    prev = M.config.get_precision()
    M.set_precision("fp32")
    try:
        net = MD.AVMnistMixerMultiLoss({"dropout": 0.0, "modalities": mods}, {"lr": LR, "betas": (0.9, 0.999), "scheduler_patience": 1}).to(dev)
        params = dict(G.make_params(R.two_tower_shapes("avmnist", c), 9))
        assert list(net.state_dict()) == list(params)
        net.load_state_dict(params)
        ref = R.Step("avmnist", c, params, LR)
        B = 8
        net.bind_engine(B, precision="fp32")
        net.configure_optimizers()
        for i in range(3):
            image, audio, label = G.avmnist_batch(B, 60 + i, c)
            out = ref.step(image, audio, label)
            r = net.training_step({"image": image.to(dev), "audio": audio.to(dev), "label": label.to(dev)}, i)
            torch.cuda.synchronize()
            assert abs(float(r["loss"]) - float(out["loss"])) < FP32_ATOL
        eng = net.engine
        sd = net.state_dict()
        assert all(torch.equal(sd[k], eng.params[k]) for k in eng.params)
        assert max(err(eng.params[k], v) for k, v in ref.p.items() if not k.endswith(NOISE_KEYS)) < 2e-3
        # checkpoint resume: a fresh engine from the saved weights + optimizer state continues bit-identically
        path = tmp_path / "ck.pt"
        torch.save({"state_dict": {k: v.cpu() for k, v in sd.items()}, "opt": eng.optimizer_state_dict()}, path)
        image, audio, label = [t.to(dev) for t in G.avmnist_batch(B, 90, c)]
        ck = torch.load(path)
        other = _engine("avmnist", c, B, dev, "fp32", ck["state_dict"])
        other.load_optimizer_state_dict(ck["opt"])
        eng.fused_step(image, audio, label)
        other.fused_step(image, audio, label)
        torch.cuda.synchronize()
        assert torch.equal(eng.flat_p, other.flat_p)
    finally:
        M.set_precision(prev)


# ---- 5. bf16 reproducibility -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fusion", ["MaxFusion", "BiModalGatedUnit"])
def test_bf16_captured_steps_are_bit_reproducible(fusion, dev):
    from m2_mixer_amd.engine import AVMnistEngine
    c = _cfg("avmnist", "B", fusion)
    B = 64
    batches = [[t.to(dev) for t in G.avmnist_batch(B, 10 + i, c)] for i in range(3)]
    runs = []
    for _ in range(2):
        eng = AVMnistEngine(c, B, device=dev, precision="bf16", lr=LR, seed=3)
        replay = eng.capture(*batches[0])
        for bt in batches:
            replay(*bt)
        eng.forward_backward(*batches[0])
        torch.cuda.synchronize()
        runs.append((eng.flat_p.clone(), eng.flat_g.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
