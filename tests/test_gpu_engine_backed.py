"""GPU tests (-m gpu) of the engine-backed task modules and of the device-resident loss weights (ABI 18):

  * m2m_heads_ce_w / m2m_heads_bce_w against m2m_heads_ce / m2m_heads_bce (bit-identical with the same weights);
  * a captured engine step follows set_fusion_loss_weight without being captured again;
  * bind_engine + training_step / validation_step against the CPU oracle (fp32), the ragged last batch, ReduceLROnPlateau
    through EngineOptimizer, the loss-weight schedule, checkpoint resume, MM-IMDb / MIMIC-H in bf16.
"""
import pytest
import torch

import gen_util as G
from conftest import observe
from oracle import m2mixer_oracle as O

pytestmark = pytest.mark.gpu

FP32_ATOL = 1e-3       # BASELINE.json north_star: fp32 within 1e-3
BF16_LOGITS = 2e-2     # as tests/test_gpu_bench_path.py
LR = 1e-3
# the token-mixing output bias adds a per-token constant across the channels that the next LayerNorm removes: its gradient
# is zero up to rounding, and Adam's normalised update of a rounding-level gradient is noise (smoke() skips it the same way)
NOISE_KEYS = ("token_mix.2.net.3.bias",)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from m2_mixer_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture
def fp32_modules():
    import m2_mixer_amd as M
    prev = M.config.get_precision()
    M.set_precision("fp32")
    yield
    M.set_precision(prev)


def abserr(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def _model_cfg(task, c, **extra):
    if task == "mimic":
        mods = {"static": dict(c["static"], block_type="MLP"), "time": dict(c["time"], block_type="MLPMixerNoPatching")}
    else:
        a, b = ("image", "audio") if task == "avmnist" else ("image", "text")
        mods = {a: dict(c[a], block_type="MLPMixer"), b: dict(c[b], block_type="MLPMixer")}
    mods["multimodal"] = dict(c["multimodal"], block_type="FusionMixer", fusion_function="ConcatFusion")
    mods["classification"] = dict(classifier="StandardClassifier", num_classes=c["num_classes"],
                                  input_shape=[16, 49, c["multimodal"]["hidden_dim"]])
    cfg = {"dropout": c["dropout"], "modalities": mods, **extra}
    if task == "mmimdb":
        cfg["pos_weight"] = c["pos_weight"]
    return cfg


def make_net(task, c, seed, dev, **extra):
    from m2_mixer_amd import models as MD
    cls = {"avmnist": MD.AVMnistMixerMultiLoss, "mimic": MD.MimicMixerMultiLoss, "mmimdb": MD.MMIMDBMixerMultiLoss}[task]
    shapes = {"avmnist": G.avmnist_shapes, "mimic": G.mimic_shapes, "mmimdb": G.mmimdb_shapes}[task](c)
    params = dict(G.make_params(shapes, seed))
    net = cls(_model_cfg(task, c, **extra), {"lr": LR, "betas": (0.9, 0.999), "scheduler_patience": 1}).to(dev)
    net.load_state_dict(params, strict=False)          # (MM-IMDb: the criteria's pos_weight buffers keep the cfg values)
    return net, params


class Oracle:
    """The reference's training step on the CPU: autograd through the oracle's forward at a given fusion_loss_weight, then
    torch.optim.Adam's update (oracle.adam_step) of every parameter."""

    def __init__(self, task, c, params):
        self.task, self.c, self.p, self.state = task, c, {k: v.clone() for k, v in params.items()}, {"step": 0, "m": {}, "v": {}}

    def forward(self, batch, p, w=1.0 / 3):
        c = self.c
        if self.task == "avmnist":
            return O.avmnist_forward(batch["image"], batch["audio"], batch["label"], p, c, fusion_loss_weight=w)
        if self.task == "mimic":
            return O.mimic_forward(*batch, p, c, fusion_loss_weight=w)
        return O.mmimdb_forward(batch["image"], batch["text"], batch["label"], p, c, torch.tensor(c["pos_weight"]))

    def step(self, batch, lr=LR, w=1.0 / 3):
        leaves = {k: v.clone().requires_grad_(True) for k, v in self.p.items()}
        out = self.forward(batch, leaves, w)
        out["loss"].backward()
        self.state["step"] += 1
        for k, leaf in leaves.items():
            g = leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)
            m = self.state["m"].get(k, torch.zeros_like(g))
            v = self.state["v"].get(k, torch.zeros_like(g))
            self.p[k], self.state["m"][k], self.state["v"][k] = O.adam_step(self.p[k], g, m, v, self.state["step"], lr)
        return {k: v.detach() for k, v in out.items() if torch.is_tensor(v)}

    def clone(self):
        o = Oracle(self.task, self.c, self.p)
        o.state = {"step": self.state["step"], "m": dict(self.state["m"]), "v": dict(self.state["v"])}
        return o


def cpu(batch):
    return {k: v.cpu() for k, v in batch.items()} if isinstance(batch, dict) else tuple(t.cpu() for t in batch)


def avmnist_batch(B, seed, c, dev):
    image, audio, labels = G.avmnist_batch(B, seed, c)
    return {"image": image.to(dev), "audio": audio.to(dev), "label": labels.to(dev)}


def param_err(net, oracle):
    return max(abserr(p, oracle.p[k]) for k, p in net.named_parameters() if not k.endswith(NOISE_KEYS))


# ---------------------------------------------------------------------------------------------------------------
# C ABI 18: the heads' loss coefficients from device memory
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bce", [False, True])
def test_heads_with_device_weights_equal_the_by_value_weights(bce, dev):
    """Same inputs, the device table holding the by-value coefficients: logits, losses, g_w, g_b, d_pooled bit-identical.
    (B = 4: one workgroup per head, so the float atomics add onto zero and the per-head outputs are order-free; the weighted
    total sums three heads' atomics in launch order, compared to 1e-6.)  A doubled table doubles every gradient exactly."""
    from m2_mixer_amd.runtime import heads_bce, heads_ce
    B, D, K, nh = 4, 64, (23 if bce else 10), 3
    gen = torch.Generator().manual_seed(7)
    r = lambda *s: (torch.rand(*s, generator=gen) * 2 - 1).to(dev)
    pooled = [r(B, D) for _ in range(nh)]
    ws, bs = [r(K, D) for _ in range(nh)], [r(K) for _ in range(nh)]
    coef = [0.9, 0.6, 1.5]
    if bce:
        labels = (torch.rand(B, K, generator=gen) > 0.7).float().to(dev)
        pos_weight = (torch.rand(K, generator=gen) * 10 + 1).to(dev)
    else:
        labels = torch.randint(0, K, (B,), generator=gen).to(dev)

    def run(weights):
        gw = [torch.zeros(K, D, device=dev) for _ in range(nh)]
        gb = [torch.zeros(K, device=dev) for _ in range(nh)]
        dp = [torch.zeros(B, D, device=dev) for _ in range(nh)]
        heads = [dict(pooled=pooled[i], w=ws[i], b=bs[i], g_w=gw[i], g_b=gb[i], d_pooled=dp[i], weight=coef[i]) for i in range(nh)]
        if bce:
            lg, ls, pr = heads_bce(heads, labels, pos_weight, B, D, K, weights=weights)
        else:
            lg, ls, pr = heads_ce(heads, labels, B, D, K, weights=weights)
        torch.cuda.synchronize()
        return lg, ls, pr, torch.stack(gw), torch.stack(gb), torch.stack(dp)

    base = run(None)
    table = torch.tensor(coef, dtype=torch.float32, device=dev)
    same = run(table)
    for name, x, y in zip(("logits", "losses", "preds", "g_w", "g_b", "d_pooled"), base, same):
        if name == "losses":
            assert torch.equal(x[:nh], y[:nh]) and abs(float(x[nh] - y[nh])) <= 1e-6 * abs(float(x[nh])), name
        else:
            assert torch.equal(x, y), name
    doubled = run(table * 2)
    for i in (3, 4, 5):
        assert torch.equal(doubled[i], 2 * base[i])
    assert torch.equal(doubled[1][:nh], base[1][:nh])                    # the per-head losses are unweighted
    assert abs(float(doubled[1][nh] - 2 * base[1][nh])) <= 1e-6 * abs(float(base[1][nh]))


def test_captured_step_follows_set_fusion_loss_weight(dev):
    """AV-MNIST S, fp32: capture, replay one step at the default 1/3, set_fusion_loss_weight(0.6), replay again -- the graph
    is not captured again.  The second step's total loss, Adam's first moments (linear in the gradient: the heads' are scaled
    by their coefficients) and the parameters after it follow the oracle at 0.6 (1e-3); the moments do not follow the oracle
    that kept 1/3."""
    from m2_mixer_amd.engine import AVMnistEngine, MMIMDBEngine
    cfg, B = dict(G.AVMNIST["S"], dropout=0.0), 24
    eng = AVMnistEngine(cfg, B, device=dev, precision="fp32", lr=LR, init=False)
    params = dict(G.make_params(G.avmnist_shapes(cfg), 11))
    eng.load_state_dict(params)
    b1, b2 = avmnist_batch(B, 12, cfg, dev), avmnist_batch(B, 13, cfg, dev)
    replay = eng.capture(b1["image"], b1["audio"], b1["label"])
    graph = eng._graph
    ora = Oracle("avmnist", cfg, params)
    replay(b1["image"], b1["audio"], b1["label"])
    ora.step(cpu(b1))
    stay = ora.clone()
    eng.set_fusion_loss_weight(0.6)
    assert eng.fusion_loss_weight == 0.6 and torch.allclose(eng.loss_weights.cpu(), torch.tensor([0.6, 0.6, 1.8]))
    replay(b2["image"], b2["audio"], b2["label"])
    torch.cuda.synchronize()
    assert eng._graph is graph
    r6, r3 = ora.step(cpu(b2), w=0.6), stay.step(cpu(b2))
    assert abs(float(eng.losses[3]) - float(r6["loss"])) < FP32_ATOL
    for k in ("classifier_image.weight", "classifier_fusion.classifer.weight"):
        scale = float(ora.state["m"][k].abs().max())
        assert abserr(eng.exp_avg[k], ora.state["m"][k]) < 1e-3 * scale, k
        assert abserr(eng.exp_avg[k], stay.state["m"][k]) > 0.05 * scale, k
    perr = max(abserr(eng.params[k], ora.p[k]) for k in params if not k.endswith(NOISE_KEYS))
    assert perr < FP32_ATOL, perr
    eng.set_loss_weights(1.0, 1.0, 1.0)
    assert eng.head_weights == {"image": 1.0, "audio": 1.0, "fusion": 1.0}
    mm = MMIMDBEngine(dict(G.MMIMDB, dropout=0.0), 4, device=dev, precision="fp32", init=False)
    with pytest.raises(NotImplementedError):
        mm.set_fusion_loss_weight(0.5)


# ---------------------------------------------------------------------------------------------------------------
# the engine-backed task modules
# ---------------------------------------------------------------------------------------------------------------
def test_bound_training_steps_match_the_oracle(dev, fp32_modules):
    """AV-MNIST S, fp32, dropout 0, B = 24: three training_steps against the oracle (losses, parameters within 1e-3); the
    module's parameters ARE the engine's (same Parameter objects, storage inside engine.flat_p, state_dict bit-identical)."""
    cfg, B = dict(G.AVMNIST["S"], dropout=0.0), 24
    net, params = make_net("avmnist", cfg, 11, dev)
    ids = [id(p) for p in net.parameters()]
    eng = net.bind_engine(B, precision="fp32")
    assert net.engine is eng and [id(p) for p in net.parameters()] == ids
    with pytest.raises(RuntimeError, match="already bound"):
        net.bind_engine(B)
    lo, hi = eng.flat_p.data_ptr(), eng.flat_p.data_ptr() + eng.flat_p.numel() * 4
    for k, p in net.named_parameters():
        assert lo <= p.data_ptr() and p.data_ptr() + p.numel() * 4 <= hi, k
    ora = Oracle("avmnist", cfg, params)
    for step in range(3):
        batch = avmnist_batch(B, 20 + step, cfg, dev)
        out = net.training_step(batch, step)
        ref = ora.step(cpu(batch))
        assert set(out) == {"loss", "loss_image", "loss_audio", "loss_fusion", "preds", "labels"}
        for k in ("loss", "loss_image", "loss_audio", "loss_fusion"):
            assert abs(float(out[k]) - float(ref[k])) < FP32_ATOL, (step, k)
        assert torch.equal(out["preds"].cpu(), ref["preds"])
        assert out["loss"].data_ptr() != eng.losses.data_ptr()          # cloned: the next replay does not overwrite it
    torch.cuda.synchronize()
    assert param_err(net, ora) < FP32_ATOL
    sd, esd = net.state_dict(), eng.state_dict()
    assert list(sd) == list(esd) and all(torch.equal(sd[k], esd[k]) for k in sd)


def test_ragged_tail_between_full_batches(dev, fp32_modules):
    """24, then 10 (a training sibling; the captured main step is captured again), then 24 samples: oracle parity of every
    step's losses and of the final parameters."""
    cfg, B = dict(G.AVMNIST["S"], dropout=0.0), 24
    net, params = make_net("avmnist", cfg, 31, dev)
    net.bind_engine(B, precision="fp32")
    ora = Oracle("avmnist", cfg, params)
    for i, bs in enumerate((24, 10, 24)):
        batch = avmnist_batch(bs, 40 + i, cfg, dev)
        out = net.training_step(batch, i)
        ref = ora.step(cpu(batch))
        for k in ("loss", "loss_image", "loss_audio", "loss_fusion"):
            assert abs(float(out[k]) - float(ref[k])) < FP32_ATOL, (bs, k)
        assert out["preds"].shape == (bs,)
    torch.cuda.synchronize()
    assert param_err(net, ora) < FP32_ATOL


def test_validation_and_test_steps_and_the_module_path_after_engine_steps(dev, fp32_modules, tmp_path):
    """After bound training steps: validation_step has shared_step(mode="val")'s keys and matches the oracle forward at the
    oracle's parameters (1e-3, predictions bit-exact), at the bound batch size and a ragged one; the module's own path
    (net.eval(); shared_step) agrees -- its packed operand copies were invalidated by the engine steps.  test_step outputs
    feed save_test_preds."""
    cfg, B = dict(G.AVMNIST["S"], dropout=0.0), 24
    net, params = make_net("avmnist", cfg, 51, dev)
    net.bind_engine(B, precision="fp32")
    ora = Oracle("avmnist", cfg, params)
    for i in range(2):
        batch = avmnist_batch(B, 60 + i, cfg, dev)
        net.training_step(batch, i)
        ora.step(cpu(batch))
        if i == 0:
            net.eval()
            with torch.no_grad():                       # the module's own runtimes now exist, packed from the engine's weights
                net.shared_step(batch, mode="val")
            net.train()
    outs = []
    for bs in (B, 7):
        batch = avmnist_batch(bs, 70 + bs, cfg, dev)
        val = net.validation_step(batch, 0)
        ref = ora.forward(cpu(batch), ora.p)
        net.eval()
        with torch.no_grad():
            mod = net.shared_step(batch, mode="val")
        net.train()
        assert set(val) == set(mod)
        for k in ("logits", "image_logits", "audio_logits", "loss", "loss_image", "loss_audio", "loss_fusion"):
            assert abserr(val[k], ref[k]) < FP32_ATOL, (bs, k)
            assert abserr(mod[k], val[k]) < FP32_ATOL, (bs, k)
        for k in ("preds", "preds_image", "preds_audio"):
            assert torch.equal(val[k].cpu(), ref[k]), (bs, k)
            assert val[k].dtype == mod[k].dtype and torch.equal(val[k], mod[k]), (bs, k)
        assert torch.equal(val["labels"], batch["label"])
        outs.append(net.test_step(batch, 0))
    path = net.save_test_preds(outs, save_dir=str(tmp_path))
    dump = torch.load(path)
    assert set(dump) == set(net.TEST_PRED_KEYS) and dump["preds"].shape == (B + 7,)


def test_reduce_lr_on_plateau_reaches_the_engine(dev, fp32_modules):
    """configure_optimizers when bound: EngineOptimizer + ReduceLROnPlateau on val_loss.  A rising val_loss cuts the rate; the
    next training_step matches an oracle Adam step at the new rate.  EngineOptimizer.state_dict() loads into a plain
    torch.optim.Adam over an unbound module's parameters."""
    from torch.optim.lr_scheduler import ReduceLROnPlateau
    from m2_mixer_amd.models import EngineOptimizer
    cfg, B = dict(G.AVMNIST["S"], dropout=0.0), 24
    net, params = make_net("avmnist", cfg, 81, dev)
    net.bind_engine(B, precision="fp32")
    conf = net.configure_optimizers()
    opt, sched = conf["optimizer"], conf["lr_scheduler"]
    assert isinstance(opt, EngineOptimizer) and isinstance(sched, ReduceLROnPlateau) and conf["monitor"] == "val_loss"
    ora = Oracle("avmnist", cfg, params)
    for i in range(2):
        batch = avmnist_batch(B, 90 + i, cfg, dev)
        net.training_step(batch, i)
        ora.step(cpu(batch))
        opt.step()
        opt.zero_grad()
    for v in (1.0, 1.5, 2.0, 2.5):
        sched.step(v)
    new_lr = opt.param_groups[0]["lr"]
    assert new_lr == pytest.approx(LR * 0.1)
    batch = avmnist_batch(B, 99, cfg, dev)
    out = net.training_step(batch, 2)
    ref = ora.step(cpu(batch), lr=new_lr)
    torch.cuda.synchronize()
    assert float(net.engine.adam_state[1]) == pytest.approx(new_lr)
    assert abs(float(out["loss"]) - float(ref["loss"])) < FP32_ATOL
    assert param_err(net, ora) < FP32_ATOL
    plain_net, _ = make_net("avmnist", cfg, 82, dev)
    plain = torch.optim.Adam(plain_net.parameters(), lr=0.5)
    plain.load_state_dict(opt.state_dict())
    assert plain.param_groups[0]["lr"] == pytest.approx(new_lr)
    for (k, p), q in zip(net.named_parameters(), plain_net.parameters()):
        st = plain.state[q]
        assert float(st["step"]) == 3.0
        assert torch.equal(st["exp_avg"].to(dev), net.engine.exp_avg[k]) and torch.equal(st["exp_avg_sq"].to(dev), net.engine.exp_avg_sq[k])


def test_loss_weight_schedule_on_a_bound_mimic_module(dev, fp32_modules):
    """MIMIC-H config with fusion_loss_change: 0.05 (cfg/mimic/mimic_m2-mixer_LC.yml), fp32, dropout 0, B = 16: one step at 1/3,
    validation_epoch_end, one more step -- its loss, the fusion head's Adam moment and the parameters after it follow the
    oracle at 1/3 + 0.05 (and the moment not the oracle that kept 1/3)."""
    cfg, B = dict(G.MIMIC_H, dropout=0.0), 16
    net, params = make_net("mimic", cfg, 101, dev, fusion_loss_change=0.05)
    net.bind_engine(B, precision="fp32")
    ora = Oracle("mimic", cfg, params)
    b1 = tuple(t.to(dev) for t in G.mimic_batch(B, 102, cfg))
    net.training_step(b1, 0)
    ora.step(cpu(b1))
    net.validation_step(b1, 0)
    net.validation_epoch_end([])
    w = 1.0 / 3 + 0.05
    assert net.fusion_loss_weight == pytest.approx(w) and net.engine.fusion_loss_weight == pytest.approx(w)
    stay = ora.clone()
    b2 = tuple(t.to(dev) for t in G.mimic_batch(B, 103, cfg))
    out = net.training_step(b2, 1)
    ref = ora.step(cpu(b2), w=w)
    stay.step(cpu(b2))
    torch.cuda.synchronize()
    assert abs(float(out["loss"]) - float(ref["loss"])) < FP32_ATOL
    k = "classifier_fusion.classifer.weight"                # its gradient scales with fusion_loss_weight
    scale = float(ora.state["m"][k].abs().max())
    assert abserr(net.engine.exp_avg[k], ora.state["m"][k]) < 1e-3 * scale
    assert abserr(net.engine.exp_avg[k], old_m := stay.state["m"][k]) > 0.02 * scale, float((ora.state["m"][k] - old_m).abs().max())
    assert torch.allclose(out["preds"].sum(1), torch.ones(B, device=dev))          # MIMIC's preds: softmax probabilities
    assert param_err(net, ora) < FP32_ATOL


def test_checkpoint_resume_is_bit_identical(dev, tmp_path):
    """M2-Mixer-B, bf16, B = 128 (the bit-reproducible configuration), dropout 0: save a bound module after two steps, load the
    checkpoint into a new module, bind, restore the optimizer state, take the third step -- the parameters are bit-identical
    to three uninterrupted steps."""
    from m2_mixer_amd import models as MD
    cfg, B = dict(G.AVMNIST["B"], dropout=0.0), 128
    net, _ = make_net("avmnist", cfg, 111, dev)
    net.bind_engine(B, precision="bf16")
    net.configure_optimizers()
    batches = [avmnist_batch(B, 112 + i, cfg, dev) for i in range(3)]
    for i in range(2):
        net.training_step(batches[i], i)
    ck = net.save_checkpoint(str(tmp_path / "two.ckpt"), epoch=0, global_step=2)
    net.training_step(batches[2], 2)
    torch.cuda.synchronize()
    ckpt = torch.load(ck, weights_only=True)
    assert len(ckpt["optimizer_states"]) == 1 and float(ckpt["optimizer_states"][0]["state"][0]["step"]) == 2.0
    again = MD.AVMnistMixerMultiLoss.load_from_checkpoint(ck, model_cfg=_model_cfg("avmnist", cfg),
                                                          optimizer_cfg={"lr": LR, "scheduler_patience": 1}).to(dev)
    again.bind_engine(B, precision="bf16")
    again.configure_optimizers()["optimizer"].load_state_dict(ckpt["optimizer_states"][0])
    again.training_step(batches[2], 2)
    torch.cuda.synchronize()
    assert torch.equal(again.engine.flat_p, net.engine.flat_p)
    assert torch.equal(again.engine.flat_m, net.engine.flat_m) and torch.equal(again.engine.flat_v, net.engine.flat_v)


@pytest.mark.parametrize("task,B", [("mmimdb", 32), ("mimic", 128)])
def test_bound_wide_models_bf16_vs_oracle(task, B, dev):
    """MM-IMDb at B = 32 (with a fixed `mute: image`: the image input is zeroed in training) and MIMIC-H at B = 128, bf16:
    the bound training_step's losses against the oracle, then validation_step's logits (no muting) against the oracle
    forward at the oracle's updated parameters, at the bf16 tolerances of the engine tests."""
    if task == "mmimdb":
        cfg = dict(G.MMIMDB, dropout=0.0)
        net, params = make_net(task, cfg, 121, dev, mute="image")
        image, text, labels = G.mmimdb_batch(B, 122, cfg)
        batch = {"image": image.to(dev), "text": text.to(dev), "label": labels.to(dev)}
        train_ref_batch = {"image": torch.zeros_like(image), "text": text, "label": labels}
        loss_keys, logit_keys = ("loss", "loss_image", "loss_text", "loss_fusion"), ("image_logits", "text_logits", "logits")
    else:
        cfg = dict(G.MIMIC_H, dropout=0.0)
        net, params = make_net(task, cfg, 131, dev)
        batch = tuple(t.to(dev) for t in G.mimic_batch(B, 132, cfg))
        train_ref_batch = cpu(batch)
        loss_keys, logit_keys = ("loss", "loss_static", "loss_time", "loss_fusion"), ("logits_static", "logits_time", "logits")
    net.bind_engine(B, precision="bf16")
    if task == "mmimdb":
        assert all(c.pos_weight is net.engine.pos_weight for c in (net.image_criterion, net.text_criterion, net.fusion_criterion))
    ora = Oracle(task, cfg, params)
    out = net.training_step(batch, 0)
    ref = ora.step(train_ref_batch)
    for k in loss_keys:
        err = abs(float(out[k]) - float(ref[k]))
        assert observe(f"bound {task} bf16 step loss (abs)", err, BF16_LOGITS) < BF16_LOGITS * max(1.0, abs(float(ref[k]))), k
    val = net.validation_step(batch, 0)
    vref = ora.forward(cpu(batch), ora.p)
    for k in logit_keys:
        tol = BF16_LOGITS * max(1.0, float(vref[k].abs().max()))
        assert observe(f"bound {task} bf16 logits after a step (abs)", abserr(val[k], vref[k]), tol) < tol, k
