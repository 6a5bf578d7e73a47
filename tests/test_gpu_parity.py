"""GPU parity tests (-m gpu): the HIP path, called through the C ABI (libm2mixer.so via ctypes), against
  (a) the CPU oracle on the same seeded inputs,
  (b) the golden vectors captured from the reference's own modules (tests/golden/*.npz),
  (c) size-independent properties at the benchmark's full size (batch 512).

Tolerances
  fp32 mode (exact fp32 MFMA): logits / activations 1e-3 absolute as BASELINE.json's north_star states
      (observed ~1e-6), gradients 1e-3 relative to the tensor's max;
  bf16 mode (bf16 operands, fp32 accumulate): logits / activations 2e-2 (BF16_REL; observed 5.5e-3), gradients 4e-2
      relative to the tensor's max (BF16_GRAD_REL; observed 1.4e-2); class predictions: the argmax of the kernel's own logits,
      equal to the oracle's wherever the oracle's top-2 margin exceeds twice the observed logit error (assert_preds_bf16) --
      bit-exact predictions are asserted in fp32 mode only.  Observed maxima are printed in the test summary (conftest.observe).
"""
import os

import numpy as np
import pytest
import torch

import drop_ref as DR
import gen_util as G
from conftest import observe
from golden_util import check, load
from oracle import m2mixer_oracle as O

pytestmark = pytest.mark.gpu

FP32_ATOL = 1e-3
BF16_REL = 2e-2        # (observed maxima are printed in the test summary)
BF16_GRAD_REL = 4e-2   # gradients, relative to the tensor's max (the same bar as tests/test_gpu_bench_path.py)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from m2_mixer_amd import _lib
    _lib.lib()      # the HIP library must be there: no fallback
    return torch.device("cuda:0")


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max()) / (float(b.abs().max()) + 1e-12)


def grads_cleared(eng):
    """After an optimizer step every gradient element Adam is responsible for clearing is zero: everything outside the ranges
    the engine leaves to the next backward's overwriting weight-gradient launch (engine._setup_wgrad)."""
    g = eng.flat_g.detach().clone()
    for lo, n, _, keep in eng._ranges_add:
        if keep:
            g[lo:lo + n] = 0
    return float(g.abs().max()) == 0.0


def abserr(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def assert_preds_bf16(pred, logits_gpu, logits_ref):
    """bf16 mode: the kernel's predictions are the argmax of its own logits, and equal the oracle's on every sample whose
    top-2 margin in the oracle exceeds twice the logit error observed in this very comparison (if |l - ref| <= e everywhere,
    the argmax can only differ where the margin is <= 2e; random-init logits do produce such near-ties: one sample of the
    B = 40 case has a margin of 3e-4).  fp32 mode asserts bit-exact predictions instead."""
    lg = logits_gpu.detach().float().cpu()
    assert torch.equal(pred.cpu().long(), lg.argmax(1))
    e = float((lg - logits_ref).abs().max())
    top2 = logits_ref.topk(2, dim=1).values
    decided = (top2[:, 0] - top2[:, 1]) > 2 * e
    assert float(decided.float().mean()) >= 0.75, "too many near-ties for the prediction check to mean anything"
    assert torch.equal(pred.cpu().long()[decided], logits_ref.argmax(1)[decided])


def run_block(case, B, prec, dev, p_drop=0.0, seed=0):
    import m2_mixer_amd as M
    from m2_mixer_amd import modules as MM
    N, D, T, Cc = case
    M.set_precision(prec)
    p, x, dy = G.block_case_tensors(case, B, seed=1000 + seed)
    blk = MM.MixerBlock(D, N, T, Cc, dropout=p_drop).to(dev)
    blk.load_state_dict(p)
    blk.train()
    xg = x.to(dev).requires_grad_(True)
    y = blk(xg)
    (y * dy.to(dev)).sum().backward()
    torch.cuda.synchronize()
    return blk, p, x, dy, y, xg


# every block shape of SURVEY.md section 8c(i): N <= 8 runs on the fused path, the MIMIC / MM-IMDb shapes
# (N = 24, 25, 40, 80; D = 256) on the wide path
GPU_BLOCK_CASES = list(enumerate(G.BLOCK_CASES))


@pytest.mark.parametrize("ci,case", GPU_BLOCK_CASES)
def test_block_fp32_vs_golden_and_oracle(ci, case, dev):
    """Single MixerBlock forward + backward, fp32 mode, against the reference's golden vectors (B = 2) and the
    oracle (B = 37: ragged last tile)."""
    gold = load("blocks.npz")
    B = int(gold[f"case{ci}//shape"][0])
    blk, p, x, dy, y, xg = run_block(case, B, "fp32", dev, seed=ci)
    check(gold, f"case{ci}//y", y, FP32_ATOL)
    check(gold, f"case{ci}//dx", xg.grad, FP32_ATOL)
    for k, prm in blk.named_parameters():
        scale = max(1.0, float(np.abs(gold[f"case{ci}//grad//{k}//l2"])))
        check(gold, f"case{ci}//grad//{k}", prm.grad, FP32_ATOL * scale, 1e-3)
    # ragged batch against the oracle
    blk, p, x, dy, y, xg = run_block(case, 37, "fp32", dev, seed=ci)
    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    xr = x.clone().requires_grad_(True)
    yo = O.mixer_block(xr, leaves)
    (yo * dy).sum().backward()
    assert abserr(y, yo) < FP32_ATOL
    assert abserr(xg.grad, xr.grad) < FP32_ATOL
    for k, prm in blk.named_parameters():
        assert relerr(prm.grad, leaves[k].grad) < 1e-3, k


@pytest.mark.parametrize("ci,case", GPU_BLOCK_CASES)
def test_block_bf16_vs_oracle(ci, case, dev):
    blk, p, x, dy, y, xg = run_block(case, 37, "bf16", dev, seed=ci)
    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    xr = x.clone().requires_grad_(True)
    yo = O.mixer_block(xr, leaves)
    (yo * dy).sum().backward()
    path = "wide" if case[0] > 8 or case[1] > 128 else "fused"
    assert observe(f"bf16 block {path} out (rel to max)", relerr(y, yo), BF16_REL) < BF16_REL
    assert observe(f"bf16 block {path} dx (rel to max)", relerr(xg.grad, xr.grad), BF16_REL) < BF16_REL
    for k, prm in blk.named_parameters():
        cls = ("LN" if ".0." in k and "net" not in k else "bias" if k.endswith("bias") else
               "token W" if k.startswith("token_mix") else "channel W")
        assert observe(f"bf16 block {path} {cls} (rel to max)", relerr(prm.grad, leaves[k].grad), BF16_REL) < BF16_REL, k


@pytest.mark.parametrize("p_drop", [0.5, 0.1])
@pytest.mark.parametrize("case", [(4, 128, 32, 3072), (8, 32, 16, 256), (24, 64, 16, 64), (40, 256, 16, 512)])
def test_block_dropout_masks_match_oracle(case, p_drop, dev):
    """Training-mode dropout: export the keep-masks the kernels regenerate (forward, backward and the
    weight-gradient pass all recompute them) and feed them to the oracle: every output and gradient
    must agree, which pins placement, scaling and cross-kernel consistency of the masks."""
    import m2_mixer_amd as M
    N, D, T, Cc = case
    B = 5
    blk, p, x, dy, y, xg = run_block(case, B, "fp32", dev, p_drop=p_drop, seed=3)
    rt, st, sd = blk._rt, blk._drop_step, M.config.dropout_seed()
    masks = {"tok_h": rt.dropout_mask(0, 0, B, sd, st).view(B, D, T), "tok_o": rt.dropout_mask(0, 1, B, sd, st).view(B, D, N),
             "ch_h": rt.dropout_mask(0, 2, B, sd, st).view(B, N, rt.Cp)[:, :, :Cc], "ch_o": rt.dropout_mask(0, 3, B, sd, st).view(B, N, D)}
    masks = {k: v.float().cpu() for k, v in masks.items()}
    thr = DR.drop_thr(p_drop)
    p_eff = 1 - thr / 65536            # keep probability is quantised to 16 bits; the kernels scale by 1/(1-p_eff)
    for k, m in masks.items():
        tol = max(0.03, 5 * 0.5 / m.numel() ** 0.5)      # 5 sigma of a Bernoulli mean over the mask's elements
        assert abs(float(m.mean()) - (1 - p_eff)) < tol, (k, float(m.mean()))
    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    xr = x.clone().requires_grad_(True)
    yo = O.mixer_block(xr, leaves, "", p_eff, masks)
    (yo * dy).sum().backward()
    assert abserr(y, yo) < FP32_ATOL
    assert abserr(xg.grad, xr.grad) < FP32_ATOL
    for k, prm in blk.named_parameters():
        assert relerr(prm.grad, leaves[k].grad) < 1e-3, k
    # a second forward draws a different mask; eval() disables dropout
    y2 = blk(x.to(dev))
    assert not torch.equal(y2, y.detach())
    blk.eval()
    ye = blk(x.to(dev))
    assert abserr(ye, O.mixer_block(x, p)) < FP32_ATOL


def _engine(size, B, prec, dev, dropout=None):
    from m2_mixer_amd.engine import AVMnistEngine
    cfg = dict(G.AVMNIST[size])
    if dropout is not None:
        cfg["dropout"] = dropout
    return AVMnistEngine(cfg, B, device=dev, precision=prec, lr=1e-2, init=False), cfg


@pytest.mark.parametrize("size,B,seed", [("S", 8, 11), ("M", 4, 21), ("B", 8, 12)])
def test_avmnist_step_fp32_vs_reference_golden(size, B, seed, dev):
    """Whole training step (towers + fusion + three heads + multi-head loss + backward + Adam) in fp32 mode
    against the vectors recorded from the reference: logits within 1e-3, class predictions identical."""
    gold = load(f"avmnist_{size}.npz")
    eng, cfg = _engine(size, B, "fp32", dev, dropout=0.0)
    shapes = G.avmnist_shapes(cfg)
    eng.load_state_dict(dict(G.make_params(shapes, seed)))
    image, audio, labels = (t.to(dev) for t in G.avmnist_batch(B, seed + 1, cfg))
    eng.forward_backward(image, audio, labels)          # gradients are consumed (cleared) by optimizer_step: look first
    torch.cuda.synchronize()
    check(gold, "step0//logits", eng.logits[2], FP32_ATOL)
    check(gold, "step0//image_logits", eng.logits[0], FP32_ATOL)
    check(gold, "step0//audio_logits", eng.logits[1], FP32_ATOL)
    for i, k in enumerate(("loss_image", "loss_audio", "loss_fusion", "loss")):
        check(gold, f"step0//{k}", eng.losses[i], FP32_ATOL)
    assert np.array_equal(eng.preds[2].cpu().numpy(), gold["step0//preds"])
    assert np.array_equal(eng.preds[0].cpu().numpy(), gold["step0//preds_image"])
    assert np.array_equal(eng.preds[1].cpu().numpy(), gold["step0//preds_audio"])
    for k in shapes:
        check(gold, f"grad//{k}", eng.grads[k], 1e-4, 1e-3, what="grad ")
    eng.optimizer_step()
    assert grads_cleared(eng), "Adam must leave the gradient buffer cleared"
    # second step goes through the Adam update
    eng.train_step(image, audio, labels)
    torch.cuda.synchronize()
    check(gold, "step1//logits", eng.logits[2], 5e-3)
    assert np.array_equal(eng.preds[2].cpu().numpy(), gold["step1//preds"])
    # (the parameters after the two Adam steps, and Adam's moments, are checked against the oracle's optimizer state in
    #  tests/test_gpu_bench_path.py::test_adam_moments_and_parameters_vs_oracle, at 2 % of lr)


@pytest.mark.parametrize("size,B", [("S", 8), ("B", 40), ("B", 13)])      # 13: ragged row tiles in every launch
def test_avmnist_step_bf16_vs_oracle(size, B, dev):
    eng, cfg = _engine(size, B, "bf16", dev, dropout=0.0)
    shapes = G.avmnist_shapes(cfg)
    params = dict(G.make_params(shapes, 7))
    eng.load_state_dict(params)
    image, audio, labels = G.avmnist_batch(B, 8, cfg)
    eng.forward_backward(image.to(dev), audio.to(dev), labels.to(dev))
    torch.cuda.synchronize()
    ref = O.avmnist_train_step(image, audio, labels, params, cfg, {}, lr=1e-2)
    assert observe("bf16 logits (abs)", abserr(eng.logits[2], ref["logits"]), BF16_REL) < BF16_REL
    assert observe("bf16 logits (abs)", abserr(eng.logits[0], ref["image_logits"]), BF16_REL) < BF16_REL
    assert observe("bf16 logits (abs)", abserr(eng.logits[1], ref["audio_logits"]), BF16_REL) < BF16_REL
    assert abs(float(eng.losses[3]) - float(ref["loss"])) < 1e-2
    assert_preds_bf16(eng.preds[2], eng.logits[2], ref["logits"])
    assert_preds_bf16(eng.preds[0], eng.logits[0], ref["image_logits"])
    assert_preds_bf16(eng.preds[1], eng.logits[1], ref["audio_logits"])
    for k, g in ref["grads"].items():
        if k.endswith("token_mix.2.net.3.bias"):
            continue
        assert observe("bf16 gradients (rel to max)", relerr(eng.grads[k], g), BF16_GRAD_REL) < BF16_GRAD_REL, k


@pytest.mark.parametrize("prec,B", [("fp32", 1), ("fp32", 3), ("bf16", 1), ("bf16", 5)])
def test_avmnist_eval_tiny_and_odd_batches_vs_oracle(prec, B, dev):
    """validation / test step (dropout off) on batches smaller than any tile of the kernels: a single sample, odd counts --
    every launch of the step runs with ragged row tiles, partial sample groups and mostly-empty workgroups."""
    eng, cfg = _engine("B", B, prec, dev)                   # cfg dropout 0.5: evaluate() must ignore it
    shapes = G.avmnist_shapes(cfg)
    params = dict(G.make_params(shapes, 31))
    eng.load_state_dict(params)
    image, audio, labels = G.avmnist_batch(B, 32, cfg)
    out = eng.evaluate(image.to(dev), audio.to(dev), labels.to(dev))
    torch.cuda.synchronize()
    ref = O.avmnist_forward(image, audio, labels, params, cfg)
    tol = FP32_ATOL if prec == "fp32" else BF16_REL
    for k in ("logits", "image_logits", "audio_logits"):
        assert abserr(out[k], ref[k]) < tol, k
    assert abs(float(out["loss"]) - float(ref["loss"])) < (1e-3 if prec == "fp32" else 2e-2)
    if prec == "fp32":
        assert torch.equal(out["preds"].cpu().long(), ref["preds"])


def test_module_path_towers_and_no_patching(dev):
    """The reference-shaped nn.Modules (registry -> MLPMixer / FusionMixer / MLPMixerNoPatching) under torch
    autograd, fp32 mode, against the oracle."""
    import m2_mixer_amd as M
    from m2_mixer_amd import modules as MM
    M.set_precision("fp32")
    cfg = G.MIMIC_H["time"]
    shapes = G.tower_shapes("", cfg, cfg["num_patch"], "proj")
    params = G.make_params(shapes, 5)
    for N in (8, cfg["num_patch"]):              # fused path (N = 8) and the MIMIC time tower as configured (N = 24: wide path)
        cfgN = {**cfg, "num_patch": N}
        tower = MM.get_block_by_name(block_type="MLPMixerNoPatching", in_channels=1, **cfgN, dropout=0.0).to(dev)
        paramsN = G.make_params(G.tower_shapes("", cfgN, N, "proj"), 5)
        tower.load_state_dict(paramsN)
        x = torch.randn(9, N, 12)
        y = tower(x.to(dev))                       # the tower input is data: no gradient is produced for it
        y.square().sum().backward()
        leaves = {k: v.clone().requires_grad_(True) for k, v in paramsN.items()}
        yo = O.mlp_mixer_no_patching(x, leaves, "", 1)
        yo.square().sum().backward()
        assert abserr(y, yo) < FP32_ATOL
        for k, prm in tower.named_parameters():
            if k.endswith("token_mix.2.net.3.bias"):      # exactly-zero true gradient (the next LayerNorm removes it): noise only
                assert float(prm.grad.abs().max()) < 1e-3
                continue
            assert relerr(prm.grad, leaves[k].grad) < 1e-3, (N, k)
        # eval forward (no saved activations: the wide path streams through its workspaces)
        tower.eval()
        with torch.no_grad():
            ye = tower(x.to(dev))
        assert abserr(ye, yo) < FP32_ATOL


def test_full_size_properties(dev):
    """Batch 512 (BASELINE.json configs[1]) properties that need no oracle run at that size:
       * samples are independent: the first 64 samples of the batch give the same eval logits alone;
       * eval is deterministic and dropout-free; hipGraph replay == eager launch for the same step counter;
       * gradient of the summed loss w.r.t. the final-LN bias of the fusion tower == column sums of d(tokens)
         (checked through the linearity of the heads: scaling all head weights scales that gradient)."""
    from m2_mixer_amd.engine import AVMnistEngine
    cfg = dict(G.AVMNIST["B"])
    B = 512
    eng = AVMnistEngine(cfg, B, device=dev, precision="bf16", lr=1e-3, seed=42)
    image, audio, labels = (t.to(dev) for t in G.avmnist_batch(B, 99, cfg))
    out = eng.evaluate(image, audio, labels)
    l1 = out["logits"].clone()
    out = eng.evaluate(image, audio, labels)
    assert torch.equal(l1, out["logits"]), "eval forward must be deterministic"
    small = AVMnistEngine(cfg, 64, device=dev, precision="bf16", lr=1e-3, seed=42)
    small.load_state_dict(eng.state_dict())
    o2 = small.evaluate(image[:64].contiguous(), audio[:64].contiguous(), labels[:64].contiguous())
    assert torch.equal(o2["logits"], l1[:64]), "a sample's logits must not depend on the rest of the batch"
    assert torch.isfinite(l1).all()
    # eager vs graph: same parameters, same Adam state, same dropout counter -> same losses and same updated weights
    a = AVMnistEngine(cfg, B, device=dev, precision="bf16", lr=1e-3, seed=42)
    a.load_state_dict(eng.state_dict())
    a.train_step(image, audio, labels)
    torch.cuda.synchronize()
    la, pa = a.losses.clone(), a.flat_p.clone()
    b = AVMnistEngine(cfg, B, device=dev, precision="bf16", lr=1e-3, seed=42)
    replay = b.capture(image, audio, labels)          # capture runs warm-up steps: rewind the state afterwards
    b.load_state_dict(eng.state_dict())
    b.flat_m.zero_(); b.flat_v.zero_(); b.flat_g.zero_(); b.adam_state[0] = 0.0; b.drop_step.zero_()
    replay()
    torch.cuda.synchronize()
    assert torch.allclose(b.losses, la, rtol=0, atol=1e-5)
    # float atomics make the order of a few small sums non-deterministic: Adam's first step is lr * sign(g)-like,
    # so compare the update direction statistically rather than bit for bit
    agree = float(((b.flat_p - eng.flat_p).sign() == (pa - eng.flat_p).sign()).float().mean())
    assert agree > 0.999, agree
    assert grads_cleared(b)
    # losses are sane for random init: each head near ln(10)
    assert all(abs(float(v) - np.log(10)) < 0.5 for v in la[:3])


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_grouped_launches_match_single_launches(prec, dev):
    """The one-launch entry points the replayed step uses (m2m_embeds_forward with its k-split partial sums,
    m2m_towers_wgrad carrying the two patch embeddings, m2m_pack_all) against the single-object entry points on the same
    inputs, at the benchmark's batch: same arithmetic, only the order of a few fp32 sums differs."""
    from m2_mixer_amd.engine import AVMnistEngine
    from m2_mixer_amd.runtime import embeds_forward, pack_all, towers_wgrad
    cfg = dict(G.AVMNIST["B"])
    B = 512 if prec == "bf16" else 64
    eng = AVMnistEngine(cfg, B, device=dev, precision=prec, lr=1e-3, seed=3)
    image, audio, labels = (t.to(dev) for t in G.avmnist_batch(B, 5, cfg))
    if prec == "bf16":
        assert eng.x0_splits[1] == 2 and eng.x0_splits[0] == 1       # audio: fast path with a k-split; image: generic path
    else:
        assert eng.x0_splits == (1, 1)
    # ---- patch embeddings: grouped (+ partial sums) vs one launch each
    embeds_forward([eng.e_a, eng.e_b], [image, audio], [eng._x0_a, eng._x0_b], B, list(eng.x0_splits))
    got_a, got_b = eng._x0_a.sum(0), eng._x0_b.sum(0)
    ref_a, ref_b = torch.empty_like(got_a), torch.empty_like(got_b)
    eng.e_a.forward(image, B, ref_a)
    eng.e_b.forward(audio, B, ref_b)
    torch.cuda.synchronize()
    assert relerr(got_a, ref_a) < 1e-5 and relerr(got_b, ref_b) < 1e-5
    # an input the fast path cannot take (not 16-byte aligned) still honours the requested partial sums
    odd = torch.empty(audio.numel() + 1, device=dev)[1:].view_as(audio).copy_(audio)
    assert odd.data_ptr() % 16 != 0
    eng._x0_b.fill_(7.0)
    embeds_forward([eng.e_a, eng.e_b], [image, odd], [eng._x0_a, eng._x0_b], B, list(eng.x0_splits))
    torch.cuda.synchronize()
    assert relerr(eng._x0_b.sum(0), ref_b) < 1e-5
    # ---- weight gradients: towers + embeddings in one launch vs separate launches (after a real forward / backward)
    eng.forward_backward(image, audio, labels)
    torch.cuda.synchronize()
    g_merged = eng.flat_g.clone()
    keys = [k for k in eng.grads if "to_patch_embedding" in k or                  # what the weight-gradient launch computes
            k.endswith(("channel_mix.1.net.0.weight", "channel_mix.1.net.0.bias", "channel_mix.1.net.3.weight"))]
    assert len(keys) == 3 * 10 + 4
    for k in keys:
        eng.grads[k].zero_()
    for t in (eng.t_fus, eng.t_a, eng.t_b):
        t.wgrad(B, eng.seed, 0, eng.drop_step)
    eng.e_a.wgrad(image, eng.dx0_a, B)
    eng.e_b.wgrad(audio, eng.dx0_b, B)
    torch.cuda.synchronize()
    for k in keys:
        g = eng.grads[k]
        o = (g.data_ptr() - eng.flat_g.data_ptr()) // 4
        # (the single-owner embedding gradients of the merged launch sum the bf16 image of d_x0^T for the bias too; the
        # separate launch sums the fp32 d_x0: bf16 rounding of the summands, 2^-9 each)
        bias_bf16 = prec == "bf16" and k.endswith("to_patch_embedding.0.bias")
        tol = 3e-3 if bias_bf16 else 1e-4
        err = relerr(g_merged[o:o + g.numel()].view_as(g), g)
        if bias_bf16:
            observe("bf16 embedding bias grad, single-owner vs fp32 sum", err, tol)      # (parity unpinned by the reference)
        assert err < tol, k
    # ---- operand packing: the whole model in one launch vs per tower / per embedding, bit for bit
    towers, embeds = [eng.t_a, eng.t_b, eng.t_fus], [eng.e_a, eng.e_b]
    pack_all(towers, embeds)
    torch.cuda.synchronize()
    packed = [[{k: v.clone() for k, v in t._keep[f"packed{i}"].items()} for i in range(t.nblocks)] for t in towers]
    wn = [e._keep["wn"].clone() for e in embeds]
    for t in towers:
        for i in range(t.nblocks):
            for v in t._keep[f"packed{i}"].values():
                v.zero_()
        t.pack(force=True)
    for e in embeds:
        e._keep["wn"].zero_()
        e.pack(force=True)
    torch.cuda.synchronize()
    for t, pt in zip(towers, packed):
        for i in range(t.nblocks):
            for k, v in t._keep[f"packed{i}"].items():
                if k == "w1tc" and t.pack_all_skips_w1tc():      # (pack_all leaves the copy nothing reads unwritten)
                    continue
                assert torch.equal(v, pt[i][k]), k
    for e, w in zip(embeds, wn):
        assert torch.equal(e._keep["wn"], w)


@pytest.mark.parametrize("task", ["avmnist_slots", "mmimdb_pair_launches", "mimic_streams", "mimic_mlp_ride_heads_pool", "mmimdb_heads_pool"])
def test_launch_forms_of_a_step_agree(task, dev, monkeypatch):
    """The launch forms the engines choose by default against the forms they replace, same parameters / batch / dropout
    stream: (a) AV-MNIST B bf16: small parameter gradients of all three towers through per-workgroup slots reduced inside the
    weight-gradient launch (M2M_WGRAD_GROUP_SLOTS / _REDUCES_SMALL) vs float atomics + a reduction launch of its own;
    (b) MM-IMDb: both modality towers per launch on one stream (m2m_towers_forward / _backward with wide pairs) vs one launch
    per tower on two streams; (c) MIMIC-H: one stream vs three; (d) MIMIC-H: the static MLP riding in the time tower's token-mixing
    launches (m2m_mlp_forward_ride / _backward_ride) and the heads pooling the tower outputs (m2m_head.tokens) vs the MLP's own
    launches and the token-mean launches; (e) MM-IMDb: heads pooling vs token-mean launches.  Same arithmetic; only the order of
    fp32 sums may differ."""
    from m2_mixer_amd.engine import AVMnistEngine, MimicEngine, MMIMDBEngine
    if task == "avmnist_slots":
        cfg, B, prec = dict(G.AVMNIST["B"]), 64, "bf16"
        make = lambda: AVMnistEngine(cfg, B, device=dev, precision=prec, lr=1e-3, seed=3)
        batch = G.avmnist_batch(B, 5, cfg)
        alt_env = {"M2M_GROUP_SLOTS": "0", "M2M_DEFER_SMALL": "0"}
    elif task in ("mmimdb_pair_launches", "mmimdb_heads_pool"):
        cfg, B, prec = dict(G.MMIMDB), 5, "fp32"
        make = lambda: MMIMDBEngine(cfg, B, device=dev, precision=prec, lr=1e-3, seed=3)
        batch = G.mmimdb_batch(B, 5, cfg)
        alt_env = {"M2M_CONCURRENT": "0"} if task == "mmimdb_pair_launches" else {"M2M_HEADS_POOL": "0"}
    else:
        cfg, B, prec = dict(G.MIMIC_H), 16, "fp32"
        make = lambda: MimicEngine(cfg, B, device=dev, precision=prec, lr=1e-3, seed=3)
        batch = G.mimic_batch(B, 5, cfg)
        alt_env = {"M2M_MIMIC_STREAMS": "both"} if task == "mimic_streams" else {"M2M_MLP_RIDE": "0", "M2M_HEADS_POOL": "0"}
    batch = tuple(t.to(dev) for t in batch)
    eng = make()
    for k, v in alt_env.items():
        monkeypatch.setenv(k, v)
    alt = make()
    alt.load_state_dict(eng.state_dict())
    if task == "avmnist_slots":
        assert eng.t_a.desc.wgrad_flags & 4 and eng.t_fus.desc.wgrad_flags & 2 and not (alt.t_a.desc.wgrad_flags & 6)
    if task == "mimic_mlp_ride_heads_pool":
        assert eng._mlp_ride and eng._heads_pool and not alt._mlp_ride and not alt._heads_pool
    if task == "mmimdb_heads_pool":
        assert eng._heads_pool and not alt._heads_pool
    if task == "mmimdb_pair_launches":
        from m2_mixer_amd.runtime import can_group
        assert can_group(eng.t_a, eng.t_b, B) and eng.concurrent and not alt.concurrent
    for e in (eng, alt):
        e.forward_backward(*batch)
    torch.cuda.synchronize()
    # (with the static split of the backward column loop -- the default -- bf16 forms differ like fp32 ones: observed 3e-7;
    # under M2M_BWD_TICKETS=1 two bf16 runs of the SAME form differ by ~2e-3 of a gradient's largest element)
    tol = 2e-4 if os.environ.get("M2M_BWD_TICKETS", "0") == "0" or prec == "fp32" else 1e-2
    assert relerr(eng.logits, alt.logits) < 1e-5
    worst = 0.0
    for k in eng.grads:
        ga, gb = eng.grads[k], alt.grads[k]
        if float(gb.abs().max()) == 0.0:
            assert float(ga.abs().max()) == 0.0, k
            continue
        assert relerr(ga, gb) < tol, (k, relerr(ga, gb))
        worst = max(worst, relerr(ga, gb))
    observe(f"launch forms [{task}] gradients (rel to max)", worst, tol)


def test_bf16_training_is_bit_reproducible(dev):
    """Two engines, same parameters / batch / dropout stream, default launch forms (static split of the backward column loop,
    small gradients, the second weight-gradient row group and the classification heads' weight gradients through slots with
    a fixed summation order, single-owner embedding gradients): every gradient is BIT-identical between the runs, and so
    are the parameters after three captured optimizer steps.  (The per-head losses are still summed with float atomics:
    reported values only.)"""
    from m2_mixer_amd.engine import AVMnistEngine
    cfg, B = dict(G.AVMNIST["B"]), 128
    make = lambda: AVMnistEngine(cfg, B, device=dev, precision="bf16", lr=1e-3, seed=3)
    eng = make()
    alt = make()
    alt.load_state_dict(eng.state_dict())
    batch = tuple(t.to(dev) for t in G.avmnist_batch(B, 5, cfg))
    for e in (eng, alt):
        e.forward_backward(*batch)
    torch.cuda.synchronize()
    assert eng._head_part is not None and torch.equal(eng.logits, alt.logits)
    differing = [k for k in eng.grads if not torch.equal(eng.grads[k], alt.grads[k])]
    assert not differing, differing
    for e in (eng, alt):
        e.optimizer_step()
        for _ in range(3):
            e.train_step(*batch)
    torch.cuda.synchronize()
    assert torch.equal(eng.flat_p, alt.flat_p)
    assert relerr(eng.losses, alt.losses) < 1e-6


def test_training_reduces_loss_bf16(dev):
    """A few dozen Adam steps on one fixed synthetic batch must overfit it (end-to-end sanity of fwd, bwd,
    wgrad, Adam and re-packing of the weights in bf16 mode with dropout on)."""
    from m2_mixer_amd.engine import AVMnistEngine
    cfg = dict(G.AVMNIST["S"])
    B = 64
    eng = AVMnistEngine(cfg, B, device=dev, precision="bf16", lr=3e-3, seed=1)
    image, audio, labels = (t.to(dev) for t in G.avmnist_batch(B, 3, cfg))
    replay = eng.capture(image, audio, labels)
    first = None
    for i in range(150):
        replay()
        if i == 0:
            torch.cuda.synchronize()
            first = float(eng.losses[3])
    torch.cuda.synchronize()
    out = eng.evaluate(image, audio, labels)
    assert float(out["loss"]) < 0.5 * first, (first, float(out["loss"]))
    assert float((out["preds"].long() == labels).float().mean()) > 0.9


def test_unsupported_shapes_are_refused(dev):
    from m2_mixer_amd import modules as MM
    blk = MM.MixerBlock(48, 4, 16, 64).to(dev)          # hidden_dim 48 has no kernel instantiation
    with pytest.raises(RuntimeError, match="hidden_dim"):
        blk(torch.zeros(2, 4, 48, device=dev))
    blk = MM.MixerBlock(32, 4, 12, 64).to(dev)          # token_dim must be a multiple of 8 on the fused path
    with pytest.raises(RuntimeError, match="token_dim"):
        blk(torch.zeros(2, 4, 32, device=dev))
    blk = MM.MixerBlock(32, 200, 16, 64).to(dev)        # more tokens than the wide path's LDS tiles hold
    with pytest.raises(RuntimeError, match="num_patch"):
        blk(torch.zeros(2, 200, 32, device=dev))
    blk = MM.MixerBlock(32, 24, 40, 64).to(dev)         # token_dim above the register budget of the token kernels
    with pytest.raises(RuntimeError, match="token_dim"):
        blk(torch.zeros(2, 24, 32, device=dev))
    # one step past each limit of the envelope (tests/shape_cases.py holds the largest accepted shapes)
    import m2_mixer_amd as M
    from m2_mixer_amd import _lib as L
    from m2_mixer_amd.runtime import EmbedRuntime
    from shape_cases import LDS_EDGE
    before = M.config.get_precision()
    M.set_precision("fp32")
    try:
        blk = MM.MixerBlock(32, 129, 16, 64).to(dev)    # num_patch 129 > 128
        with pytest.raises(RuntimeError, match="num_patch"):
            blk(torch.zeros(2, 129, 32, device=dev))
        blk = MM.MixerBlock(32, 24, 33, 64).to(dev)     # token_dim 33 > 32
        with pytest.raises(RuntimeError, match="token_dim"):
            blk(torch.zeros(2, 24, 32, device=dev))
        blk = MM.MixerBlock(32, 4, 16, 4097).to(dev)    # Cp 4128 > 8 x 512 threads
        with pytest.raises(RuntimeError, match="channel_dim"):
            blk(torch.zeros(2, 4, 32, device=dev))
        # the fused path's LDS: the largest accepted (nblocks, Cp) with one more channel column (Cp + 32): the forward fits,
        # the backward launch's LDS does not
        e = LDS_EDGE
        tower = MM.FusionMixer(e["D"], e["N"], e["nb"], e["T"], e["C"] + 1).to(dev)
        with pytest.raises(RuntimeError, match="channel_dim"):
            tower(torch.zeros(2, e["N"], e["D"], device=dev, requires_grad=True)).sum().backward()
        tower = MM.MLPMixerNoPatching(32, 4, 1, 16, 64, 3969, 32).to(dev)       # Kp > 3968
        with pytest.raises(RuntimeError, match=r"Cin\*ph\*pw"):
            tower(torch.zeros(2, 4, 3969, device=dev))
        # a 30 x 28 image in 14 x 14 patches (MLPMixer's constructor refuses it as the reference does, with an AssertionError)
        ert = EmbedRuntime(1, 30, 28, 14, 14, 32, L.PREC_F32)
        w, b = torch.zeros(32, 1, 14, 14, device=dev), torch.zeros(32, device=dev)
        ert.bind_params(w, b)
        with pytest.raises(RuntimeError, match="image not divisible by patch"):
            ert.forward(torch.zeros(2, 1, 30, 28, device=dev), 2, torch.empty(2, 2, 32, device=dev))
        mlp = MM.MLP(129, 64, 1).to(dev)                # layer width 129 > 128
        with pytest.raises(RuntimeError, match="widths"):
            mlp(torch.zeros(2, 129, device=dev))
        # a refusal leaves no error or runtime state behind: a valid forward in the same process still matches the oracle
        p, x, _ = G.block_case_tensors((5, 32, 16, 33), 3, seed=77)
        blk = MM.MixerBlock(32, 5, 16, 33).to(dev)
        blk.load_state_dict(p)
        blk.eval()
        with torch.no_grad():
            y = blk(x.to(dev))
        assert abserr(y, O.mixer_block(x.double(), {k: v.double() for k, v in p.items()})) < 1e-4
    finally:
        M.set_precision(before)


# ---------------------------------------------------------------------------------------------------------------
# MIMIC-H and MM-IMDb: the wide tower path, the static MLP,
# BCE heads -- whole training step against the vectors recorded from the reference
# ---------------------------------------------------------------------------------------------------------------
def test_mimic_step_fp32_vs_reference_golden(dev):
    from m2_mixer_amd.engine import MimicEngine
    gold = load("mimic_H.npz")
    cfg = dict(G.MIMIC_H, dropout=0.0)
    B = 6
    eng = MimicEngine(cfg, B, device=dev, precision="fp32", lr=1e-2, init=False)
    shapes = G.mimic_shapes(cfg)
    assert list(eng.shapes.keys()) == list(shapes.keys()) and eng.n_params == int(gold["n_params"])
    eng.load_state_dict(dict(G.make_params(shapes, 31)))
    static, time, labels = (t.to(dev) for t in G.mimic_batch(B, 32, cfg))
    eng.forward_backward(static, time, labels)
    torch.cuda.synchronize()
    check(gold, "logits", eng.logits[2], FP32_ATOL)
    check(gold, "logits_static", eng.logits[0], FP32_ATOL)
    check(gold, "logits_time", eng.logits[1], FP32_ATOL)
    for i, k in enumerate(("loss_static", "loss_time", "loss_fusion", "loss")):
        check(gold, k, eng.losses[i], FP32_ATOL)
    check(gold, "time_tokens", eng.fused[:, 1:, :], FP32_ATOL)
    check(gold, "fusion_tokens", eng.fus_out, FP32_ATOL)
    for k in shapes:
        check(gold, f"grad//{k}", eng.grads[k], 1e-4, 1e-3, what="grad ")
    # the update itself: one Adam step moves every parameter with a non-zero gradient by ~lr
    before = eng.flat_p.clone()
    eng.optimizer_step()
    torch.cuda.synchronize()
    assert grads_cleared(eng)
    assert float((eng.flat_p - before).abs().max()) <= 1e-2 * 1.001


def test_mmimdb_step_fp32_vs_reference_golden(dev):
    from m2_mixer_amd.engine import MMIMDBEngine
    gold = load("mmimdb.npz")
    cfg = dict(G.MMIMDB, dropout=0.0)
    B = 3
    eng = MMIMDBEngine(cfg, B, device=dev, precision="fp32", lr=1e-3, init=False)
    shapes = G.mmimdb_shapes(cfg)
    assert list(eng.shapes.keys()) == list(shapes.keys()) and eng.n_params == int(gold["n_params"])
    eng.load_state_dict(dict(G.make_params(shapes, 51)))
    image, text, labels = (t.to(dev) for t in G.mmimdb_batch(B, 52, cfg))
    eng.forward_backward(image, text, labels)
    torch.cuda.synchronize()
    check(gold, "logits", eng.logits[2], FP32_ATOL)
    check(gold, "image_logits", eng.logits[0], FP32_ATOL)
    check(gold, "text_logits", eng.logits[1], FP32_ATOL)
    for i, k in enumerate(("loss_image", "loss_text", "loss_fusion", "loss")):
        check(gold, k, eng.losses[i], FP32_ATOL)
    assert np.array_equal(eng.preds[2].cpu().numpy(), gold["preds"])
    for k in shapes:
        check(gold, f"grad//{k}", eng.grads[k], 1e-4, 1e-3, what="grad ")


@pytest.mark.parametrize("task", ["mimic", "mmimdb"])
def test_wide_models_bf16_vs_oracle_and_training(task, dev):
    """bf16 mode on the wide path against the oracle (dropout off), then a captured training run with the configs'
    dropout on (p = 0.3: 16-bit-draw masks; p = 0.5: one-bit masks) must overfit one batch."""
    from m2_mixer_amd.engine import MimicEngine, MMIMDBEngine
    if task == "mimic":
        cfg, B = dict(G.MIMIC_H), 40
        shapes = G.mimic_shapes(cfg)
        batch = G.mimic_batch(B, 5, cfg)
        mk = lambda c, lr: MimicEngine(c, B, device=dev, precision="bf16", lr=lr, init=False)
        fwd = lambda p: O.mimic_forward(*batch, p, cfg)
        names = ("logits_static", "logits_time", "logits")
    else:
        cfg, B = dict(G.MMIMDB), 6
        shapes = G.mmimdb_shapes(cfg)
        batch = G.mmimdb_batch(B, 5, cfg)
        mk = lambda c, lr: MMIMDBEngine(c, B, device=dev, precision="bf16", lr=lr, init=False)
        fwd = lambda p: O.mmimdb_forward(*batch, p, cfg, torch.tensor(cfg["pos_weight"]))
        names = ("image_logits", "text_logits", "logits")
    params = dict(G.make_params(shapes, 9))
    eng = mk(dict(cfg, dropout=0.0), 1e-3)
    eng.load_state_dict(params)
    gb = tuple(t.to(dev) for t in batch)
    eng.forward_backward(*gb)
    torch.cuda.synchronize()
    leaves = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    ref = fwd(leaves)
    ref["loss"].backward()
    for i, k in enumerate(names):
        assert observe("bf16 logits (abs)", abserr(eng.logits[i], ref[k]), BF16_REL) < BF16_REL * max(1.0, float(ref[k].detach().abs().max())), k
    assert abs(float(eng.losses[3]) - float(ref["loss"].detach())) < 2e-2 * max(1.0, abs(float(ref["loss"].detach())))
    for k, leaf in leaves.items():
        if k.endswith("token_mix.2.net.3.bias"):      # exactly-zero true gradient
            continue
        assert observe("bf16 gradients (rel to max)", relerr(eng.grads[k], leaf.grad), BF16_GRAD_REL) < BF16_GRAD_REL, k
    # training with dropout on
    eng = mk(cfg, 2e-3)
    eng.load_state_dict(params)
    first = float(eng.evaluate(*gb)["loss"])
    replay = eng.capture(*gb)
    for _ in range(300):
        replay()
    torch.cuda.synchronize()
    last = float(eng.evaluate(*gb)["loss"])
    assert np.isfinite(last) and last < 0.85 * first, (first, last)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_mimic_large_batch_token_gradients_vs_oracle(prec, dev):
    """Batch 2500 on the wide path: the token-mixing backward walks several column blocks per workgroup (more than 1024
    blocks in the launch, a ragged last workgroup) and accumulates the token-weight gradients in LDS, the LayerNorm-1 backward
    takes its larger row groups.  Every gradient against autograd through the oracle."""
    from m2_mixer_amd.engine import MimicEngine
    cfg, B = dict(G.MIMIC_H), 2500
    cfg["dropout"] = 0.0
    shapes = G.mimic_shapes(cfg)
    params = dict(G.make_params(shapes, 19))
    batch = G.mimic_batch(B, 23, cfg)
    eng = MimicEngine(cfg, B, device=dev, precision=prec, lr=1e-3, init=False)
    eng.load_state_dict(params)
    eng.forward_backward(*(t.to(dev) for t in batch))
    torch.cuda.synchronize()
    leaves = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    ref = O.mimic_forward(*batch, leaves, cfg)
    ref["loss"].backward()
    tol_l, tol_g = (FP32_ATOL, 2e-3) if prec == "fp32" else (BF16_REL, BF16_GRAD_REL)
    assert abserr(eng.logits[2], ref["logits"]) < tol_l * max(1.0, float(ref["logits"].detach().abs().max()))
    assert abs(float(eng.losses[3]) - float(ref["loss"].detach())) < (1e-3 if prec == "fp32" else 2e-2)
    for k, leaf in leaves.items():
        if k.endswith("token_mix.2.net.3.bias"):      # exactly-zero true gradient
            continue
        assert relerr(eng.grads[k], leaf.grad) < tol_g, k


def test_mlp_ride_is_the_mlp_launch_with_or_without_a_carrier(dev):
    """m2m_mlp_forward_ride / _backward_ride record the MLP call; a small token-mixing launch of a wide tower carries it, or
    m2m_mlp_ride_flush launches it on its own.  Either way the results are those of m2m_mlp_forward / _backward, bit for bit
    (same device code); a second recorded call while one is pending is refused; a flush with nothing pending is a no-op."""
    from m2_mixer_amd import _lib as L
    from m2_mixer_amd.runtime import MlpRuntime
    cs = G.MIMIC_H["static"]
    B, p_drop = 48, 0.3
    shapes = {k: v for k, v in G.mimic_shapes(G.MIMIC_H).items() if k.startswith("static_extractor.")}
    params = {k: v.to(dev) for k, v in G.make_params(shapes, 3).items()}
    keys = [f"static_extractor.module_list.{i}." for i in (0, 3, 6)]
    dims = [cs["input_dim"], cs["hidden_dim"], cs["hidden_dim"], cs["output_dim"]]
    x = torch.randn(B, cs["input_dim"], device=dev)
    d1, d2 = torch.randn(B, 3, cs["output_dim"], device=dev), torch.randn(B, cs["output_dim"], device=dev)

    def run(ride: bool):
        grads = {k: torch.zeros_like(v) for k, v in params.items()}
        rt = MlpRuntime(dims, True, p_drop, 77)
        rt.bind([(params[k + "weight"], params[k + "bias"]) for k in keys], [(grads[k + "weight"], grads[k + "bias"]) for k in keys], B)
        out = torch.zeros(B, 3, cs["output_dim"], device=dev)
        dense = torch.zeros(B, cs["output_dim"], device=dev)
        if ride:
            rt.forward_ride(x, B, out, 3 * cs["output_dim"], dense, True, 123, 1)
            with pytest.raises(RuntimeError):                 # one pending call per host thread
                rt.forward_ride(x, B, out, 3 * cs["output_dim"], dense, True, 123, 1)
            rt.ride_flush()                                   # no carrier: a launch of its own
            rt.ride_flush()                                   # nothing pending: no-op
            rt.backward_ride(x, B, d1, 3 * cs["output_dim"], d2)
            rt.ride_flush()
        else:
            rt.forward(x, B, out, 3 * cs["output_dim"], dense, True, 123, 1)
            rt.backward(x, B, d1, 3 * cs["output_dim"], d2)
        torch.cuda.synchronize()
        return out, dense, grads

    a, b = run(False), run(True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for k in a[2]:
        assert relerr(a[2][k], b[2][k]) < 1e-6, k            # (weight gradients: float atomics over 3 workgroups)


def test_static_mlp_dropout_consistency(dev):
    """The MIMIC static MLP (Linear-ReLU-Dropout x2 + Linear) with dropout on: forward equals the oracle under the
    masks the kernel drew (read back from the saved activations), backward equals autograd through those masks."""
    from m2_mixer_amd.runtime import MlpRuntime
    cs = G.MIMIC_H["static"]
    B, p_drop = 97, 0.3
    shapes = {k: v for k, v in G.mimic_shapes(G.MIMIC_H).items() if k.startswith("static_extractor.")}
    params = {k: v.to(dev) for k, v in G.make_params(shapes, 3).items()}
    grads = {k: torch.zeros_like(v) for k, v in params.items()}
    keys = [f"static_extractor.module_list.{i}." for i in (0, 3, 6)]
    rt = MlpRuntime([cs["input_dim"], cs["hidden_dim"], cs["hidden_dim"], cs["output_dim"]], True, p_drop, 77)
    rt.bind([(params[k + "weight"], params[k + "bias"]) for k in keys], [(grads[k + "weight"], grads[k + "bias"]) for k in keys], B)
    x = torch.randn(B, cs["input_dim"], device=dev)
    out = torch.zeros(B, 3, cs["output_dim"], device=dev)            # strided destination: token 0 of a (B, 3, D) buffer
    dense = torch.zeros(B, cs["output_dim"], device=dev)
    rt.forward(x, B, out, 3 * cs["output_dim"], dense, True, 123, 1)
    torch.cuda.synchronize()
    acts = [a.cpu() for a in rt._keep["act"][:2]]
    thr = DR.drop_thr(p_drop)
    scale = 65536.0 / thr
    leaves = {k[len("static_extractor."):]: v.detach().cpu().clone().requires_grad_(True) for k, v in params.items()}
    h = x.cpu()
    keep_rates = []
    for i, a in enumerate(acts):
        z = torch.relu(h @ leaves[f"module_list.{3 * i}.weight"].T + leaves[f"module_list.{3 * i}.bias"])
        mask = (a != 0).float()
        keep_rates.append(float(mask[z.detach() > 1e-6].mean()))
        h = z * mask * scale
        assert abserr(a, h) < 1e-4
    yo = h @ leaves["module_list.6.weight"].T + leaves["module_list.6.bias"]
    assert abserr(dense, yo) < 1e-4 and torch.equal(out[:, 0, :], dense) and float(out[:, 1:, :].abs().max()) == 0.0
    assert all(abs(r - thr / 65536) < 0.05 for r in keep_rates), keep_rates
    d1, d2 = torch.randn(B, 3, cs["output_dim"], device=dev), torch.randn(B, cs["output_dim"], device=dev)
    rt.backward(x, B, d1, 3 * cs["output_dim"], d2)
    torch.cuda.synchronize()
    (yo * (d1[:, 0, :] + d2).cpu()).sum().backward()
    for k, g in grads.items():
        assert relerr(g, leaves[k[len("static_extractor."):]].grad) < 1e-4, k
    # eval: no dropout
    rt.forward(x, B, out, 3 * cs["output_dim"], dense, False, 123, 2)
    ye = O.mlp(x.cpu(), {k: v.cpu() for k, v in params.items()}, "static_extractor.", 2, True)
    assert abserr(dense, ye) < 1e-4


def test_data_parallel_step_path_matches_fused_step(dev):
    """The multi-GPU step is captured as two graphs with the gradient all-reduce between them (forward + backward |
    exchange | Adam + re-pack).  With an identity exchange it must produce the same losses and the same update as the
    fused single-GPU step (which applies Adam per tower inside one graph)."""
    from m2_mixer_amd.engine import AVMnistEngine
    cfg = dict(G.AVMNIST["S"])
    B = 48
    batch = tuple(t.to(dev) for t in G.avmnist_batch(B, 5, cfg))
    calls = []

    def exchange(flat):                     # stands in for parallel.GradSync: sees the flat gradient, returns the scale
        calls.append(int(flat.numel()))
        return 1.0

    a = AVMnistEngine(cfg, B, device=dev, precision="bf16", lr=1e-3, seed=3)
    b = AVMnistEngine(cfg, B, device=dev, precision="bf16", lr=1e-3, seed=3)
    b.load_state_dict(a.state_dict())
    ra = a.capture(*batch)
    rb = b.capture(*batch, grad_sync=exchange)
    for e in (a, b):                        # rewind what the capture warm-ups changed
        e.load_state_dict(a.state_dict() if e is a else b.state_dict())
    b.load_state_dict(a.state_dict())
    for e in (a, b):
        e.flat_m.zero_(); e.flat_v.zero_(); e.flat_g.zero_(); e.adam_state[0] = 0.0; e.drop_step.zero_()
    p0 = a.flat_p.clone()
    for _ in range(3):
        ra(); rb()
    torch.cuda.synchronize()
    assert calls and all(n == a.n_params for n in calls)
    assert torch.allclose(a.losses, b.losses, rtol=0, atol=2e-3), (a.losses, b.losses)     # float-atomic order in the small gradients
    assert grads_cleared(b) and grads_cleared(a)
    da, db = a.flat_p - p0, b.flat_p - p0
    assert float((da - db).abs().max()) <= 2e-3 * 3 * 0.51      # a few sign flips of ~0 gradients at most (lr = 1e-3, 3 steps)
    assert float((da.sign() == db.sign()).float().mean()) > 0.995


def test_pipelined_exchange_update_is_bit_identical_to_the_whole_buffer_update(dev):
    """parallel.PipelinedGradSync: the step's tail runs per parameter segment (all-reduce of chunk k + 1 behind Adam + re-pack
    of chunk k).  With one rank the exchange is the identity, so three captured steps must leave EXACTLY the parameters,
    moments and packed operand copies of the whole-buffer form (forward + backward | exchange | Adam + pack_all): Adam is
    elementwise, the chunks partition the buffers, the kept gradient ranges are cut at the chunk bounds."""
    from m2_mixer_amd import parallel
    from m2_mixer_amd.engine import AVMnistEngine
    cfg, B = dict(G.AVMNIST["B"]), 64
    batch = tuple(t.to(dev) for t in G.avmnist_batch(B, 5, cfg))
    make = lambda: AVMnistEngine(cfg, B, device=dev, precision="bf16", lr=1e-3, seed=3)
    a, b, c = make(), make(), make()
    for e in (b, c):
        e.load_state_dict(a.state_dict())
    chunks = b._update_chunks()
    assert [lo for lo, _, _ in chunks] == sorted(lo for lo, _, _ in chunks) and chunks[0][0] == 0 and chunks[-1][1] == b.n_params
    assert len(chunks) == 3 and all(chunks[i][1] == chunks[i + 1][0] for i in range(2))
    ra = a.capture(*batch, grad_sync=lambda flat: 1.0)              # whole-buffer form with an identity exchange
    rb = b.capture(*batch, grad_sync=parallel.PipelinedGradSync())  # per-segment graphs
    for _ in range(3):
        ra(); rb()
        c.train_step(*batch, grad_sync=parallel.PipelinedGradSync())     # the same, eager
    torch.cuda.synchronize()
    for e in (b, c):
        assert torch.equal(a.flat_p, e.flat_p) and torch.equal(a.flat_m, e.flat_m) and torch.equal(a.flat_v, e.flat_v)
        assert grads_cleared(e)
        for ta, te in ((a.t_a, e.t_a), (a.t_b, e.t_b), (a.t_fus, e.t_fus)):
            for i in range(ta.nblocks):
                for k, v in ta._keep[f"packed{i}"].items():
                    if k == "w1tc" and ta.pack_all_skips_w1tc():     # (written by the per-tower re-pack only; nothing reads it)
                        continue
                    assert torch.equal(v, te._keep[f"packed{i}"][k]), k
        for ea, ee in ((a.e_a, e.e_a), (a.e_b, e.e_b)):
            assert torch.equal(ea._keep["wn"], ee._keep["wn"])


def test_adam_from_bf16_gradient_equals_adam_from_widened_gradient(dev):
    """The data-parallel step hands Adam the all-reduced gradient as bf16 (GradSync(widen=False)); the update must be
    bit-identical to widening that bf16 gradient into the fp32 buffer first, and the fp32 buffer must come out cleared."""
    from m2_mixer_amd.engine import AVMnistEngine
    cfg = dict(G.AVMNIST["S"])
    a = AVMnistEngine(cfg, 8, device=dev, precision="bf16", lr=1e-2, seed=1)
    b = AVMnistEngine(cfg, 8, device=dev, precision="bf16", lr=1e-2, seed=1)
    b.load_state_dict(a.state_dict())
    g = torch.randn(a.n_params, device=dev) * 1e-2
    gb = g.to(torch.bfloat16)
    for e in (a, b):
        e._prologue()
    a.flat_g.copy_(gb)                      # reference: widen, then the fp32 Adam
    a.optimizer_step(0.5)
    b.flat_g.copy_(g)                       # the local fp32 gradient stays in place and is only cleared
    b.optimizer_step(0.5, gb)
    torch.cuda.synchronize()
    assert torch.equal(a.flat_p, b.flat_p) and torch.equal(a.flat_m, b.flat_m) and torch.equal(a.flat_v, b.flat_v)
    assert grads_cleared(b)


# ---------------------------------------------------------------------------------------------------------------
# the callers: Lightning-free task modules with the reference's constructor / shared_step contract (models.py)
# ---------------------------------------------------------------------------------------------------------------
def _model_cfg(task):
    if task == "avmnist":
        c = G.AVMNIST["S"]
        mods = {"image": dict(c["image"], block_type="MLPMixer"), "audio": dict(c["audio"], block_type="MLPMixer"),
                "multimodal": dict(c["multimodal"], block_type="FusionMixer", fusion_function="ConcatFusion")}
        hid = c["multimodal"]["hidden_dim"]
    elif task == "mimic":
        c = G.MIMIC_H
        mods = {"static": dict(c["static"], block_type="MLP"), "time": dict(c["time"], block_type="MLPMixerNoPatching"),
                "multimodal": dict(c["multimodal"], block_type="FusionMixer", fusion_function="ConcatFusion")}
        hid = c["multimodal"]["hidden_dim"]
    else:
        c = G.MMIMDB
        mods = {"image": dict(c["image"], block_type="MLPMixer"), "text": dict(c["text"], block_type="MLPMixer"),
                "multimodal": dict(c["multimodal"], block_type="FusionMixer", fusion_function="ConcatFusion")}
        hid = c["multimodal"]["hidden_dim"]
    mods["classification"] = dict(classifier="StandardClassifier", num_classes=c["num_classes"], input_shape=[16, 49, hid])
    cfg = {"dropout": 0.0, "modalities": mods}
    if task == "mmimdb":
        cfg["pos_weight"] = c["pos_weight"]
    return cfg, c


@pytest.mark.parametrize("task", ["avmnist", "mimic", "mmimdb"])
def test_task_modules_shared_step_vs_reference_golden(task, dev):
    """AVMnistMixerMultiLoss / MimicMixerMultiLoss / MMIMDBMixerMultiLoss built from cfg dicts like the reference builds
    them (registry, `.num_patch`, fusion shape algebra), weights loaded through the reference's state-dict keys, fp32
    mode: shared_step's logits / losses and the autograd gradients against the reference's recorded vectors."""
    import m2_mixer_amd as M
    from m2_mixer_amd import models as MD
    M.set_precision("fp32")
    model_cfg, c = _model_cfg(task)
    opt_cfg = {"lr": 1e-2, "betas": (0.9, 0.999), "scheduler_patience": 2}
    if task == "avmnist":
        gold, seed, B = load("avmnist_S.npz"), 11, 8
        net = MD.AVMnistMixerMultiLoss(model_cfg, opt_cfg).to(dev)
        shapes = G.avmnist_shapes(dict(c, dropout=0.0))
        image, audio, labels = (t.to(dev) for t in G.avmnist_batch(B, seed + 1, c))
        batch = {"image": image, "audio": audio, "label": labels}
        names = {"logits": "step0//logits", "image_logits": "step0//image_logits", "audio_logits": "step0//audio_logits",
                 "loss": "step0//loss", "loss_image": "step0//loss_image", "loss_audio": "step0//loss_audio",
                 "loss_fusion": "step0//loss_fusion"}
    elif task == "mimic":
        gold, seed, B = load("mimic_H.npz"), 31, 6
        net = MD.MimicMixerMultiLoss(model_cfg, opt_cfg).to(dev)
        shapes = G.mimic_shapes(c)
        batch = tuple(t.to(dev) for t in G.mimic_batch(B, 32, c))
        names = {k: k for k in ("logits", "logits_static", "logits_time", "loss", "loss_fusion", "loss_static", "loss_time")}
    else:
        gold, seed, B = load("mmimdb.npz"), 51, 3
        net = MD.MMIMDBMixerMultiLoss(model_cfg, opt_cfg).to(dev)
        shapes = G.mmimdb_shapes(c)
        image, text, labels = (t.to(dev) for t in G.mmimdb_batch(B, 52, c))
        batch = {"image": image, "text": text, "label": labels}
        names = {k: k for k in ("logits", "image_logits", "text_logits", "loss", "loss_image", "loss_text", "loss_fusion")}
    assert [k for k, _ in net.named_parameters()] == list(shapes.keys()), "parameter names / creation order must match the reference"
    net.load_state_dict(G.make_params(shapes, seed), strict=False)     # (MM-IMDb: the criteria's pos_weight buffers keep the cfg values)
    net.train()
    out = net.shared_step(batch, mode="train")
    out["loss"].backward()
    torch.cuda.synchronize()
    for k, gk in names.items():
        check(gold, gk, out[k], FP32_ATOL)
    if task == "avmnist":
        assert np.array_equal(out["preds"].cpu().numpy(), gold["step0//preds"])
    if task == "mmimdb":
        assert np.array_equal(out["preds"].cpu().numpy(), gold["preds"])
    for k, prm in net.named_parameters():
        check(gold, f"grad//{k}", prm.grad, 1e-4, 1e-3, what="grad ")
    opt = net.configure_optimizers()
    assert isinstance(opt["optimizer"], torch.optim.Adam) and opt["monitor"] == "val_loss"
    # the fused engine over the same weights gives the same losses
    eng = net.to_engine(B, precision="fp32")
    eb = tuple(batch.values()) if isinstance(batch, dict) else batch
    res = eng.evaluate(*eb)
    assert abs(float(res["loss"]) - float(out["loss"].detach())) < FP32_ATOL
    # freezing the unimodal parts (models/avmnist.py:314-324): their parameters stop requiring grad, training loss = fusion loss
    if task != "mimic":
        net._freeze_modalities()
        o2 = net.shared_step(batch, mode="train")
        assert float((o2["loss"] - o2["loss_fusion"]).detach().abs()) == 0.0
        assert not any(p.requires_grad for p in net.image_mixer.parameters())
        assert all(p.requires_grad for p in net.fusion_mixer.parameters())


def test_resident_pipeline_trains_end_to_end(dev, tmp_path):
    """SURVEY section 8f rows f1-f3 together: dataset in the reference's .npy layout resident in HBM, batches as views,
    the captured training step, device-side loss / accuracy accumulators, ReduceLROnPlateau on the device-side lr: two
    epochs on a small learnable set must classify the held-out split."""
    from test_host_cpu import _write_avmnist
    from m2_mixer_amd.data import PlateauLR, ResidentAVMnist, run_epoch
    from m2_mixer_amd.engine import AVMnistEngine
    root = str(tmp_path / "avmnist")
    _write_avmnist(root, 1440, 100, seed=3, learnable=True)
    data = ResidentAVMnist(root, device=dev)
    cfg, B = dict(G.AVMNIST["S"]), 120
    eng = AVMnistEngine(cfg, B, device=dev, precision="bf16", lr=3e-3, seed=0)
    image, audio, labels = next(iter(data.batches("train", B)))
    replay = eng.capture(image, audio, labels)
    sched = PlateauLR(eng, 3e-3, patience=2)
    logs = []
    first = run_epoch(eng, data, "val", B, train=False)
    for _ in range(4):
        tr = run_epoch(eng, data, "train", B, train=True, log_interval_steps=4, replay=replay, log=logs.append)
        va = run_epoch(eng, data, "val", B, train=False)
        sched.step(va["loss"])
    assert tr["steps"] == 11 and tr["samples"] == 1320 and len(logs) >= 4 * 3
    assert va["loss"] < 0.5 * first["loss"] and va["acc"] > 0.8, (first, va)
    # the test split (shuffled on the device) through a second engine sized for its batch, same weights
    small = AVMnistEngine(cfg, 100, device=dev, precision="bf16", lr=3e-3, seed=0)
    small.load_state_dict(eng.state_dict())
    te = run_epoch(small, data, "test", 100, train=False)
    assert te["acc"] > 0.8, te


def test_multi_step_graph_equals_single_steps(dev):
    """capture(steps=3): three consecutive training steps (own input slots, own dropout draws, own Adam steps) in one
    hipGraph give the per-step losses of three single-step replays."""
    from m2_mixer_amd.engine import AVMnistEngine
    cfg, B = dict(G.AVMNIST["S"]), 32
    batches = [tuple(t.to(dev) for t in G.avmnist_batch(B, 40 + i, cfg)) for i in range(3)]
    a = AVMnistEngine(cfg, B, device=dev, precision="bf16", lr=1e-3, seed=5)
    b = AVMnistEngine(cfg, B, device=dev, precision="bf16", lr=1e-3, seed=5)
    ra = a.capture(*batches[0])
    rb = b.capture(*batches[0], steps=3)
    for e in (a, b):                        # rewind what the capture warm-ups changed
        e.load_state_dict(AVMnistEngine(cfg, B, device=dev, precision="bf16", lr=1e-3, seed=5).state_dict())
        e.flat_m.zero_(); e.flat_v.zero_(); e.flat_g.zero_(); e.adam_state[0] = 0.0; e.drop_step.zero_()
    singles = []
    for bt in batches:
        ra(*bt)
        singles.append(a.losses.clone())
    multi = rb(*[t for bt in batches for t in bt]).clone()
    torch.cuda.synchronize()
    assert multi.shape == (3, 4)
    for i in range(3):
        assert torch.allclose(multi[i], singles[i], rtol=0, atol=2e-3), (i, multi[i], singles[i])
    assert float(b.adam_state[0]) == 3.0 and int(b.drop_step[0]) == 3
    with pytest.raises(ValueError):
        rb(*batches[0])                     # a 3-step graph wants 3 batches (or none: reuse the slots)
