"""The classification heads (m2m_heads_ce / m2m_heads_bce and their _w forms) called directly (-m gpu), against the float64
restatement of tests/leaf_ref.py: logits, per-head losses, the weighted total, predictions, d_pooled, g_w and g_b over a
covering set of hidden_dim x workgroup shape x K x B x head count x input form (leaf_ref.HEAD_CASES), the g_part slots, the
numerical edges of both losses, the accumulation contract and the refusals.

Bars: the project's fp32 bar, 1e-4 relative to the tensor's max, for every float tensor; losses absolutely at 1e-4 x
max(1, |loss|).  Predictions are compared exactly wherever the float64 margin (CE: best minus second-best logit; BCE: |logit|)
exceeds 10 x the logits bar, and fewer than 1 % of a case's decisions may be excluded (the inputs are built so that the float64
reference alone satisfies that: tests/test_host_leaf_ref.py).  Every error is recorded per loss kind and tensor
(conftest.observe)."""
import pytest
import torch

import leaf_ref as R
from conftest import observe

pytestmark = pytest.mark.gpu

BAR = R.FP32_REL
SENT = -777.25            # sentinel of buffers a call must not write


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from m2_mixer_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def rel(got, ref):
    ref = R.f64(ref)
    return float((R.f64(got) - ref).abs().max()) / (float(ref.abs().max()) + 1e-300)


def run_heads(case, inp, dev, zero_losses=True, losses_fill=None, training=True, coef_by_value=None):
    """One call of the case's entry point; returns the outputs and the gradient buffers."""
    from m2_mixer_amd import _lib as L
    from m2_mixer_amd.runtime import heads_bce, heads_ce
    B, D, K, nh = case["B"], case["D"], case["K"], len(case["forms"])
    keep, hd = [], []
    tiles = L.lib().m2m_heads_part_tiles(B)
    gpart = torch.full((nh, tiles, L.SPLIT_GPART), SENT, device=dev) if case["gpart"] else None
    fill = SENT if (case["gpart"] or not training) else 0.0           # atomics add onto zero; untouched buffers keep the sentinel
    for h, f in enumerate(case["forms"]):
        d = dict(w=inp["ws"][h].to(dev), b=inp["bs"][h].to(dev), g_w=torch.full((K, D), fill, device=dev),
                 g_b=torch.full((K,), fill, device=dev), d_pooled=torch.full((B, D), SENT, device=dev) if training else None,
                 weight=(coef_by_value or case["coef"])[h])
        if f == "p":
            d["pooled"] = inp["xs"][h].to(dev).contiguous()
        else:
            buf = inp["bufs"][h].to(dev).contiguous()
            d["tokens"] = (buf, f[1], buf.shape[1])
        if gpart is not None:
            d["g_part"] = gpart[h]
        hd.append(d)
    weights = torch.tensor(case["coef"], dtype=torch.float32, device=dev) if case["dev_weights"] else None
    out = None
    if losses_fill is not None:
        out = (torch.empty(nh, B, K, device=dev), torch.full((nh + 1,), float(losses_fill), device=dev),
               torch.empty((nh, B, K) if case["bce"] else (nh, B), dtype=torch.int32, device=dev))
    labels = inp["labels"].to(dev)
    if case["bce"]:
        logits, losses, preds = heads_bce(hd, labels, inp["pos_weight"].to(dev), B, D, K, out=out, zero_losses=zero_losses, weights=weights)
    else:
        logits, losses, preds = heads_ce(hd, labels, B, D, K, out=out, zero_losses=zero_losses, weights=weights)
    torch.cuda.synchronize()
    return dict(logits=logits, losses=losses, preds=preds, heads=hd, gpart=gpart)


def check_forward(kind, got, ref, losses_offset=0.0):
    assert observe(f"heads {kind} logits (rel to max)", rel(got["logits"], ref["logits"]), BAR) < BAR
    for i, (g, r) in enumerate(zip(R.f64(got["losses"]).tolist(), ref["losses"].tolist())):
        tol = BAR * max(1.0, abs(r))
        assert observe(f"heads {kind} losses (abs / max(1, |loss|))", abs(g - losses_offset - r) / max(1.0, abs(r)), BAR) < BAR, (i, g, r, tol)
    ok = R.decided(ref)
    assert float((~ok).float().mean()) < R.PRED_EXCLUDED_MAX
    assert torch.equal(got["preds"].cpu().long()[ok], ref["preds"][ok])


def check_grads(kind, got, ref, case):
    K, D = case["K"], case["D"]
    for h, hd in enumerate(got["heads"]):
        assert observe(f"heads {kind} d_pooled (rel to max)", rel(hd["d_pooled"], ref["d_pooled"][h]), BAR) < BAR, h
        if case["gpart"]:
            slots = got["gpart"][h].double().cpu()
            g_w, g_b = slots[:, :K * D].sum(0).view(K, D), slots[:, K * D:K * D + K].sum(0)
            assert float(slots[:, K * D + K:K * D + K + 2].abs().max()) == 0.0            # the two trailing slot entries
            assert bool((hd["g_w"] == SENT).all()) and bool((hd["g_b"] == SENT).all())    # g_w / g_b themselves untouched
        else:
            g_w, g_b = hd["g_w"], hd["g_b"]
        assert observe(f"heads {kind} g_w (rel to max)", rel(g_w, ref["g_w"][h]), BAR) < BAR, h
        assert observe(f"heads {kind} g_b (rel to max)", rel(g_b, ref["g_b"][h]), BAR) < BAR, h


@pytest.mark.parametrize("case", R.HEAD_CASES, ids=lambda c: c["name"])
def test_heads_vs_float64(case, dev):
    """Every output of one training call against float64.  Cases with device weights pass a wrong by-value coefficient, which
    the _w entry points must ignore."""
    inp, ref = R.head_inputs(case)
    got = run_heads(case, inp, dev, coef_by_value=[99.0] * len(case["forms"]) if case["dev_weights"] else None)
    kind = "bce" if case["bce"] else "ce"
    check_forward(kind, got, ref)
    check_grads(kind, got, ref, case)


def test_ce_large_logits_stay_finite_and_ties_take_the_first_index(dev):
    """Pooled rows scaled so that the logits reach about +-80: loss, dlogits (through d_pooled, g_w, g_b) stay finite and within
    the bar of the float64 log-softmax.  Then two identical weight rows with equal biases that carry the maximum: bit-equal
    logits, and the prediction is the first of the two indices."""
    case = dict(name="ce large", B=5, D=64, K=10, forms=["p", "p"], coef=[1.0, 0.5], bce=False, gpart=False, dev_weights=False)
    gen = torch.Generator().manual_seed(31)
    xs = [30.0 * torch.randn(5, 64, generator=gen) for _ in range(2)]
    ws = [torch.randn(10, 64, generator=gen) / 8.0 for _ in range(2)]
    bs = [0.1 * torch.randn(10, generator=gen) for _ in range(2)]
    labels = torch.tensor([0, 9, 3, 7, 5])
    inp = dict(xs=xs, bufs=[None, None], ws=ws, bs=bs, labels=labels, pos_weight=None)
    ref = R.heads(xs, ws, bs, case["coef"], labels)
    assert 60.0 < float(ref["logits"].abs().max()) < 160.0
    got = run_heads(case, inp, dev)
    for t in (got["logits"], got["losses"]) + tuple(h[k] for h in got["heads"] for k in ("d_pooled", "g_w", "g_b")):
        assert bool(torch.isfinite(t).all())
    check_forward("ce large", got, ref)
    check_grads("ce large", got, ref, case)
    # ties: rows 3 and 7 identical and dominant (positive rows x positive weights)
    xs = [torch.randn(5, 64, generator=gen).abs()]
    w = torch.randn(10, 64, generator=gen) / 8.0
    w[3] = w[7] = 3.0 * torch.rand(64, generator=gen) / 8.0
    b = torch.zeros(10)
    case = dict(case, forms=["p"], coef=[1.0])
    inp = dict(xs=xs, bufs=[None], ws=[w], bs=[b], labels=labels, pos_weight=None)
    ref = R.heads(xs, [w], [b], [1.0], labels)
    assert torch.equal(ref["logits"][0].argmax(1), torch.full((5,), 3))          # float64: rows 3 / 7 carry the maximum
    got = run_heads(case, inp, dev)
    assert torch.equal(got["logits"][0, :, 3], got["logits"][0, :, 7])
    assert got["preds"][0].tolist() == [3] * 5
    assert observe("heads ce tie logits (rel to max)", rel(got["logits"], ref["logits"]), BAR) < BAR
    check_grads("ce tie", got, ref, case)


def test_bce_overflowing_logits_and_the_zero_logit(dev):
    """Logits beyond +-100 (exp overflows in fp32): loss and gradients finite and within the bar of float64.  A head with zero
    weights and bias has logits exactly 0: sigmoid = 0.5 is not > 0.5, so it predicts 0 everywhere."""
    case = dict(name="bce large", B=5, D=64, K=10, forms=["p", "p"], coef=[1.0, 2.0], bce=True, gpart=False, dev_weights=False)
    gen = torch.Generator().manual_seed(37)
    xs = [60.0 * torch.randn(5, 64, generator=gen), torch.randn(5, 64, generator=gen)]
    ws = [torch.randn(10, 64, generator=gen) / 8.0, torch.zeros(10, 64)]
    bs = [0.1 * torch.randn(10, generator=gen), torch.zeros(10)]
    labels = (torch.rand(5, 10, generator=gen) > 0.5).float()
    labels[0], labels[4] = 0.0, 1.0
    pos_weight = 0.2 + 4.8 * torch.rand(10, generator=gen)
    inp = dict(xs=xs, bufs=[None, None], ws=ws, bs=bs, labels=labels, pos_weight=pos_weight)
    ref = R.heads(xs, ws, bs, case["coef"], labels, True, pos_weight)
    assert float(ref["logits"][0].max()) > 100.0 and float(ref["logits"][0].min()) < -100.0
    got = run_heads(case, inp, dev)
    for t in (got["logits"], got["losses"]) + tuple(h[k] for h in got["heads"] for k in ("d_pooled", "g_w", "g_b")):
        assert bool(torch.isfinite(t).all())
    assert observe("heads bce large logits (rel to max)", rel(got["logits"], ref["logits"]), BAR) < BAR
    for g, r in zip(R.f64(got["losses"]).tolist(), ref["losses"].tolist()):
        assert observe("heads bce large losses (abs / max(1, |loss|))", abs(g - r) / max(1.0, abs(r)), BAR) < BAR
    ok = R.decided(ref)[0]
    assert float((~ok).float().mean()) < R.PRED_EXCLUDED_MAX
    assert torch.equal(got["preds"][0].cpu().long()[ok], ref["preds"][0][ok])
    assert float(got["logits"][1].abs().max()) == 0.0 and int(got["preds"][1].abs().max()) == 0
    check_grads("bce large", got, ref, case)


@pytest.mark.parametrize("bce", [False, True], ids=["ce", "bce"])
def test_losses_accumulate_or_overwrite_and_evaluation_writes_no_gradients(bce, dev):
    case = next(c for c in R.HEAD_CASES if c["name"] == ("bce D128 B5 K31" if bce else "ce D128 B4 K10"))
    inp, ref = R.head_inputs(case)
    kind = "bce" if bce else "ce"
    check_forward(kind, run_heads(case, inp, dev, zero_losses=False, losses_fill=5.0), ref, losses_offset=5.0)     # adds
    check_forward(kind, run_heads(case, inp, dev, zero_losses=True, losses_fill=5.0), ref)                         # overwrites
    got = run_heads(case, inp, dev, training=False)              # d_pooled = NULL: evaluation
    check_forward(kind, got, ref)
    for hd in got["heads"]:
        assert bool((hd["g_w"] == SENT).all()) and bool((hd["g_b"] == SENT).all())


REFUSALS = ["K=1", "K=33", "D=48", "five heads", "tokens unaligned", "stride below ntok*D", "g_part on BCE", "g_part K12 D128", "g_part K23 D64"]


@pytest.mark.parametrize("what", REFUSALS)
def test_refusals_return_minus_one_and_launch_nothing(what, dev):
    """Every unsupported call returns -1 with a message and leaves every output buffer as it was (zero_losses = 1 included: the
    losses' zero fill must not run either)."""
    from m2_mixer_amd import _lib as L
    B, D, K, nh, bce = 8, 128, 10, 1, False
    ntok, stride, tok_off, gp = 0, 0, 0, False
    if what == "K=1": K = 1
    if what == "K=33": K = 33
    if what == "D=48": D = 48
    if what == "five heads": nh = 5
    if what == "tokens unaligned": ntok, stride, tok_off = 4, 4 * D, 1
    if what == "stride below ntok*D": ntok, stride = 4, 4 * D - 4
    if what == "g_part on BCE": gp, bce = True, True
    if what == "g_part K12 D128": gp, K = True, 12
    if what == "g_part K23 D64": gp, K, D = True, 23, 64
    # generous buffers: whatever a wrongly accepted call would touch is inside them
    x = torch.randn(B * 8 * 256 + 8, device=dev)
    w, b = torch.randn(64, 256, device=dev), torch.randn(64, device=dev)
    outs = dict(g_w=torch.full((64, 256), SENT, device=dev), g_b=torch.full((64,), SENT, device=dev),
                d_pooled=torch.full((B, 256), SENT, device=dev), g_part=torch.full((5, 8, L.SPLIT_GPART), SENT, device=dev),
                logits=torch.full((5, B, 64), SENT, device=dev), losses=torch.full((8,), SENT, device=dev),
                preds=torch.full((5, B, 64), -7, dtype=torch.int32, device=dev))
    arr = (L.Head * 5)()
    for h in range(5):
        arr[h].w, arr[h].b, arr[h].g_w, arr[h].g_b, arr[h].d_pooled = w.data_ptr(), b.data_ptr(), outs["g_w"].data_ptr(), outs["g_b"].data_ptr(), outs["d_pooled"].data_ptr()
        arr[h].weight = 1.0
        if ntok:
            arr[h].tokens, arr[h].ntok, arr[h].tok_sample_stride = x.data_ptr() + 4 * tok_off, ntok, stride
        else:
            arr[h].pooled = x.data_ptr()
        if gp:
            arr[h].g_part = outs["g_part"][h].data_ptr()
    st = L.stream_ptr()
    if bce:
        tg, pw = torch.zeros(B, 64, device=dev), torch.ones(64, device=dev)
        rc = L.lib().m2m_heads_bce(arr, nh, tg.data_ptr(), pw.data_ptr(), B, D, K, outs["logits"].data_ptr(), outs["losses"].data_ptr(), outs["preds"].data_ptr(), 1, st)
    else:
        lab = torch.zeros(B, dtype=torch.int64, device=dev)
        rc = L.lib().m2m_heads_ce(arr, nh, lab.data_ptr(), B, D, K, outs["logits"].data_ptr(), outs["losses"].data_ptr(), outs["preds"].data_ptr(), 1, st)
    torch.cuda.synchronize()
    assert rc == -1 and len(L.lib().m2m_last_error()) > 0
    for k, t in outs.items():
        assert bool((t == (-7 if k == "preds" else SENT)).all()), k
