"""float64 restatement of the evidential heads (m2m_heads_edl; the reference's AVMnistMixerMultiLossUQ, models/avmnist.py:447-572,
with EDLMSELoss, modules/losses.py:5-31), in the shape of leaf_ref.heads, the shared case table of tests/test_gpu_edl.py and the
float64 reference of an AVMnistUQEngine step.  Plain torch float64 on the CPU, autograd for the gradients.
tests/test_host_edl.py pins this file against the reference's own EDLMSELoss (tests/golden/edl.npz) and against its closed-form
gradient.

The gate.  A logit within rounding of 0 has a discontinuous gradient (relu), so a reference that picks the other side of the gate
than a kernel did would differ from it by far more than any bar.  `gate` (nheads, B, K) bool -- the dropout-mask technique of the
engine tests -- makes the evidence z * gate instead of relu(z): the GPU tests pass the kernel's own gate (its logits > 0) and
assert separately that it equals the reference's wherever |z_ref| exceeds 10x the logits bar.

Decisions.  A head's prediction is held only where the float64 reference is decided: top1 < -bar (all evidence zero: class 0),
or top1 > bar and top1 - max(top2, 0) > bar, with bar = PRED_MARGIN x FP32_REL x max|logits|.  The combined prediction is decided
when the two smallest uncertainties differ by more than PRED_MARGIN x FP32_REL (or all are exactly equal) and every head is
decided.  At most PRED_EXCLUDED_MAX of a case's decisions may be excluded; that is a condition on the inputs: a case's seed is the
first at which the reference alone stays under the cap."""
import math
from collections import namedtuple

import torch

import leaf_ref as LR
from oracle import m2mixer_oracle as O

f64 = LR.f64


# ---- the loss and its closed-form gradient ------------------------------------------------------------------------------------
def evidence(z, gate=None):
    return torch.relu(z) if gate is None else z * gate.to(z.dtype)


def edl_loss(z, labels, gate=None):
    """mean_i sum_k [(y_k - p_k)^2 + p_k (1 - p_k) / (S + 1)]  (losses.py:24-31; the KL term is times 0, losses.py:20)."""
    a = evidence(z, gate) + 1.0
    S = a.sum(dim=-1, keepdim=True)
    p = a / S
    y = torch.nn.functional.one_hot(labels, z.shape[-1]).to(z.dtype)
    return ((y - p) ** 2 + p * (1 - p) / (S + 1)).sum(dim=-1).mean()


def edl_grad(z, labels, gate=None):
    """d edl_loss / dz in closed form: [gate] (dE + dV) / B."""
    g = (z > 0) if gate is None else gate
    a = evidence(z, gate) + 1.0
    S = a.sum(dim=-1, keepdim=True)
    p = a / S
    y = torch.nn.functional.one_hot(labels, z.shape[-1]).to(z.dtype)
    sp2 = (p * p).sum(dim=-1, keepdim=True)
    dE = (-2 / S) * ((y - p) - ((y - p) * p).sum(dim=-1, keepdim=True))
    dV = (-2 / (S * (S + 1))) * (p - sp2) - (1 - sp2) / (S + 1) ** 2
    return (dE + dV) * g.to(z.dtype) / z.shape[0]


def uncertainty(z, gate=None):
    return z.shape[-1] / (evidence(z, gate) + 1.0).sum(dim=-1)


def combine(preds, u):
    """preds, u (nheads, B): the prediction of the head whose u is strictly below every other head's, else 0 (avmnist.py:533-537)."""
    nh = preds.shape[0]
    out = torch.zeros_like(preds[0])
    for h in range(nh):
        strict = torch.ones_like(u[0], dtype=torch.bool)
        for o in range(nh):
            if o != h:
                strict &= u[h] < u[o]
        out = out + preds[h] * strict.long()
    return out


def decisions(logits):
    """(head decided (nheads, B), combined decided (B)) of float64 logits (nheads, B, K): see the module docstring."""
    bar = LR.PRED_MARGIN * LR.FP32_REL * float(logits.abs().max())
    top = logits.topk(2, dim=2).values
    t1, t2 = top[..., 0], top[..., 1]
    head = (t1 < -bar) | ((t1 > bar) & (t1 - t2.clamp(min=0) > bar))
    u = uncertainty(logits)
    if u.shape[0] == 1:
        return head, head[0].clone()
    us = u.sort(dim=0).values
    apart = ((us[1] - us[0]) > LR.PRED_MARGIN * LR.FP32_REL) | (us[-1] == us[0])
    return head, apart & head.all(dim=0)


def excluded(logits):
    head, comb = decisions(logits)
    return float((~head).float().mean()), float((~comb).float().mean())


def heads(xs, ws, bs, coef, labels, gate=None):
    """The multi-head evidential loss in float64.  xs[h]: (B, D) pooled rows or (B, ntok, D) tokens; ws[h] (K, D), bs[h] (K);
    coef[h]: the head's coefficient in the total; labels (B) int64; gate: None (relu) or (nheads, B, K) bool.  Returns logits
    (nh, B, K), losses (nh + 1), preds (nh, B), uncertainty (nh, B), combined (B), the gradients of the total (lists d_pooled,
    g_w, g_b) and the decision masks of the RELU form of these logits (head_decided (nh, B), combined_decided (B))."""
    pooled, W, Bv, logits, losses = [], [], [], [], []
    labels = labels.cpu()
    for h, (x, w, b) in enumerate(zip(xs, ws, bs)):
        x = f64(x)
        p = (x.mean(dim=1) if x.dim() == 3 else x).clone().requires_grad_(True)
        w, b = f64(w).requires_grad_(True), f64(b).requires_grad_(True)
        lg = O.linear(p, w, b)
        losses.append(edl_loss(lg, labels, None if gate is None else gate[h].cpu()))
        pooled.append(p); W.append(w); Bv.append(b); logits.append(lg)
    total = sum(float(c) * l for c, l in zip(coef, losses))
    total.backward()
    logits = torch.stack([l.detach() for l in logits])
    g = None if gate is None else gate.cpu()
    preds = evidence(logits, g).argmax(dim=2)
    u = uncertainty(logits, g)
    head_ok, comb_ok = decisions(logits)
    return {"logits": logits, "losses": torch.stack([l.detach() for l in losses] + [total.detach()]), "preds": preds,
            "uncertainty": u, "combined": combine(preds, u), "head_decided": head_ok, "combined_decided": comb_ok,
            "d_pooled": [p.grad for p in pooled], "g_w": [w.grad for w in W], "g_b": [b.grad for b in Bv]}


# ---- the leaf cases -------------------------------------------------------------------------------------------------------------
# A covering set, not the product.  Forms as in leaf_ref.HEAD_CASES: "p" (pooled rows) or ("t", ntok, pad): tokens with sample
# stride ntok * D + pad floats.  D over {32, 64, 128, 256}; B over {1, 3, 4, 5, 64, 65, 81} (4 samples per workgroup up to 64,
# 16 above, ragged tiles of both); K over {2, 3, 10, 23, 32}; 1..4 heads; ntok over {1, 7, 9, 25}; slots (gpart: K D + K + 2 <=
# 1472) and atomics; coefficients by value and from device memory; `combined` aliased onto the last preds row and apart.
def _ec(name, B, D, K, forms, coef, **kw):
    return dict(name=name, B=B, D=D, K=K, forms=forms, coef=coef, gpart=kw.pop("gpart", False), dev_weights=kw.pop("dev_weights", False),
                alias=kw.pop("alias", False))


EDL_CASES = [
    _ec("D32 B1 K2 h1", 1, 32, 2, ["p"], [1.0]),
    _ec("D64 B3 K3 h2", 3, 64, 3, ["p", "p"], [0.5, 1.5]),
    _ec("D128 B4 K10 h3 alias", 4, 128, 10, ["p", "p", "p"], [1.0, 1.0, 1.0], alias=True),
    _ec("D256 B5 K23 h4", 5, 256, 23, ["p", "p", "p", "p"], [0.9, 0.6, 1.5, 0.3]),
    _ec("D32 B64 K32 h2 devw alias", 64, 32, 32, ["p", "p"], [1.0, 3.0], dev_weights=True, alias=True),
    _ec("D64 B65 K10 h3 tokens alias", 65, 64, 10, [("t", 1, 0), ("t", 7, 192), "p"], [1.0, 0.5, 2.0], alias=True),
    _ec("D128 B81 K23 h4 tokens devw", 81, 128, 23, [("t", 9, 640), ("t", 25, 0), "p", "p"], [1.0, 0.8, 0.6, 0.4], dev_weights=True),
    _ec("D256 B81 K32 h1", 81, 256, 32, ["p"], [0.7]),
    _ec("D128 B64 K2 h3", 64, 128, 2, ["p", "p", "p"], [1.0, 0.25, 2.0]),
    _ec("gpart D128 B5 K10 h3 alias", 5, 128, 10, ["p", "p", "p"], [1.0, 1.0, 1.0], gpart=True, alias=True),
    _ec("gpart D32 B81 K32 h4 devw", 81, 32, 32, ["p", "p", "p", "p"], [1.0, 0.5, 0.25, 2.0], gpart=True, dev_weights=True),
    _ec("gpart D64 B65 K3 h2 tokens", 65, 64, 3, [("t", 25, 64), "p"], [2.0, 0.5], gpart=True),
]

SEEDS_PER_CASE = 1000


def _draw(case, seed):
    B, D, K = case["B"], case["D"], case["K"]
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    xs, bufs = [], []
    for f in case["forms"]:
        if f == "p":
            xs.append(rn(B, D)); bufs.append(None)
        else:
            _, ntok, pad = f
            buf = rn(B, ntok * D + pad)                              # the pad holds another tower's (random) tokens
            xs.append(buf[:, :ntok * D].reshape(B, ntok, D) * (math.sqrt(ntok) if ntok > 1 else 1.0))
            buf[:, :ntok * D] = xs[-1].reshape(B, ntok * D)          # (token rows scaled so the pooled rows stay ~ N(0, 1))
            bufs.append(buf)
    ws = [rn(K, D) / math.sqrt(D) for _ in case["forms"]]
    bs = [0.1 * rn(K) for _ in case["forms"]]
    labels = torch.randint(0, K, (B,), generator=gen)
    labels[0] = 0
    if B > 1:
        labels[B - 1] = K - 1
    return dict(xs=xs, bufs=bufs, ws=ws, bs=bs, labels=labels, seed=seed)


def _logits64(inp):
    return torch.stack([O.linear(f64(x).mean(dim=1) if x.dim() == 3 else f64(x), f64(w), f64(b))
                        for x, w, b in zip(inp["xs"], inp["ws"], inp["bs"])])


def case_seed(case):
    """The first seed of the case's own range at which the float64 reference ALONE keeps both kinds of decision under the cap."""
    base = SEEDS_PER_CASE * (EDL_CASES.index(case) + 1)
    for seed in range(base, base + SEEDS_PER_CASE):
        if max(excluded(_logits64(_draw(case, seed)))) < LR.PRED_EXCLUDED_MAX:
            return seed
    raise AssertionError(f"no seed keeps the float64 reference of {case['name']} under the exclusion cap")


def edl_inputs(case):
    """The case's inputs (float32 CPU tensors): standard-normal pooled rows, weights ~ N(0, 1 / D), biases ~ 0.1 N(0, 1), labels
    that include 0 and K - 1 where B allows -- logits ~ N(0, 1), about half of them behind the gate."""
    return _draw(case, case_seed(case))


# ---- the engine step ------------------------------------------------------------------------------------------------------------
UQCase = namedtuple("UQCase", "name engine cfg B p expect")


def uq_forward(case, batch, p, drop_p=0.0, masks=None, gates=None):
    """AVMnistMixerMultiLossUQ.shared_step in float64: the oracle's AV-MNIST forward for the three logits (its cross-entropy
    losses are not used), then the evidential losses with coefficients 1, 1, 1.  gates: None or (3, B, K) bool in the engine's
    head order (image, audio, fusion)."""
    image, audio, labels = batch
    o = O.avmnist_forward(image.double(), audio.double(), labels, p, case.cfg, drop_p, masks)
    logits = [o["image_logits"], o["audio_logits"], o["logits"]]
    losses = [edl_loss(z, labels, None if gates is None else gates[h]) for h, z in enumerate(logits)]
    logits = torch.stack(logits)
    g = None if gates is None else gates
    return {"logits": logits, "losses": torch.stack(losses + [losses[0] + losses[1] + losses[2]]), "uncertainty": uncertainty(logits, g)}


class UQStep:
    """engine_ref.Step for the evidential model: autograd through uq_forward, then oracle.adam_step of every parameter."""

    def __init__(self, case, params, lr):
        self.case, self.lr = case, lr
        self.p = {k: v.detach().double().clone() for k, v in params.items()}
        self.t, self.m, self.v = 0, {}, {}

    def forward(self, batch, params=None, gates=None):
        with torch.no_grad():
            return uq_forward(self.case, batch, self.p if params is None else params, gates=gates)

    def step(self, batch, masks=None, gates=None):
        import engine_ref as R
        leaves = {k: v.clone().requires_grad_(True) for k, v in self.p.items()}
        out = uq_forward(self.case, batch, leaves, R.p_effective(self.case.p) if masks is not None else 0.0, masks, gates)
        out["losses"][3].backward()
        self.t += 1
        grads = {}
        for k, leaf in leaves.items():
            g = leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)
            grads[k] = g
            m, v = self.m.get(k, torch.zeros_like(g)), self.v.get(k, torch.zeros_like(g))
            self.p[k], self.m[k], self.v[k] = O.adam_step(self.p[k], g, m, v, self.t, self.lr)
        out = {k: v.detach() for k, v in out.items()}
        out["grads"] = grads
        return out
