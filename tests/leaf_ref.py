"""float64 restatements of the leaf kernels around the towers -- the classification heads, Adam, GELU -- and the shared
case tables of tests/test_gpu_heads.py / test_gpu_adam.py / test_gpu_probes.py.  Plain torch float64 on the CPU, autograd for
the gradients, the oracle's own functions where they fit.  tests/test_host_leaf_ref.py pins this file against
torch.nn.functional, torch.optim.Adam and scipy.special.erf, so a GPU test that disagrees with it disagrees with those."""
import math

import torch

from oracle import m2mixer_oracle as O

FP32_REL = 1e-4            # the project's fp32 bar, relative to the tensor's max (tests/test_gpu_shape_envelope.py)
PRED_MARGIN = 10.0         # predictions are compared where the float64 decision margin exceeds PRED_MARGIN x the logits bar
PRED_EXCLUDED_MAX = 0.01   # and fewer than 1 % of a case's decisions may be excluded that way


def f64(t):
    return t.detach().cpu().double()


# ---- GELU -------------------------------------------------------------------------------------------------------------------
def gelu(x):
    """0.5 x (1 + erf(x / sqrt 2)) in float64 (the oracle's formula)."""
    return O.gelu(x.double())


def gelu_grad(x):
    """d gelu / dx = Phi(x) + x phi(x) in float64."""
    x = x.double()
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


# ---- Adam -------------------------------------------------------------------------------------------------------------------
def adam(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0):
    """One torch.optim.Adam update in float64 on the gradient |grad_scale| * g: returns (param, exp_avg, exp_avg_sq)."""
    return O.adam_step(p.double(), g.double() * abs(grad_scale), m.double(), v.double(), step, lr, betas[0], betas[1], eps, weight_decay)


def adam_torch(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0, dtype=torch.float32):
    """The same update by torch.optim.Adam itself on CPU tensors of `dtype` (float32: the error a careful fp32 Adam has against
    float64 on the same inputs -- the yardstick of the GPU test's bars).  `step` is 1-based: the state enters at step - 1."""
    q = torch.nn.Parameter(p.detach().cpu().to(dtype).clone())
    opt = torch.optim.Adam([q], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, foreach=False, fused=False)
    opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.detach().cpu().to(dtype).clone(),
                    "exp_avg_sq": v.detach().cpu().to(dtype).clone()}
    q.grad = g.detach().cpu().to(dtype) * abs(grad_scale)
    opt.step()
    st = opt.state[q]
    return q.detach(), st["exp_avg"], st["exp_avg_sq"]


# ---- heads ------------------------------------------------------------------------------------------------------------------
def heads(xs, ws, bs, coef, labels, bce=False, pos_weight=None):
    """The multi-head loss in float64.  xs[h]: (B, D) pooled rows, or (B, ntok, D) tokens the reference pools itself
    (x.mean(dim=1)); ws[h] (K, D), bs[h] (K); coef[h]: the head's coefficient in the total.  labels: (B) int64 class indices, or
    with bce (B, K) multi-hot targets and pos_weight (K).  Returns logits (nh, B, K), losses (nh + 1: per head, then the weighted
    total), d_pooled / g_w / g_b (lists: the gradients of the total), and the float64 decision margins (see `decided`)."""
    pooled, W, Bv, logits, losses = [], [], [], [], []
    for x, w, b in zip(xs, ws, bs):
        x = f64(x)
        p = (x.mean(dim=1) if x.dim() == 3 else x).clone().requires_grad_(True)
        w, b = f64(w).requires_grad_(True), f64(b).requires_grad_(True)
        lg = O.linear(p, w, b)
        losses.append(O.bce_with_logits(lg, f64(labels), f64(pos_weight)) if bce else O.cross_entropy(lg, labels.cpu()))
        pooled.append(p); W.append(w); Bv.append(b); logits.append(lg)
    total = sum(float(c) * l for c, l in zip(coef, losses))
    total.backward()
    logits = torch.stack([l.detach() for l in logits])
    if bce:
        margin = logits.abs()                                   # distance of each label's logit from the decision point 0
        preds = (logits > 0).long()
    else:
        top2 = logits.topk(2, dim=2).values
        margin = top2[..., 0] - top2[..., 1]
        preds = logits.argmax(dim=2)
    return {"logits": logits, "losses": torch.stack([l.detach() for l in losses] + [total.detach()]), "preds": preds,
            "margin": margin, "d_pooled": [p.grad for p in pooled], "g_w": [w.grad for w in W], "g_b": [b.grad for b in Bv]}


def decided(ref):
    """Mask of the decisions (samples; BCE: labels) a prediction is held to: float64 margin above PRED_MARGIN x the logits bar."""
    return ref["margin"] > PRED_MARGIN * FP32_REL * float(ref["logits"].abs().max())


# A covering set, not the product.  Per case: B, D, K, the heads' input forms and coefficients.  A form is "p" (pooled rows) or
# ("t", ntok, pad): tokens, sample stride ntok * D + pad floats (pad > 0: another tower's tokens interleaved, as ConcatFusion
# lays them out).  Workgroup shapes: 4 samples per workgroup at B <= 64, 16 above; every D with both; K over {2, 3, 10, 23, 31, 32};
# B over {1, 3, 4, 5, 64, 65, 81}; ntok over {1, 7, 8, 9, 25}.
def _hc(name, B, D, K, forms, coef, **kw):
    return dict(name=name, B=B, D=D, K=K, forms=forms, coef=coef, bce=kw.pop("bce", False), gpart=kw.pop("gpart", False),
                dev_weights=kw.pop("dev_weights", False), seed=kw.pop("seed", 0))


HEAD_CASES = [
    _hc("ce D32 B1 K2", 1, 32, 2, ["p"], [1.0]),
    _hc("ce D64 B3 K3", 3, 64, 3, ["p", "p"], [0.5, 1.5]),
    _hc("ce D128 B4 K10", 4, 128, 10, ["p", "p", "p"], [1.0, 0.25, 2.0]),
    _hc("ce D256 B5 K23", 5, 256, 23, ["p", "p", "p", "p"], [0.9, 0.6, 1.5, 0.3]),
    _hc("ce D32 B64 K31", 64, 32, 31, ["p", "p"], [1.0, 3.0]),
    _hc("ce D64 B65 K32", 65, 64, 32, ["p"], [0.7]),
    _hc("ce D128 B81 K32 devw", 81, 128, 32, ["p", "p", "p"], [1.0, 1.0, 0.4], dev_weights=True),
    _hc("ce D256 B65 K10", 65, 256, 10, ["p", "p"], [2.0, 0.5]),
    _hc("ce D32 B81 K23", 81, 32, 23, ["p", "p", "p", "p"], [0.1, 0.2, 0.3, 0.4]),
    _hc("ce D64 B5 K10 tokens", 5, 64, 10, [("t", 1, 0), ("t", 7, 192), "p"], [1.0, 0.5, 2.0]),
    _hc("ce D128 B65 K23 tokens", 65, 128, 23, [("t", 8, 0), ("t", 9, 640), ("t", 25, 0), "p"], [1.0, 0.8, 0.6, 0.4]),
    _hc("ce D256 B4 K3 tokens", 4, 256, 3, [("t", 25, 256)], [1.0]),
    _hc("ce D32 B64 K31 tokens", 64, 32, 31, ["p", ("t", 9, 32)], [1.0, 1.0]),
    _hc("ce gpart K10 D128 B5", 5, 128, 10, ["p", "p", "p"], [1.0, 0.5, 1.5], gpart=True),
    _hc("ce gpart K11 D128 B81", 81, 128, 11, ["p", ("t", 7, 0)], [1.0, 0.5], gpart=True),
    _hc("ce gpart K22 D64 B65", 65, 64, 22, ["p"], [2.0], gpart=True),
    _hc("ce gpart K32 D32 B64", 64, 32, 32, ["p", "p", "p", "p"], [1.0, 0.5, 0.25, 2.0], gpart=True),
    _hc("bce D32 B1 K2", 1, 32, 2, ["p"], [1.0], bce=True),
    _hc("bce D64 B65 K23 devw", 65, 64, 23, ["p", "p", "p"], [1.0, 1.0, 1.0], bce=True, dev_weights=True),
    _hc("bce D128 B5 K31", 5, 128, 31, ["p", "p"], [0.5, 2.0], bce=True),
    _hc("bce D256 B81 K32", 81, 256, 32, ["p", "p", "p", "p"], [1.0, 0.3, 0.6, 1.2], bce=True),
    _hc("bce D128 B64 K3", 64, 128, 3, ["p"], [1.5], bce=True),
    _hc("bce D256 B3 K10 tokens", 3, 256, 10, [("t", 9, 0), "p", ("t", 8, 512)], [1.0, 0.5, 0.25], bce=True),
    _hc("bce D32 B81 K10 tokens", 81, 32, 10, [("t", 25, 64), ("t", 1, 0)], [1.0, 2.0], bce=True),
    _hc("bce D64 B4 K32", 4, 64, 32, ["p", "p"], [1.0, 1.0], bce=True),
]


def head_inputs(case):
    """The case's inputs (float32 CPU tensors), deterministic: standard-normal rows, weights ~ N(0, 1 / D), biases ~ 0.1 N(0, 1),
    labels that include 0 and K - 1 where B allows, BCE targets with an all-zero and an all-one row where B allows, pos_weight
    from [0.2, 5].  The generator seed is the first from the case's own on at which the float64 reference ALONE holds fewer than
    PRED_EXCLUDED_MAX of its decisions inside the exclusion margin (a property of the inputs, never of a kernel)."""
    B, D, K = case["B"], case["D"], case["K"]
    for seed in range(1000 * (HEAD_CASES.index(case) + 1) + case["seed"], 1000 * (HEAD_CASES.index(case) + 2)):
        gen = torch.Generator().manual_seed(seed)
        rn = lambda *s: torch.randn(*s, generator=gen)
        xs, bufs = [], []
        for f in case["forms"]:
            if f == "p":
                xs.append(rn(B, D)); bufs.append(None)
            else:
                _, ntok, pad = f
                stride = ntok * D + pad
                buf = rn(B, stride)                                  # the pad holds another tower's (random) tokens
                bufs.append(buf)
                xs.append(buf[:, :ntok * D].reshape(B, ntok, D) * (math.sqrt(ntok) if ntok > 1 else 1.0))
                buf[:, :ntok * D] = xs[-1].reshape(B, ntok * D)      # (token rows scaled so the pooled rows stay ~ N(0, 1))
        ws = [rn(K, D) / math.sqrt(D) for _ in case["forms"]]
        bs = [0.1 * rn(K) for _ in case["forms"]]
        if case["bce"]:
            labels = (torch.rand(B, K, generator=gen) > 0.7).float()
            labels[0] = 0.0
            if B > 1:
                labels[B - 1] = 1.0
            pos_weight = 0.2 + 4.8 * torch.rand(K, generator=gen)
        else:
            labels = torch.randint(0, K, (B,), generator=gen)
            labels[0] = 0
            if B > 1:
                labels[B - 1] = K - 1
            pos_weight = None
        inp = dict(xs=xs, bufs=bufs, ws=ws, bs=bs, labels=labels, pos_weight=pos_weight, seed=seed)
        ref = heads(xs, ws, bs, case["coef"], labels, case["bce"], pos_weight)
        if float((~decided(ref)).float().mean()) < PRED_EXCLUDED_MAX:
            return inp, ref
    raise AssertionError(f"no seed keeps the float64 reference of {case['name']} under the exclusion cap")
