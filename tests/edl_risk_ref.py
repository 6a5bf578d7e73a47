"""float64 restatement of the evidential heads with a choice of Bayes risk and the annealed KL term (m2m_heads_edl_risk; the
reference's modules/losses.py: EDLMSELoss :5-31, kl_divergence_loss :33-49 / :52-68, EDLCELoss :71-93), on top of tests/edl_ref.py:
its gate, its decisions, its case conventions and its engine-step reference are imported, not repeated.  Plain torch float64 on
the CPU.  tests/test_host_edl_risk.py pins this file against the reference's own results (tests/golden/edl_risk.npz) and its
closed-form gradients against autograd.

Per sample, e = relu(z) (or z * gate: edl_ref's docstring), a = e + 1, S = sum a, y the label:
    ce    L = psi(S) - psi(a_y)                          dL/dz_j  = [gate_j] (psi1(S) - [j == y] psi1(a_j))
    kl    at = a off the label, 1 on it; St = sum at
          KL = lgamma(St) - lgamma(K) - sum lgamma(at) + sum (at - 1)(psi(at) - psi(St))
                                                         dKL/dz_j = [gate_j][j != y] ((at_j - 1) psi1(at_j) - psi1(St)(St - K))
    head  loss = mean_B(risk) + lambda mean_B(KL),  lambda = kl_weight min(1, epoch / annealing_step)"""
import torch

import edl_ref as E
import leaf_ref as LR
from oracle import m2mixer_oracle as O

f64 = LR.f64
RISKS = ("mse", "ce")


def kl_lambda(kl_weight, epoch, annealing_step=10):
    return float(kl_weight) * min(1.0, epoch / annealing_step)


def _one_hot(labels, z):
    return torch.nn.functional.one_hot(labels, z.shape[-1]).to(z.dtype)


def ce_loss(z, labels, gate=None):
    a = E.evidence(z, gate) + 1.0
    y = _one_hot(labels, z)
    return (y * (torch.digamma(a.sum(dim=-1))[:, None] - torch.digamma(a))).sum(dim=-1).mean()


def ce_grad(z, labels, gate=None):
    g = (z > 0) if gate is None else gate
    a = E.evidence(z, gate) + 1.0
    y = _one_hot(labels, z)
    return (torch.polygamma(1, a.sum(dim=-1))[:, None] - y * torch.polygamma(1, a)) * g.to(z.dtype) / z.shape[0]


def kl_loss(z, labels, gate=None):
    a = E.evidence(z, gate) + 1.0
    y = _one_hot(labels, z)
    at = y + (1 - y) * a
    st = at.sum(dim=-1)
    first = torch.lgamma(st) - torch.lgamma(at.new_tensor(float(z.shape[-1]))) - torch.lgamma(at).sum(dim=-1)
    second = ((at - 1) * (torch.digamma(at) - torch.digamma(st)[:, None])).sum(dim=-1)
    return (first + second).mean()


def kl_grad(z, labels, gate=None):
    g = (z > 0) if gate is None else gate
    a = E.evidence(z, gate) + 1.0
    y = _one_hot(labels, z)
    at = y + (1 - y) * a
    st = at.sum(dim=-1, keepdim=True)
    d = (at - 1) * torch.polygamma(1, at) - torch.polygamma(1, st) * (st - z.shape[-1])
    return d * (1 - y) * g.to(z.dtype) / z.shape[0]


def risk_loss(risk, z, labels, gate=None):
    return {"mse": E.edl_loss, "ce": ce_loss}[risk](z, labels, gate)


def risk_grad(risk, z, labels, gate=None):
    return {"mse": E.edl_grad, "ce": ce_grad}[risk](z, labels, gate)


def head_loss(z, labels, risk="mse", lam=None, gate=None):
    """(loss, unscaled KL or None) of one head; lam None: no KL term at all."""
    loss = risk_loss(risk, z, labels, gate)
    if lam is None:
        return loss, None
    kl = kl_loss(z, labels, gate)
    return loss + lam * kl, kl


def heads(xs, ws, bs, coef, labels, risk="mse", lam=None, gate=None):
    """edl_ref.heads with the loss of head_loss; adds `kl` (nh): the heads' unscaled batch-mean KL (zeros without the term)."""
    pooled, W, Bv, logits, losses, kls = [], [], [], [], [], []
    labels = labels.cpu()
    for h, (x, w, b) in enumerate(zip(xs, ws, bs)):
        x = f64(x)
        p = (x.mean(dim=1) if x.dim() == 3 else x).clone().requires_grad_(True)
        w, b = f64(w).requires_grad_(True), f64(b).requires_grad_(True)
        lg = O.linear(p, w, b)
        loss, kl = head_loss(lg, labels, risk, lam, None if gate is None else gate[h].cpu())
        losses.append(loss)
        kls.append(torch.zeros((), dtype=torch.float64) if kl is None else kl.detach())
        pooled.append(p); W.append(w); Bv.append(b); logits.append(lg)
    total = sum(float(c) * l for c, l in zip(coef, losses))
    total.backward()
    logits = torch.stack([l.detach() for l in logits])
    g = None if gate is None else gate.cpu()
    preds = E.evidence(logits, g).argmax(dim=2)
    u = E.uncertainty(logits, g)
    head_ok, comb_ok = E.decisions(logits)
    return {"logits": logits, "losses": torch.stack([l.detach() for l in losses] + [total.detach()]), "kl": torch.stack(kls),
            "preds": preds, "uncertainty": u, "combined": E.combine(preds, u), "head_decided": head_ok, "combined_decided": comb_ok,
            "d_pooled": [p.grad for p in pooled], "g_w": [w.grad for w in W], "g_b": [b.grad for b in Bv]}


# ---- the leaf cases of tests/test_gpu_edl_risk.py (edl_ref's case dicts; its _draw gives the inputs) -------------------------------
def _rc(name, B, D, K, forms, coef, **kw):
    c = E._ec(name, B, D, K, forms, coef, **{k: v for k, v in kw.items() if k != "scale"})
    c["scale"] = kw.get("scale", 1.0)
    return c


# The four shapes of the issue; a covering set of forms over them, not the product: slots (K D + K + 2 <= 1472 holds for the
# first two shapes only) and atomics, coefficients by value and from device memory, `combined` aliased and apart, and the scale-50
# inputs (logits ~ 50 N(0, 1): psi, psi1 and lgamma past x = 6) on a slot case and on the many-tile atomic case.
RISK_CASES = [
    _rc("D32 B1 K2", 1, 32, 2, ["p"], [1.0], gpart=True),                                      # one sample of a 4-sample tile, 30 dead lanes
    _rc("D64 B5 K10 tokens", 5, 64, 10, [("t", 3, 0)], [0.7], dev_weights=True, gpart=True),   # one head from tokens, ntok = 3
    _rc("D128 B65 K32", 65, 128, 32, ["p", "p"], [1.0, 0.5]),                                  # 16-sample tiles + a one-row tile, no dead lane
    _rc("D256 B9 K23", 9, 256, 23, ["p", "p"], [1.0, 2.0], dev_weights=True, alias=True),
    _rc("D64 B5 K10 tokens scale50", 5, 64, 10, [("t", 3, 0)], [0.7], gpart=True, scale=50.0),
    _rc("D128 B65 K32 scale50", 65, 128, 32, ["p", "p"], [1.0, 0.5], dev_weights=True, scale=50.0),
]
SEED_BASE = 500000


def _scaled(case, seed):
    inp = E._draw(case, seed)
    s = case["scale"]
    if s != 1.0:                                 # logits ~ scale x N(0, 1): the weights and biases carry the scale
        inp["ws"] = [w * s for w in inp["ws"]]
        inp["bs"] = [b * s for b in inp["bs"]]
    return inp


def risk_inputs(case):
    """The case's inputs at the first seed of its own range at which the float64 reference ALONE keeps both kinds of decision
    under edl_ref's exclusion cap."""
    base = SEED_BASE + E.SEEDS_PER_CASE * RISK_CASES.index(case)
    for seed in range(base, base + E.SEEDS_PER_CASE):
        inp = _scaled(case, seed)
        if max(E.excluded(E._logits64(inp))) < LR.PRED_EXCLUDED_MAX:
            return inp
    raise AssertionError(f"no seed keeps the float64 reference of {case['name']} under the exclusion cap")


# ---- the engine step ------------------------------------------------------------------------------------------------------------
def uq_forward(case, batch, p, drop_p=0.0, masks=None, gates=None, risk="mse", lam=None):
    """edl_ref.uq_forward under head_loss; adds `kl` (3)."""
    image, audio, labels = batch
    o = O.avmnist_forward(image.double(), audio.double(), labels, p, case.cfg, drop_p, masks)
    logits = [o["image_logits"], o["audio_logits"], o["logits"]]
    pairs = [head_loss(z, labels, risk, lam, None if gates is None else gates[h]) for h, z in enumerate(logits)]
    losses = [l for l, _ in pairs]
    logits = torch.stack(logits)
    kl = torch.stack([torch.zeros((), dtype=torch.float64) if k is None else k.detach() for _, k in pairs])
    return {"logits": logits, "losses": torch.stack(losses + [losses[0] + losses[1] + losses[2]]), "kl": kl,
            "uncertainty": E.uncertainty(logits, gates)}


class UQStep(E.UQStep):
    """edl_ref.UQStep with the risk and lambda of the step (lam is an attribute: the test moves it with the epoch)."""

    def __init__(self, case, params, lr, risk="mse", lam=None):
        super().__init__(case, params, lr)
        self.risk, self.lam = risk, lam

    def forward(self, batch, params=None, gates=None):
        with torch.no_grad():
            return uq_forward(self.case, batch, self.p if params is None else params, gates=gates, risk=self.risk, lam=self.lam)

    def step(self, batch, masks=None, gates=None):
        import engine_ref as R
        leaves = {k: v.clone().requires_grad_(True) for k, v in self.p.items()}
        out = uq_forward(self.case, batch, leaves, R.p_effective(self.case.p) if masks is not None else 0.0, masks, gates,
                         risk=self.risk, lam=self.lam)
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
