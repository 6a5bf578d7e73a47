"""Pins tests/leaf_ref.py -- the float64 reference the GPU tests of the heads, Adam and GELU compare with -- against
torch.nn.functional, torch.optim.Adam and scipy.special.erf on the CPU."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import leaf_ref as R


def _close(a, b, tol=1e-12):
    a, b = a.double(), b.double()
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("case", [c for c in R.HEAD_CASES if not c["bce"]][:6] + [c for c in R.HEAD_CASES if c["bce"]][:4],
                         ids=lambda c: c["name"])
def test_heads_reference_is_torch_functional_in_float64(case):
    inp, ref = R.head_inputs(case)
    leaves, total = [], 0.0
    for h, (x, w, b) in enumerate(zip(inp["xs"], inp["ws"], inp["bs"])):
        x, w, b = (t.double().requires_grad_(True) for t in (x, w, b))
        p = x.mean(dim=1) if x.dim() == 3 else x
        p.retain_grad()
        lg = F.linear(p, w, b)
        if case["bce"]:
            loss = F.binary_cross_entropy_with_logits(lg, inp["labels"].double(), pos_weight=inp["pos_weight"].double())
        else:
            loss = F.cross_entropy(lg, inp["labels"])
        assert _close(ref["logits"][h], lg.detach()) and _close(ref["losses"][h], loss.detach())
        total = total + case["coef"][h] * loss
        leaves.append((p, w, b))
    total.backward()
    assert _close(ref["losses"][-1], total.detach())
    for h, (p, w, b) in enumerate(leaves):
        assert _close(ref["d_pooled"][h], p.grad) and _close(ref["g_w"][h], w.grad) and _close(ref["g_b"][h], b.grad)


@pytest.mark.parametrize("case", R.HEAD_CASES, ids=lambda c: c["name"])
def test_head_case_inputs_keep_the_reference_decisions_clear(case):
    """Standard-normal pooled rows, weights ~ N(0, 1 / D): fewer than 1 % of the float64 reference's own decisions lie inside
    the margin the GPU test excludes from the exact comparison of predictions; labels / targets hold the edge rows."""
    inp, ref = R.head_inputs(case)
    assert float((~R.decided(ref)).float().mean()) < R.PRED_EXCLUDED_MAX
    if case["bce"]:
        assert float(inp["labels"][0].sum()) == 0 and (case["B"] == 1 or float(inp["labels"][-1].min()) == 1)
        assert 0.2 <= float(inp["pos_weight"].min()) and float(inp["pos_weight"].max()) <= 5.0
    else:
        assert int(inp["labels"][0]) == 0 and (case["B"] == 1 or int(inp["labels"][-1]) == case["K"] - 1)
    for x, f in zip(inp["xs"], case["forms"]):
        assert x.dim() == (2 if f == "p" else 3)
        pooled = x.mean(dim=1) if x.dim() == 3 else x
        assert 0.5 < float(pooled.std()) < 1.5 or pooled.numel() < 256


@pytest.mark.parametrize("hp", [dict(), dict(betas=(0.8, 0.95), eps=1e-3, weight_decay=1e-2, grad_scale=0.5)], ids=["defaults", "wd"])
@pytest.mark.parametrize("step", [1, 3, 1000])
def test_adam_reference_is_torch_optim_adam_in_float64(step, hp):
    gen = torch.Generator().manual_seed(5)
    n = 1025
    p, g = torch.randn(n, generator=gen).double(), torch.randn(n, generator=gen).double() * 0.1
    m = torch.randn(n, generator=gen).double() * 0.01 if step > 1 else torch.zeros(n).double()
    v = torch.rand(n, generator=gen).double() * 1e-3 if step > 1 else torch.zeros(n).double()
    got = R.adam(p, g, m, v, step, 1e-2, **hp)
    want = R.adam_torch(p, g, m, v, step, 1e-2, dtype=torch.float64, **hp)
    for a, b in zip(got, want):
        assert _close(a, b, 1e-13)
    assert not torch.equal(got[0], p)
    # the float32 yardstick is float32 torch, close to but not equal to float64
    w32 = R.adam_torch(p, g, m, v, step, 1e-2, dtype=torch.float32, **hp)
    assert w32[0].dtype == torch.float32 and 0 < float((w32[2].double() - got[2]).abs().max()) < 1e-6 * float(got[2].abs().max())


def test_gelu_reference_is_scipy_erf():
    from scipy import special
    x = np.concatenate([np.linspace(-8.0, 8.0, 200001), [0.0, -0.0, 1e-20, -1e-20, 40.0, -40.0]])
    t = torch.from_numpy(x)
    cdf = 0.5 * (1.0 + special.erf(x / math.sqrt(2.0)))
    assert np.abs(R.gelu(t).numpy() - x * cdf).max() < 1e-15
    assert np.abs(R.gelu_grad(t).numpy() - (cdf + x * np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi))).max() < 1e-15
    h = 1e-6                                                     # and gelu_grad is the derivative of gelu
    num = (R.gelu(t + h) - R.gelu(t - h)) / (2 * h)
    assert float((num - R.gelu_grad(t)).abs().max()) < 1e-8
