"""Reference side of the value envelope (tests/value_cases.py): the float64 oracle on a case's transformed tensors, what the case
reaches there (reach), its conditioning (bf16_twin, the oracle in float32), oracle variants that stand for a subtly wrong kernel
(MUTANTS), and the one comparison both the host test and the GPU test apply (compare).

bf16_twin is the oracle with both operands of every `linear` rounded to bf16 (straight-through for autograd) and float64
accumulation.  It measures how far bf16 operands alone move a case's results; it is not a model of the kernels and is never
compared with them.
"""
import contextlib
import math

import numpy as np
import torch

import drop_ref as DR
import gen_util as G
import value_cases as VC
from oracle import m2mixer_oracle as O
from test_gpu_shape_envelope import (BF16_GRAD_REL, BF16_REL, FP32_REL, case_shapes, make_input, oracle, rel, tail_of,
                                     tensor_class)

PARAM_SEED = 4242            # run_case's seeds: the host side regenerates what the device side is given
INPUT_SEED = 977
CELL = 12.0 / 512            # one cell of the GELU table
BARS = {"fp32": dict(act=FP32_REL, grad=FP32_REL), "bf16": dict(act=BF16_REL, grad=BF16_GRAD_REL)}


def inputs(vc, seed=0):
    """(params, x, dy) of a case, float32: run_case's tensors under the case's regime."""
    params = G.make_params(case_shapes(vc.case), PARAM_SEED + seed)
    rng = np.random.default_rng(INPUT_SEED + seed)
    x = make_input(vc.case, rng)
    dy = torch.from_numpy(rng.standard_normal(tuple(x.shape)).astype(np.float32))
    params, x = VC.transform(vc.regime)(params, x)
    return params, x, dy


def host_masks(vc, seed=1, step=1, site_base=0):
    """Keep-masks of a dropout case from the host replica of the kernels' stream (tests/drop_ref.py), in the oracle's layout."""
    c = vc.case
    if c.p == 0:
        return None
    Cp = (c.C + 31) // 32 * 32
    out = []
    for b in range(c.nb):
        m = lambda site, *shape: torch.from_numpy(
            DR.tower_mask(seed, step, site_base, b, site, c.p, c.B, c.N, c.D, c.T, Cp).astype(np.float64)).view(*shape)
        out.append({"tok_h": m(0, c.B, c.D, c.T), "tok_o": m(1, c.B, c.D, c.N), "ch_h": m(2, c.B, c.N, Cp)[:, :, :c.C],
                    "ch_o": m(3, c.B, c.N, c.D)})
    return out


@contextlib.contextmanager
def patched(**fns):
    """The oracle with some of its primitives replaced (its functions look them up in the module at call time)."""
    old = {k: getattr(O, k) for k in fns}
    try:
        for k, f in fns.items():
            setattr(O, k, f)
        yield
    finally:
        for k, f in old.items():
            setattr(O, k, f)


def run(vc, params, x, dy, dtype=torch.float64, masks=None, training=True, **patches):
    """{'out', 'dx', every parameter key}: the oracle's output and gradients under upstream gradient dy."""
    leaves = {k: v.to(dtype).requires_grad_(True) for k, v in params.items()}
    xr = x.to(dtype).requires_grad_(True)
    drop_p = DR.p_effective(vc.case.p) if (vc.case.p > 0 and training) else 0.0
    if masks is not None:
        masks = [{k: v.to(dtype) for k, v in m.items()} for m in masks]
    with patched(**patches):
        y = oracle(vc.case, xr, leaves, drop_p, masks if drop_p > 0 else None)
        (y * dy.to(dtype)).sum().backward()
    out = {"out": y.detach().double(), "dx": xr.grad.double()}
    out.update({k: v.grad.double() for k, v in leaves.items()})
    return out


def reference(vc, masks=None):
    params, x, dy = inputs(vc)
    return run(vc, params, x, dy, masks=masks if masks is not None else host_masks(vc))


ENGINE_CASES = ("av_grouped_n2_n4_d64_half", "av_grouped_n1_n3_d128_gen")     # of tests/engine_cases.py
ENGINE_PARAM_SEED = 31
ENGINE_TOWERS = ("image_mixer.", "audio_mixer.", "fusion_mixer.")


def engine_params(case):
    """A case of tests/engine_cases.py with `trained` towers: gamma, beta and the tails on every tower (the first block of each),
    the patch embeddings and the heads at initialisation scale."""
    import engine_ref as R
    return VC.transform_towers("trained", G.make_params(R.case_shapes(case), ENGINE_PARAM_SEED), ENGINE_TOWERS)


# ---- what a case reaches ----------------------------------------------------------------------------------------------------
def reach(vc):
    """Per block, from the float64 oracle: shares of the token- and channel-mixing hidden pre-activations below -6 and at or
    above 6, the nearest distance of one to each of -6 and +6, and min over rows of |mean| / std, min |mean| and min / max variance
    of the rows entering the block's first LayerNorm."""
    params, x, _ = inputs(vc)
    lin, lns = [], []
    lin0, ln0 = O.linear, O.layer_norm

    def linear(a, w, b):
        y = lin0(a, w, b)
        lin.append(y.detach())
        return y

    def layer_norm(a, w, b, eps=O.LN_EPS):
        lns.append(a.detach())
        return ln0(a, w, b, eps)

    with torch.no_grad(), patched(linear=linear, layer_norm=layer_norm):
        oracle(vc.case, x.double(), {k: v.double() for k, v in params.items()}, DR.p_effective(vc.case.p) if vc.case.p else 0.0,
               host_masks(vc))
    out = []
    for b in range(vc.case.nb):
        tok_h, _, ch_h, _ = lin[4 * b:4 * b + 4]
        rows = lns[2 * b]
        mu, sd = rows.mean(-1), rows.var(-1, unbiased=False).sqrt()
        d = {"ratio": float((mu.abs() / sd.clamp_min(1e-300)).min()), "mean": float(mu.abs().min()),
             "var_min": float(sd.min()) ** 2, "var_max": float(sd.max()) ** 2,
             "var_of_sample": [float(sd[s].max()) ** 2 for s in range(rows.shape[0])]}
        for name, h in (("tok", tok_h), ("ch", ch_h)):
            d[name + "_lo"] = float((h < -6).double().mean())
            d[name + "_hi"] = float((h >= 6).double().mean())
            d[name + "_near_lo"] = float((h + 6).abs().min())
            d[name + "_near_hi"] = float((h - 6).abs().min())
        out.append(d)
    return out


# ---- conditioning -----------------------------------------------------------------------------------------------------------
def _bf(t):
    return t.float().to(torch.bfloat16).to(t.dtype)


def _linear_bf16(x, w, b):
    xr = x + (_bf(x.detach()) - x.detach())
    wr = w + (_bf(w.detach()) - w.detach())
    y = xr @ wr.t()
    return y if b is None else y + b


def bf16_twin(vc):
    params, x, dy = inputs(vc)
    return run(vc, params, x, dy, masks=host_masks(vc), linear=_linear_bf16)


def float32_oracle(vc):
    params, x, dy = inputs(vc)
    return run(vc, params, x, dy, dtype=torch.float32, masks=host_masks(vc))


# ---- oracle variants that stand for a subtly wrong kernel -----------------------------------------------------------------------
def _gelu_wrong_outer_cells(x):
    """0 below -6 (right to 1e-8), slope 0.9 instead of 1 at and above +6."""
    return torch.where(x >= 6, 0.9 * x, torch.where(x < -6, torch.zeros_like(x), _GELU(x)))


def _gelu_zero_slope_above_6(x):
    """The value is right, the derivative at and above +6 is 0."""
    return torch.where(x >= 6, x.detach(), _GELU(x))


def _ln_one_pass_float32(x, weight, bias, eps=O.LN_EPS):
    """Variance as E[x^2] - mean^2, accumulated in float32."""
    x32 = x.float()
    mu = x32.mean(dim=-1, keepdim=True)
    var = ((x32 * x32).mean(dim=-1, keepdim=True) - mu * mu).clamp_min(0.0)
    return (x - mu.to(x.dtype)) * torch.rsqrt(var.to(x.dtype) + eps) * weight + bias


def _ln_rstd_off_at_small_variance(x, weight, bias, eps=O.LN_EPS):
    """rstd 1e-3 (relative) too large where the variance is below 1e-4."""
    mu = x.mean(dim=-1, keepdim=True)
    xc = x - mu
    var = (xc * xc).mean(dim=-1, keepdim=True)
    rstd = torch.rsqrt(var + eps) * torch.where(var.detach() < 1e-4, 1.0 + 1e-3, 1.0)
    return xc * rstd * weight + bias


_GELU = O.gelu
# name -> (oracle primitive it replaces, replacement, the precision whose bars it has to miss, the regimes whose every case has to
# see it)
# The table mutants stand for a bf16 kernel (only bf16 launches read the table) and are held to the bf16 bars; the statistics
# code is shared by both precisions, an error of its size is far below bf16 resolution, and fp32 mode is where it has to show.
MUTANTS = {
    "gelu outer cells: 0 / slope 0.9": ("gelu", _gelu_wrong_outer_cells, "bf16", ("gelu_tails",)),
    "gelu' = 0 above +6": ("gelu", _gelu_zero_slope_above_6, "bf16", ("gelu_tails",)),
    "one-pass variance in float32": ("layer_norm", _ln_one_pass_float32, "fp32", ("ln_offset",)),
    "rstd off by 1e-3 at variance < 1e-4": ("layer_norm", _ln_rstd_off_at_small_variance, "fp32",
                                            ("ln_constant_zero", "ln_constant_three")),
}


def mutant(vc, name):
    params, x, dy = inputs(vc)
    prim, fn, _, _ = MUTANTS[name]
    return run(vc, params, x, dy, masks=host_masks(vc), **{prim: fn})


# ---- the comparison -----------------------------------------------------------------------------------------------------------
def zero_gradient_floor(key, ref):
    """The existing exemption (tests/test_gpu_shape_envelope.py): under a final LayerNorm the token-mixing output bias has a true
    gradient of exactly zero and is measured against its weight's gradient scale."""
    if not key.endswith("token_mix.2.net.3.bias"):
        return 0.0
    floor = float(ref[key[:-4] + "weight"].abs().max())
    return 0.0 if float(ref[key].abs().max()) > 1e-6 * floor else floor


def compare(vc, got, ref, acts=("out", "dx"), slices=True):
    """Yields (kind, what, error, 'act' | 'grad') for everything the envelope holds a result to: the output, dx and every
    parameter gradient over the whole tensor and over the shape envelope's tails, all relative to the float64 reference's
    maximum over the same slice; for outlier_channels the output and dx also per channel class -- the two outlier
    channels and the rest -- since relative to the whole tensor's maximum the ordinary channels are invisible."""
    for what in acts:
        g, r = got[what], ref[what]
        yield f"{what} (rel to max)", what, rel(g, r), "act"
        if not slices:
            continue
        yield f"{what} tail (rel to slice max)", f"{what}[last sample]", rel(g[-1], r[-1]), "act"
        yield f"{what} tail (rel to slice max)", f"{what}[:, last token]", rel(g[:, -1], r[:, -1]), "act"
        if vc.regime == "outlier_channels":
            hot = list(VC.outlier_index(r.shape[-1]))
            cold = [c for c in range(r.shape[-1]) if c not in hot]
            yield f"{what} outlier channels (rel to slice max)", f"{what}[..., outliers]", rel(g[..., hot], r[..., hot]), "act"
            yield f"{what} ordinary channels (rel to slice max)", f"{what}[..., others]", rel(g[..., cold], r[..., cold]), "act"
    for k in ref:
        if k in ("out", "dx") or k not in got:
            continue
        floor = zero_gradient_floor(k, ref)
        cls = tensor_class(k)
        yield f"{cls} (rel to max)", k, rel(got[k], ref[k], floor), "grad"
        tg, tr = tail_of(k, got[k], vc.case), tail_of(k, ref[k], vc.case)
        if tg is not None and slices:
            yield f"{cls} tail (rel to slice max)", f"{k}[tail]", rel(tg, tr, floor), "grad"


def finite(result):
    return all(bool(torch.isfinite(v).all()) for v in result.values())


def worst(vc, got, ref, **kw):
    """{'act': largest error of the activations, 'grad': of the gradients} under compare."""
    out = {"act": 0.0, "grad": 0.0}
    for _, _, err, cls in compare(vc, got, ref, **kw):
        out[cls] = max(out[cls], err if math.isfinite(err) else float("inf"))
    return out
