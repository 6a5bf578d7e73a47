"""The I/O contract of the tower entry points (include/m2mixer.h: m2m_tower_forward / _backward, m2m_towers_forward / _backward
and the m2m_tower_wgrad behind them): one plain table of towers and pairs at the smallest shapes that still leave a ragged last
tile on each execution path, the restated host rules that say which path a case takes, the inputs of the GPU test and their
float64 reference.

tests/test_host_tower_io.py classifies every case with these rules, checks that the table reaches every path, and checks on the
CPU -- with the float64 oracle alone -- that the inputs make the GPU test's clauses sharp (a kernel that dropped one upstream
term, one input part, or read one token for the mean cannot hide under the bf16 bar).  tests/test_gpu_tower_io.py runs the
clauses.

Singles are shape_cases.Case rows ("fusion": final LayerNorm, "block": none), pairs are two split_cases.Tow; dropout is 0 in
the table (the evaluation clause rebuilds three towers with p = 0.5).
"""
import functools

import numpy as np
import torch

import gen_util as G
import split_cases as SC
from oracle import m2mixer_oracle as O
from shape_cases import Case
from split_cases import Tow

GROUP_BLOCKS = 4        # M2M_GROUP_BLOCKS: blocks per tower of a two-tower launch
TW_COLS = 64            # columns of a token-mixing workgroup (csrc/token_wide.hip)


def _s(name, kind, D, N, T, C, nb, B):
    return Case(name, kind, D, N, T, C, nb, B, 0.0, None, None)


# name -> Case; the comment: what the size forces
SINGLES = [
    _s("fused_n3", "fusion", 32, 3, 8, 33, 2, 7),        # 5 samples per 16-row tile: two tiles, the second with two samples; 15 of 16 rows
    _s("fused_n7_noln", "block", 64, 7, 24, 31, 1, 3),   # no final LayerNorm; 2 samples per tile; NMAX 8 / TG 8
    _s("wide_d32", "fusion", 32, 9, 8, 33, 2, 3),        # two samples per token workgroup, odd B; 27 rows: ragged 16-row chain tile
    _s("wide_d256", "fusion", 256, 5, 12, 40, 2, 3),     # D = 256 with N <= 8
    _s("split_single", "fusion", 128, 3, 24, 130, 2, 7),  # split_cases' u5_s2_odd without dropout; bf16 only
]
PAIRS = {
    # both N <= 4, same token class; 2 and 2 tiles with different fill, unequal depth
    "fused_pair": (Tow(32, 3, 8, 33, 2, 7, 0.0), Tow(32, 4, 8, 31, 1, 7, 0.0)),
    # 1 and 3 tiles: the shorter tower's workgroups leave early
    "fused_pair_tiles": (Tow(64, 1, 16, 40, 1, 9, 0.0), Tow(64, 4, 16, 33, 1, 9, 0.0)),
    # unequal N: Nmax differs from one tower's N
    "wide_pair": (Tow(256, 5, 12, 40, 2, 3, 0.0), Tow(256, 9, 8, 33, 2, 3, 0.0)),
    # 1 and 2 chain row tiles (split_cases.PAIR_UNEQUAL without dropout)
    "split_pair": tuple(t._replace(p=0.0) for t in SC.PAIR_UNEQUAL),
}
# the path every case must take: (fused | wide | split, single | pair)
PATHS = {"fused_n3": ("fused", "single"), "fused_n7_noln": ("fused", "single"), "wide_d32": ("wide", "single"),
         "wide_d256": ("wide", "single"), "split_single": ("split", "single"), "fused_pair": ("fused", "pair"),
         "fused_pair_tiles": ("fused", "pair"), "wide_pair": ("wide", "pair"), "split_pair": ("split", "pair")}
SINGLE = {c.name: c for c in SINGLES}
NAMES = [c.name for c in SINGLES] + list(PAIRS)


def precisions(name):
    return ("bf16",) if PATHS[name][0] == "split" else ("fp32", "bf16")


CASE_PRECS = [(n, p) for n in NAMES for p in precisions(n)]
# accumulation runs once per path class; the parts clause on these pairs; the evaluation clause on these singles
ACCUMULATE = ["fused_n3", "fused_pair", "wide_d32", "wide_pair", "split_single", "split_pair"]
PARTS_CASES = ["fused_pair", "split_pair"]
EVAL_CASES = ["fused_n3", "wide_d32", "split_single"]


def towers_of(name):
    """[(Tow, has_final_ln)] of a case."""
    if name in SINGLE:
        c = SINGLE[name]
        return [(Tow(c.D, c.N, c.T, c.C, c.nb, c.B, c.p), c.kind == "fusion")]
    return [(t, True) for t in PAIRS[name]]


# ---- the host rules -----------------------------------------------------------------------------------------------------
def is_wide(t):
    return t.N > 8 or t.D > 128


def can_group(a, b):
    """m2m_can_group (csrc/tower_fwd.hip) of two towers of one precision."""
    if is_wide(a) or is_wide(b) or a.D != b.D or a.p != b.p:
        return False
    if (a.N <= 4) != (b.N <= 4) or (a.T % 16 == 0) != (b.T % 16 == 0):
        return False
    return a.nb <= GROUP_BLOCKS and b.nb <= GROUP_BLOCKS


def can_group_wide(a, b, B):
    """m2m_can_group_wide (csrc/token_wide.hip) of two towers of one precision (M2M_WIDE_GROUP unset)."""
    if not is_wide(a) or not is_wide(b) or a.D != b.D or a.D != 256 or a.p != b.p:
        return False
    if (a.T <= 16) != (b.T <= 16) or a.T > 16:
        return False
    if a.nb != b.nb or a.nb < 1 or a.nb > GROUP_BLOCKS:
        return False
    chunks, spw = (a.D // TW_COLS, 1) if a.D >= TW_COLS else (1, TW_COLS // a.D)
    return (B + spw - 1) // spw * chunks <= 256


def path_of(name, prec, split=True):
    """(fused | wide | split, single | pair) of a case under M2M_SPLIT=1 (split: the switch the split cases run under)."""
    tows = [t for t, _ in towers_of(name)]
    mode = 1 if split and PATHS[name][0] == "split" else 0
    if len(tows) == 1:
        t = tows[0]
        if is_wide(t):
            return ("wide", "single")
        return ("split" if SC.split_form(t, prec=prec, mode=mode) else "fused", "single")
    a, b = tows
    if SC.split_form(a, b, prec=prec, mode=mode):
        return ("split", "pair")
    if can_group_wide(a, b, a.B):
        return ("wide", "pair")
    return ("fused", "pair") if can_group(a, b) else ("refused", "pair")


# ---- inputs and their float64 reference ------------------------------------------------------------------------------------
# The seed of a (case, tower): the first one from its base whose float64 REFERENCE meets the conditions of
# tests/test_host_tower_io.py (nothing a kernel computes enters the choice); found once, fixed here, re-checked by that test.
SEEDS = {("fused_n3", 0): 1004, ("wide_d32", 0): 3004, ("wide_d256", 0): 4001, ("split_single", 0): 5002, ("fused_pair", 0): 6014,
         ("fused_pair_tiles", 0): 7023, ("wide_pair", 0): 8001, ("split_pair", 0): 9004}       # (every other tower: its base seed)
BASE_SEED = 1000          # case c, tower i: seeds from 1000 (c + 1) + 100 i on
MAX_PARTS = 4


def base_seed(name, i):
    return BASE_SEED * (NAMES.index(name) + 1) + 100 * i


def seed_of(name, i):
    return SEEDS.get((name, i), base_seed(name, i))


def keys_of(tow, has_ln):
    from_fields = ["token_mix.0.weight", "token_mix.0.bias", "token_mix.2.net.0.weight", "token_mix.2.net.0.bias",
                   "token_mix.2.net.3.weight", "token_mix.2.net.3.bias", "channel_mix.0.weight", "channel_mix.0.bias",
                   "channel_mix.1.net.0.weight", "channel_mix.1.net.0.bias", "channel_mix.1.net.3.weight", "channel_mix.1.net.3.bias"]
    return [f"mixer_blocks.{i}.{k}" for i in range(tow.nb) for k in from_fields] + (["layer_norm.weight", "layer_norm.bias"] if has_ln else [])


def draw(tow, has_ln, seed):
    """(params, xparts (4, B, N, D), d_out (B, N, D), d_pooled (B, D)) of a tower, float32 on the CPU.  The input of a call with p
    parts is the sum of the first p; d_pooled is drawn at N times the scale of d_out, so that the two contributions to a token's
    gradient (d_out and d_pooled / N) are comparable."""
    cfg = dict(hidden_dim=tow.D, token_dim=tow.T, channel_dim=tow.C, num_mixers=tow.nb)
    params = G.make_params(G.tower_shapes("", cfg, tow.N, "none"), seed)
    params = {k: params[k] for k in keys_of(tow, has_ln)}
    rng = np.random.default_rng(seed + 1)
    f32 = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    return params, f32(MAX_PARTS, tow.B, tow.N, tow.D), f32(tow.B, tow.N, tow.D), tow.N * f32(tow.B, tow.D)


class _Bf16OperandLinear(torch.autograd.Function):
    """linear() whose matrix products take their operands rounded to bf16, forward and backward, and accumulate in float64:
    what a bf16 MFMA does to the operands of the oracle's products, and nothing else."""

    @staticmethod
    def forward(ctx, x, w, b):
        xr, wr = _bf16(x), _bf16(w)
        ctx.save_for_backward(xr, wr)
        return xr @ wr.transpose(-1, -2) + b

    @staticmethod
    def backward(ctx, dy):
        xr, wr = ctx.saved_tensors
        dyr = _bf16(dy)
        return dyr @ wr, dyr.reshape(-1, dyr.shape[-1]).t() @ xr.reshape(-1, xr.shape[-1]), dy.reshape(-1, dy.shape[-1]).sum(0)


def _bf16(x):
    return x.to(torch.bfloat16).to(x.dtype)


def run_oracle(tow, has_ln, params, x, d_out, d_pooled, bf16_operands=False):
    """float64: dict(out, pooled, dx, grads) for the upstream gradient d_out (or None) + d_pooled (or None).  bf16_operands:
    the same with the operands of every Linear rounded to bf16 (the conditioning of the reference, see conditioning())."""
    if bf16_operands:
        plain, O.linear = O.linear, lambda x, w, b: _Bf16OperandLinear.apply(x, w, b)
        try:
            return run_oracle(tow, has_ln, params, x, d_out, d_pooled)
        finally:
            O.linear = plain
    leaves = {k: v.double().requires_grad_(True) for k, v in params.items()}
    xr = x.double().requires_grad_(True)
    y = xr
    for i in range(tow.nb):
        y = O.mixer_block(y, leaves, f"mixer_blocks.{i}.", 0.0, None)
    if has_ln:
        y = O.layer_norm(y, leaves["layer_norm.weight"], leaves["layer_norm.bias"])
    pooled = y.mean(1)
    loss = (y * 0).sum()
    if d_out is not None:
        loss = loss + (y * d_out.double()).sum()
    if d_pooled is not None:
        loss = loss + (pooled * d_pooled.double()).sum()
    loss.backward()
    return dict(out=y.detach(), pooled=pooled.detach(), dx=xr.grad, grads={k: v.grad for k, v in leaves.items()})


FORMS = ("out", "pooled", "both", "none")


@functools.lru_cache(maxsize=None)
def reference(name, i, parts=1, form="out", seed=None, bf16_operands=False):
    """The float64 reference of tower i of a case, computed once per (parts, upstream form) and shared by the tests (seed: another
    than the case's own, for the search of tests/test_host_tower_io.py)."""
    tow, has_ln = towers_of(name)[i]
    params, xparts, d_out, d_pooled = draw(tow, has_ln, seed_of(name, i) if seed is None else seed)
    return run_oracle(tow, has_ln, params, xparts[:parts].double().sum(0), d_out if form in ("out", "both") else None,
                      d_pooled if form in ("pooled", "both") else None, bf16_operands)


def conditioning(name, i, parts, form, seed=None):
    """How far bf16 OPERAND rounding alone moves the float64 reference: (activations, parameter gradients), each the largest
    error relative to its tensor's maximum, as the GPU test measures.  A parameter gradient is a sum over all token rows in
    which large terms can cancel (behind a LayerNorm the gradient of a token row sums to zero over the hidden units, so whatever
    the hidden activation has in common over them cancels in the token MLP's gradients -- with ONE token nearly everything);
    the rounding of the terms does not cancel with them.  A case whose reference is that ill-conditioned measures its own
    inputs, not a kernel."""
    ref, rnd = reference(name, i, parts, form, seed), reference(name, i, parts, form, seed, True)
    err = lambda a, b, floor=0.0: float((a - b).abs().max()) / max(float(b.abs().max()), floor, 1e-30)
    acts = max(err(rnd[k], ref[k]) for k in ("out", "pooled", "dx"))
    return acts, max(err(rnd["grads"][k], g, grad_floor(k, ref["grads"])) for k, g in ref["grads"].items())


def grad_floor(key, grads):
    """tests/test_gpu_shape_envelope.py's rule for token_mix.2.net.3.bias: behind a LayerNorm its true gradient is exactly zero
    and is measured against its weight's gradient scale."""
    if not key.endswith("token_mix.2.net.3.bias"):
        return 0.0
    floor = float(grads[key[:-4] + "weight"].abs().max())
    return 0.0 if float(grads[key].abs().max()) > 1e-6 * floor else floor


def g0_of(key, grads, seed=77):
    """The pre-fill of a gradient: fixed random multiples of 1/8 in [-1, 1], times the power of two at or above the float64
    reference gradient's maximum (its floor where the reference is exactly zero) -- the scale comes from the reference alone,
    and G0 is exact in float32."""
    ref = grads[key]
    scale = 2.0 ** int(np.ceil(np.log2(max(float(ref.abs().max()), grad_floor(key, grads), 1e-30))))
    rng = np.random.default_rng(seed + len(key) + ref.numel())
    return torch.from_numpy(rng.integers(-8, 9, size=tuple(ref.shape)).astype(np.float64) / 8.0 * scale)
