"""The value envelope of the tower kernels: one plain table of value regimes, each named for the device code it reaches, and the
shapes they run on.

Every other tower test draws its parameters at initialisation scale (gen_util.make_params) and its inputs from N(0,1) / U[0,1):
hidden pre-activations stay within about +-3, every LayerNorm row has mean 0 and variance 1, gamma is 1 +- 0.1.  The regimes below
are seeded numpy (PCG64) transforms of (params, x) as shape-envelope's run_case produces them; tests/value_ref.py measures what each
reaches on the float64 oracle, tests/test_host_value_cases.py holds the table to its reach conditions and reference-side margins
on the CPU, tests/test_gpu_value_envelope.py runs it against the float64 oracle on the device.

regime              reaches                                                        reach condition (float64 oracle)
gelu_tails          common.h pwl_index's saturation and clamp, cells 0 and 513 of  block 0: >= 5 % of the channel-mixing and of
                    every table form (and the dropout scale folded into cell       the token-mixing hidden pre-activations < -6,
                    513); fp32: erf_fast's clamp at |x / sqrt 2| = 4               >= 5 % >= 6; one within a cell (12 / 512) of each
ln_offset           the five LayerNorm statistics (two-pass variance, rsqf +       |row mean| / row std >= 50 at the first
                    Newton) where mean >> std                                      LayerNorm of every block
ln_constant_zero    rstd = 1 / sqrt(1e-5): rows of zeros                           the last token row of every third sample has
ln_constant_three   the same with rows of 3.0 (mean != 0, variance exactly 0)      variance exactly 0 at block 0's first LayerNorm
ln_gamma            gamma 0, < 0 and of several units; beta of a few units         gamma spans [0.05, 4] in size, both signs, zeros
outlier_channels    bf16 operand images with a wide range in one row               channels 3 and D - 2 of x are 50 x the others
trained             ln_offset, ln_gamma and gelu_tails at once                     gelu_tails' shares and ln_offset's ratio at block 0

Every strength is the largest tried at which the bf16 comparison stays well conditioned: the float64 oracle with bf16-rounded
`linear` operands (value_ref.bf16_twin) has to stay within a third of the bf16 bars under every measurement the GPU test makes --
whole tensors, and every tail and channel class relative to the slice's own maximum -- on every (regime, shape, dropout rate);
tests/test_host_value_cases.py asserts it, DESIGN.md section 2 ("Value envelope") lists the measured figures.
  gelu_tails   on both MLPs of the FIRST block: W1 (net.0.weight) x 4, W2 (net.3.weight) x 0.4, b1 evenly spaced over +-12 and
               shuffled, so that a hidden width of 8 has units in both tails too.  Shares beyond +-6: 0.24 .. 0.30.  Stronger
               settings are not well conditioned: W1 x 8 with b1 ~ 2 N(0,1) puts the MLP branch 8 x above the residual in dx and
               gives a hidden element an absolute bf16 error 8 x larger right where GELU' bends (twin 0.98 / 1.07 of the bars for
               outputs and dx / gradients); with the tails on the second block of the two-block tower as well, the last-token row
               of that block's token_mix.2.net.3.weight gradient is 5 % of the tensor's maximum and the twin is off by 1.04 bars
               relative to that row.
  ln_constant  the LAST token row (trailing padding) of every third sample is constant, the other rows are untouched.  Whole
               constant samples are not well conditioned (twin 1.5 / 0.8): their token mixing sees beta only, and the second
               LayerNorm normalises what is left.
  ln_offset    x = 50 + 0.3 N(0,1) per channel + 0.4 N(0,1): row std 0.5.  In towers of two blocks the output Linears (net.3 weight
               and bias of both MLPs) of every block but the last are scaled by 0.1, so that the second block's input keeps
               |mean| / std >= 50.
  ln_gamma     gamma = +-exp(U[log 0.05, log 4]), every 7th entry 0, beta ~ 2 N(0,1), on both LayerNorms of each block and the final
               one.
  outlier_channels   channels 3 and D - 2 of x times 50.
  trained      ln_offset with mean 40 (the float32 oracle's margin), then ln_gamma with gamma in [0.1, 2] and beta ~ N(0,1), then
               gelu_tails with W2 x 0.5.  The outlier
               channels and the constant rows stay in their own regimes: an offset of 50 under two channels x 50 leaves the
               ordinary channels 1e-3 of the row's std, below bf16 resolution, and a zero-variance row multiplies whatever error
               its upstream gradient carries by 316 (all regimes at once: twin 3.6 / 1.3).  So the tests built on `trained` --
               homogeneity of the backward, the engine steps -- see neither outlier channels nor zero-variance rows.
"""
from collections import namedtuple

import numpy as np
import torch

from shape_cases import Case
from split_cases import CASES as SPLIT_CASES

REGIME_SEED = 20240
FULL = dict(w1_scale=4.0, b1_span=12.0, w2_scale=0.4, tails_blocks=1,
            offset_mean=50.0, offset_ch_std=0.3, offset_row_std=0.4, offset_out_scale=0.1,     # sqrt(0.3^2 + 0.4^2) = 0.5: the row std
            gamma_lo=0.05, gamma_hi=4.0, beta_std=2.0, outlier_scale=50.0)
TRAINED = dict(FULL, gamma_lo=0.1, gamma_hi=2.0, beta_std=1.0, w2_scale=0.5, offset_mean=40.0)
GAMMA_ZERO_EVERY = 7
CONST_EVERY = 3
CONST_TOKENS = 1               # the trailing token rows (padding) of every third sample that are constant

REGIMES = ("gelu_tails", "ln_offset", "ln_constant_zero", "ln_constant_three", "ln_gamma", "outlier_channels", "trained")
DROPOUT_REGIMES = ("gelu_tails", "trained")       # these also run at p = 0.5 (one-bit masks, masked fp16 table) and p = 0.1


def _c(name, kind, D, N, T, C, nb=1, B=2):
    return Case(name, kind, D, N, T, C, nb, B, 0.0, None, None)


# (path, Case): the smallest shapes that reach every build -- not the workloads' shapes
SHAPES = [
    ("fused", _c("fused_n4_d64", "block", 64, 4, 16, 100, B=5)),           # SPW 4, ragged tile
    ("fused", _c("fused_n8_d128", "block", 128, 8, 32, 96, B=3)),          # the D = 128 bf16 builds
    ("fused", _c("fused_n3_d32_x2", "fusion", 32, 3, 8, 31, nb=2, B=6)),   # two blocks and the final LayerNorm (tile.h row_stats)
    ("wide", _c("wide_n16_d64", "block", 64, 16, 8, 90, B=3)),
    ("wide", _c("wide_n5_d256", "block", 256, 5, 24, 33, B=3)),
    ("wide", _c("wide_n9_d32", "block", 32, 9, 8, 45, B=5)),               # two samples per workgroup
    # column-split path (bf16 only, forced with M2M_SPLIT=1): the smallest case of tests/split_cases.py that m2m_split_form accepts
    ("split", SPLIT_CASES[0]._replace(name="split_u4_s2")),
]
assert SPLIT_CASES[0].name == "u4_s2" and SPLIT_CASES[0].p == 0.0

ValueCase = namedtuple("ValueCase", "name regime path case")


def _table():
    out = []
    for path, shape in SHAPES:
        for regime in REGIMES:
            ps = (0.0, 0.5, 0.1) if regime in DROPOUT_REGIMES else (0.0,)
            for p in ps:
                tag = "" if p == 0 else ("_half" if p == 0.5 else "_gen")
                out.append(ValueCase(f"{regime}-{shape.name}{tag}", regime, path, shape._replace(p=p)))
    return out


CASES = _table()


def precisions(vc):
    return ("bf16",) if vc.path == "split" else ("fp32", "bf16")


def by_name(name):
    return next(c for c in CASES if c.name == name)


# ---- the transforms ---------------------------------------------------------------------------------------------------------
def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _blocks(params):
    """Key prefixes of the MixerBlocks of a parameter set ('' for a lone block)."""
    return sorted({k[:k.index("token_mix.")] for k in params if "token_mix." in k})


def _gelu_tails(params, x, rng, k):
    for pre in _blocks(params)[:k["tails_blocks"]]:
        for ff in ("token_mix.2.", "channel_mix.1."):
            w, b = pre + ff + "net.0.weight", pre + ff + "net.0.bias"
            params[w] = params[w] * k["w1_scale"]
            n = params[b].numel()          # evenly spaced over +-b1_span, shuffled: every width, T = 8 included, has units in both tails
            params[b] = _f32(rng.permutation(np.linspace(-k["b1_span"], k["b1_span"], n)))
            params[pre + ff + "net.3.weight"] = params[pre + ff + "net.3.weight"] * k["w2_scale"]
    return x


def _ln_offset(params, x, rng, k):
    ch = k["offset_ch_std"] * rng.standard_normal(x.shape[-1])
    for pre in _blocks(params)[:-1]:
        for ff in ("token_mix.2.", "channel_mix.1."):
            for leaf in ("net.3.weight", "net.3.bias"):
                params[pre + ff + leaf] = params[pre + ff + leaf] * k["offset_out_scale"]
    return _f32(k["offset_mean"] + ch + k["offset_row_std"] * x.numpy())


def _ln_constant(value):
    def f(params, x, rng, k):
        x = x.clone()
        x[CONST_EVERY - 1::CONST_EVERY, -CONST_TOKENS:] = value
        return x
    return f


def _ln_gamma(params, x, rng, k):
    for key in list(params):
        ln = key.endswith("token_mix.0.weight") or key.endswith("channel_mix.0.weight") or key.endswith("layer_norm.weight")
        lb = key.endswith("token_mix.0.bias") or key.endswith("channel_mix.0.bias") or key.endswith("layer_norm.bias")
        shp = tuple(params[key].shape)
        if ln:
            g = np.exp(rng.uniform(np.log(k["gamma_lo"]), np.log(k["gamma_hi"]), shp)) * rng.choice([-1.0, 1.0], shp)
            g[::GAMMA_ZERO_EVERY] = 0.0
            params[key] = _f32(g)
        elif lb:
            params[key] = _f32(k["beta_std"] * rng.standard_normal(shp))
    return x


def outlier_index(D):
    return (3, D - 2)


def _outliers(params, x, rng, k):
    x = x.clone()
    for c in outlier_index(x.shape[-1]):
        x[..., c] *= k["outlier_scale"]
    return x


# every step draws from a stream of its own (REGIME_SEED, its index here), so `trained` gets the draws of the single regimes
_STEP_ORDER = (_ln_offset, _outliers, _ln_gamma, _gelu_tails)
_STEPS = {
    "gelu_tails": (_gelu_tails,),
    "ln_offset": (_ln_offset,),
    "ln_constant_zero": (_ln_constant(0.0),),
    "ln_constant_three": (_ln_constant(3.0),),
    "ln_gamma": (_ln_gamma,),
    "outlier_channels": (_outliers,),
    "trained": (_ln_offset, _ln_gamma, _gelu_tails),
}


def transform(regime):
    """(params, x) -> (params', x'): the regime applied to initialisation-scale parameters and a standard-normal input.  The input
    dict is not modified; every tensor of the result is float32."""
    def f(params, x):
        params = type(params)((k, v.clone()) for k, v in params.items())
        k = TRAINED if regime == "trained" else FULL
        for step in _STEPS[regime]:
            i = _STEP_ORDER.index(step) if step in _STEP_ORDER else len(_STEP_ORDER)
            x = step(params, x, np.random.default_rng([REGIME_SEED, i]), k)
        return params, x.float()
    return f


def transform_towers(regime, params, towers):
    """The parameter side of a regime applied to each tower of a task model's parameter set (key prefixes `towers`); every other
    tensor -- embeddings, heads -- keeps its initialisation scale.  The inputs are the task's own batches."""
    out = type(params)((k, v.clone()) for k, v in params.items())
    k = TRAINED if regime == "trained" else FULL
    for t, pre in enumerate(towers):
        sub = {key: out[key] for key in out if key.startswith(pre) and ("mixer_blocks." in key or key.startswith(pre + "layer_norm."))}
        for step in _STEPS[regime]:
            if step in (_ln_gamma, _gelu_tails):
                step(sub, None, np.random.default_rng([REGIME_SEED, _STEP_ORDER.index(step), t]), k)
        out.update(sub)
    return out


def constant_samples(B):
    return list(range(CONST_EVERY - 1, B, CONST_EVERY))


# ---- which device code a case runs (restated as for test_host_cpu.test_shape_envelope_covers_every_build) ---------------------
LN_SITES = ("tile.h row_stats", "tile.h reg_stats", "token_wide.hip tok_row_stats", "token_wide.hip ln1_bwd_rows", "split_mix.hip")
TABLE_FORMS = ("forward-only {a, b}", "fp32 {a, b, c, d}", "fp16", "fp16 masked", "fp32 closed form")


def ln_sites(vc):
    """The LayerNorm statistics sites a case's launches run: the fused launches and the wide path's channel-mixing launch keep a
    row in registers (reg_stats); a tower's final LayerNorm goes through ln_to_tile / ln_backward_tile (row_stats); the wide token
    launches have their own two sites; the column-split mix kernels theirs (row_stats through the tile calls, and the backward's
    own call)."""
    c = vc.case
    if vc.path == "split":
        return {"split_mix.hip", "tile.h row_stats"}
    sites = {"tile.h reg_stats"}
    if c.kind != "block":
        sites.add("tile.h row_stats")
    if vc.path == "wide":
        sites |= {"token_wide.hip tok_row_stats", "token_wide.hip ln1_bwd_rows"}
    return sites


def table_forms(vc, prec):
    """The GELU forms of a case's launches: tower_fwd.hip fills the forward-only table, tower_bwd.hip the fp16 one (read through the
    keep-mask at p = 0.5), the split kernels the fp32 four-coefficient table (their chain forward a two-coefficient one); fp32 mode
    evaluates erf_fast."""
    if prec == "fp32":
        return {"fp32 closed form"}
    if vc.path == "split":
        return {"fp32 {a, b, c, d}", "forward-only {a, b}"}
    return {"forward-only {a, b}", "fp16 masked" if vc.case.p == 0.5 else "fp16"}
