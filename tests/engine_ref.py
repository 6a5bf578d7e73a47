"""Helpers of the engine tests: the float64 reference of an engine step (autograd through the oracle's task forwards +
oracle.adam_step, in the manner of fusion_ref.Step, with the kernels' dropout masks), the dropout masks and the dispatch
decisions read off a built engine, and the gradient-clearing check."""
from collections import OrderedDict

import torch

import drop_ref as DR
import gen_util as G
from oracle import m2mixer_oracle as O

NOISE_KEYS = ("token_mix.2.net.3.bias",)       # rounding-level gradient under a final LayerNorm


def p_effective(p):
    """The keep probability is quantised to 16 bits; the kernels scale by 1 / keep_q (drop_ref.drop_thr: the library's rounding)."""
    return DR.p_effective(p)


def grads_cleared(eng):
    """After an optimizer step every gradient element Adam is responsible for clearing is zero: everything outside the ranges
    the engine leaves to the next backward's overwriting weight-gradient launch (engine._setup_wgrad)."""
    g = eng.flat_g.detach().clone()
    for lo, n, _, keep in eng._ranges_add:
        if keep:
            g[lo:lo + n] = 0
    return float(g.abs().max()) == 0.0


def assert_update_forms_bit_identical(sep, fus):
    """A two-tower engine that updates with the flat Adam followed by m2m_pack_all (sep) against one that updates with the
    one-launch m2m_adam_pack_all (fus), after the same steps from the same state: parameters, both moments, the cleared
    gradient and every packed operand copy the kernels read, BIT FOR BIT."""
    assert fus._fused_update and not sep._fused_update
    assert torch.equal(sep.flat_p, fus.flat_p) and torch.equal(sep.flat_m, fus.flat_m) and torch.equal(sep.flat_v, fus.flat_v)
    assert torch.equal(sep.flat_g, fus.flat_g)
    for ts, tf in zip((sep.t_a, sep.t_b, sep.t_fus), (fus.t_a, fus.t_b, fus.t_fus)):
        for i in range(ts.nblocks):
            for k, v in ts._keep[f"packed{i}"].items():
                if k == "w1tc" and ts.pack_all_skips_w1tc():
                    continue
                assert torch.equal(v, tf._keep[f"packed{i}"][k]), (i, k)
    for es, ef in zip((sep.e_a, sep.e_b), (fus.e_a, fus.e_b)):
        assert torch.equal(es._keep["wn"], ef._keep["wn"])


def tower_masks(rt, B, seed, step):
    """The keep-masks of one tower's dropout sites at `step`, per block, in the oracle's layout."""
    blocks = []
    for b in range(rt.nblocks):
        m = {"tok_h": rt.dropout_mask(b, 0, B, seed, step).view(B, rt.D, rt.T),
             "tok_o": rt.dropout_mask(b, 1, B, seed, step).view(B, rt.D, rt.N),
             "ch_h": rt.dropout_mask(b, 2, B, seed, step).view(B, rt.N, rt.Cp)[:, :, :rt.C],
             "ch_o": rt.dropout_mask(b, 3, B, seed, step).view(B, rt.N, rt.D)}
        blocks.append({k: v.float().cpu() for k, v in m.items()})
    return blocks


def mlp_masks(mlp, B, seed, step):
    """The keep-masks of the plain MLP's hidden layers at `step`, from the host replica of the dropout stream (tests/drop_ref.py:
    the MLP has no mask probe): one (B, width) tensor per hidden layer, as oracle.mlp takes them."""
    d = mlp.desc
    return [torch.from_numpy(DR.mlp_mask(seed, step, d.site_base, l, d.p_drop, B, mlp.dims[l + 1])).float()
            for l in range(mlp.nlayers - int(mlp.has_out))]


def engine_masks(eng, B):
    """The keep-masks of every dropout site of an engine at its current step: the three towers of a two-tower engine, or the MIMIC
    engine's two towers ("time", "fusion") and its static MLP ("static")."""
    from m2_mixer_amd.engine import MimicEngine
    step, seed = int(eng.drop_step[0]), eng.seed
    if isinstance(eng, MimicEngine):
        return {"time": tower_masks(eng.t_time, B, seed, step), "fusion": tower_masks(eng.t_fus, B, seed, step),
                "static": mlp_masks(eng.mlp, B, seed, step)}
    return {name: tower_masks(rt, B, seed, step) for name, rt in ((eng.MODS[0], eng.t_a), (eng.MODS[1], eng.t_b), ("fusion", eng.t_fus))}


def masks_equal(a, b):
    """Two results of engine_masks (or None: dropout off) hold the same masks.  A group is a list: one dict of site masks per tower
    block, or one tensor per hidden layer of the MIMIC engine's static MLP."""
    if a is None or b is None:
        return a is b
    flat = lambda m: [t for n in m for x in m[n] for t in (x.values() if isinstance(x, dict) else (x,))]
    return len(flat(a)) == len(flat(b)) and all(torch.equal(x, y) for x, y in zip(flat(a), flat(b)))


# ---- the case table's engines ------------------------------------------------------------------------------------------------
HEAD_LOGITS = {"avmnist": ("image_logits", "audio_logits", "logits"), "mmimdb": ("image_logits", "text_logits", "logits"),
               "mimic": ("logits_static", "logits_time", "logits")}
HEAD_LOSSES = {"avmnist": ("loss_image", "loss_audio", "loss_fusion", "loss"), "mmimdb": ("loss_image", "loss_text", "loss_fusion", "loss"),
               "mimic": ("loss_static", "loss_time", "loss_fusion", "loss")}


def case_shapes(case) -> "OrderedDict[str, tuple]":
    return {"avmnist": G.avmnist_shapes, "mmimdb": G.mmimdb_shapes, "mimic": G.mimic_shapes}[case.engine](case.cfg)


def case_batch(case, seed):
    return {"avmnist": G.avmnist_batch, "mmimdb": G.mmimdb_batch, "mimic": G.mimic_batch}[case.engine](case.B, seed, case.cfg)


def engine_class(case):
    from m2_mixer_amd import engine as E
    return {"avmnist": E.AVMnistEngine, "mmimdb": E.MMIMDBEngine, "mimic": E.MimicEngine}[case.engine]


def case_forward(case, batch, p, drop_p=0.0, masks=None):
    """The task's shared_step in float64: {"logits": (3, B, K) in the engine's head order, "losses": (4,) heads then total}."""
    x1, x2, y = batch
    x1, x2 = x1.double(), x2.double()
    if case.engine == "avmnist":
        o = O.avmnist_forward(x1, x2, y, p, case.cfg, drop_p, masks)
    elif case.engine == "mmimdb":
        o = O.mmimdb_forward(x1, x2, y.double(), p, case.cfg, torch.tensor(case.cfg["pos_weight"], dtype=torch.float64), drop_p, masks)
    else:
        o = O.mimic_forward(x1, x2, y, p, case.cfg, drop_p, masks)
    return {"logits": torch.stack([o[k] for k in HEAD_LOGITS[case.engine]]), "losses": torch.stack([o[k] for k in HEAD_LOSSES[case.engine]])}


class Step:
    """Autograd through case_forward in float64, then torch.optim.Adam's update (oracle.adam_step) of every parameter."""

    def __init__(self, case, params, lr):
        self.case, self.lr = case, lr
        self.p = {k: v.detach().double().clone() for k, v in params.items()}
        self.t, self.m, self.v = 0, {}, {}

    def forward(self, batch, params=None):
        with torch.no_grad():
            return case_forward(self.case, batch, self.p if params is None else params)

    def step(self, batch, masks=None):
        leaves = {k: v.clone().requires_grad_(True) for k, v in self.p.items()}
        out = case_forward(self.case, batch, leaves, p_effective(self.case.p) if masks is not None else 0.0, masks)
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


def decisions(eng) -> dict:
    """Every dispatch decision of tests/engine_cases.py as the built engine took it."""
    from m2_mixer_amd.engine import MimicEngine
    from m2_mixer_amd.runtime import can_group, can_group_embeds, can_pack_all
    B = eng.B
    d = {"heads_pool": bool(eng._heads_pool), "fused_heads": bool(eng._fused_heads),
         "pack_all": bool(can_pack_all(eng._towers, eng._embeds)), "adam_pack": eng._adam_pack_modules() is not None,
         "wide_fus": bool(eng.t_fus.wide)}
    if isinstance(eng, MimicEngine):
        d.update(time_wide=bool(eng.t_time.wide), mlp_ride=bool(eng._mlp_ride))
        return d
    d.update(grouped=bool(can_group(eng.t_a, eng.t_b, B)), embeds_grouped=bool(can_group_embeds(eng.e_a, eng.e_b)),
             wide_a=bool(eng.t_a.wide), wide_b=bool(eng.t_b.wide), head_part=eng._head_part is not None,
             embed_fast=bool(eng._embed_towers), embed_overwrite=bool(eng.e_a.desc.wgrad_flags & 1) and bool(eng.e_b.desc.wgrad_flags & 1),
             group_slots=bool(eng.t_a.desc.wgrad_flags & 4) and bool(eng.t_b.desc.wgrad_flags & 4))
    for name, t in (("a", eng.t_a), ("b", eng.t_b), ("fus", eng.t_fus)):
        d["overwrite_" + name] = bool(t.desc.wgrad_flags & 1)
        d["groups_" + name] = int(t.wgrad_groups(B))
        d["slot_" + name] = any(t is s for s in eng._slot_towers)
    return d


def expected(case, prec: str) -> dict:
    """The case's `expect` for one precision."""
    return {k: (v[prec] if isinstance(v, dict) else v) for k, v in case.expect.items()}
