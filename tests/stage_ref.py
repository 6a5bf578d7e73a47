"""Stage two of the reference's two-stage training in float64 (models/avmnist.py:292-293, :314-324): FrozenStep is an
engine_ref.Step whose training loss is losses[2] (loss_fusion, coefficient 1) and whose Adam updates the trainable keys only --
the frozen keys (the two modality towers with their embeddings, and their two heads) keep their parameters and both moments.
The ONE step count goes on from stage one, as the fused Adam's does."""
import torch

import engine_ref as R
from oracle import m2mixer_oracle as O

MODS = {"avmnist": ("image", "audio"), "mmimdb": ("image", "text"), "mimic": ("static", "time")}


def frozen_prefixes(case):
    """The key prefixes _MultiLossModule._freeze_modalities stops training, written out per task (not taken from the engine)."""
    a, b = MODS[case.engine]
    towers = ("static_extractor.", "time_mixer.") if case.engine == "mimic" else (f"{a}_mixer.", f"{b}_mixer.")
    return towers + (f"classifier_{a}.", f"classifier_{b}.")


def is_frozen(case, key):
    return key.startswith(frozen_prefixes(case))


def flat_ranges(shapes, keys):
    """[(lo, hi)] of `keys` in the flat buffer laid out in the order of `shapes`, neighbours not merged."""
    out, off = [], 0
    for k, shp in shapes.items():
        n = int(torch.Size(shp).numel())
        if k in keys:
            out.append((off, off + n))
        off += n
    return out


class FrozenStep(R.Step):
    """Continue a Step (its parameters, moments and step count) in stage two."""

    def __init__(self, step):
        self.case, self.lr = step.case, step.lr
        self.p = {k: v.clone() for k, v in step.p.items()}
        self.t = step.t
        self.m = {k: v.clone() for k, v in step.m.items()}
        self.v = {k: v.clone() for k, v in step.v.items()}

    def step(self, batch, masks=None):
        leaves = {k: v.clone().requires_grad_(True) for k, v in self.p.items()}
        out = R.case_forward(self.case, batch, leaves, R.p_effective(self.case.p) if masks is not None else 0.0, masks)
        out["losses"][2].backward()
        self.t += 1
        grads = {}
        for k, leaf in leaves.items():
            if is_frozen(self.case, k):
                continue
            g = leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)
            grads[k] = g
            m, v = self.m.get(k, torch.zeros_like(g)), self.v.get(k, torch.zeros_like(g))
            self.p[k], self.m[k], self.v[k] = O.adam_step(self.p[k], g, m, v, self.t, self.lr)
        losses = out["losses"].detach().clone()
        losses[3] = losses[2]                            # the training loss of stage two
        return {"logits": out["logits"].detach(), "losses": losses, "grads": grads}
