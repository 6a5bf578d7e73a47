"""Gradient-Blending in float64 on engine_ref.Step: the modalities-only stage (ModalityStep, the mirror image of
stage_ref.FrozenStep) and the whole of the reference's GradBlend.get_weights() (modules/gradblend.py:62-109) restated on it --
the image-only and the audio-only model trained SEPARATELY (as the reference trains them; the engines train both at once),
then the fusion mixer over frozen towers (stage_ref.FrozenStep from a fresh optimizer)."""
import torch

import engine_ref as R
import stage_ref as S
from oracle import m2mixer_oracle as O


def modality_prefixes(case, heads=(0, 1)):
    """The key prefixes the unimodal model(s) `heads` (indices into the task's two modalities) train: the tower with its
    embedding and its own head -- written out per task, not taken from the engine."""
    a, b = S.MODS[case.engine]
    towers = ("static_extractor.", "time_mixer.") if case.engine == "mimic" else (f"{a}_mixer.", f"{b}_mixer.")
    heads_ = (f"classifier_{a}.", f"classifier_{b}.")
    return tuple(towers[h] for h in heads) + tuple(heads_[h] for h in heads)


def is_modal(case, key, heads=(0, 1)):
    return key.startswith(modality_prefixes(case, heads))


class ModalityStep(R.Step):
    """Continue a Step (its parameters, moments and step count) in the modalities-only stage: the training loss is the sum of the
    chosen modality heads' losses (both: l0 + l1), Adam updates their keys only; the fusion keys -- and a modality left out --
    keep their parameters and both moments."""

    def __init__(self, step, heads=(0, 1)):
        self.case, self.lr, self.heads = step.case, step.lr, tuple(heads)
        self.p = {k: v.clone() for k, v in step.p.items()}
        self.t = step.t
        self.m = {k: v.clone() for k, v in step.m.items()}
        self.v = {k: v.clone() for k, v in step.v.items()}

    def step(self, batch, masks=None):
        leaves = {k: v.clone().requires_grad_(True) for k, v in self.p.items()}
        out = R.case_forward(self.case, batch, leaves, R.p_effective(self.case.p) if masks is not None else 0.0, masks)
        sum(out["losses"][h] for h in self.heads).backward()
        self.t += 1
        grads = {}
        for k, leaf in leaves.items():
            if not is_modal(self.case, k, self.heads):
                continue
            g = leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)
            grads[k] = g
            m, v = self.m.get(k, torch.zeros_like(g)), self.v.get(k, torch.zeros_like(g))
            self.p[k], self.m[k], self.v[k] = O.adam_step(self.p[k], g, m, v, self.t, self.lr)
        losses = out["losses"].detach().clone()
        losses[2] = 0.0                                  # the fusion head is not computed in this stage
        losses[3] = losses[0] + losses[1]
        return {"logits": out["logits"].detach(), "losses": losses, "grads": grads}


def batches(tensors, B, order=None):
    n = tensors[0].shape[0]
    for lo in range(0, n, B):
        idx = slice(lo, lo + B) if order is None else order[lo:lo + B]
        yield tuple(t[idx] for t in tensors)


def loss_sums(step, tensors, B):
    """The three heads' sums of batch-mean losses over `tensors` in their stored order (gradblend.py:43-60), float64."""
    tot = torch.zeros(3, dtype=torch.float64)
    for b in batches(tensors, B):
        tot += step.forward(b)["losses"][:3]
    return tot


def blend(a, b, c, d):
    """gradblend.py:85-90 written out again (not imported from the package under test)."""
    return abs(((d - c) - (b - a)) / ((d - b) ** 2))


def get_weights(case, params, tensors, nval, B, orders, lr=1e-3):
    """(sums (3, 4) float64: heads x (N_train, N_val, Nn_train, Nn_val); weights (3,)) of GradBlend.get_weights() from `params`
    over `tensors` (the first `nval` rows val, the rest train), one training pass per entry of `orders`."""
    val, train = tuple(t[:nval] for t in tensors), tuple(t[nval:] for t in tensors)
    base = R.Step(case, params, lr)
    sums = torch.zeros(3, 4, dtype=torch.float64)
    sums[:, 0], sums[:, 1] = loss_sums(base, train, B), loss_sums(base, val, B)
    models = [ModalityStep(base, (0,)), ModalityStep(base, (1,)), S.FrozenStep(base)]
    for h, model in enumerate(models):
        for order in orders:
            for b in batches(train, B, order):
                model.step(b)
        sums[h, 2], sums[h, 3] = loss_sums(model, train, B)[h], loss_sums(model, val, B)[h]
    ws = [blend(*(float(x) for x in sums[h])) for h in range(3)]
    z = sum(ws)
    return sums, torch.tensor([w / z for w in ws], dtype=torch.float64)
